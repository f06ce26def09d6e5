"""GPU parity of the episode budget (include/mapf_hip.h mapf_set_episode_budget; VecMapfEnv.set_episode_budget): fused rollouts that
stop each env after n episodes against the composition over the unchanged C oracle in tests/episode_budget_cases.py -- recorded rows,
the float64 bit patterns of reward / prob / returns, the totals with live_steps, ages, episodes left, cells and the step index, bit
for bit after every launch.  Every bad input here is one the host rejects: nothing provokes a device fault."""
import ctypes

import numpy as np
import pytest

import episode_budget_cases as bc
import episode_limit_cases as ec
from conftest import set_tune
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import policies
from parity_checks import SOURCE_TAG, make, raw_bytes, to_np

pytestmark = pytest.mark.gpu


def _budgeted(w, N, slip, B, criteria='Makespan', source='table', **kw):
    """a handle under the limit N (0: none) and the budget B, and its reference"""
    env, lim = make(w, N, slip, criteria, source, **kw)
    env.set_episode_budget(B)
    assert env.episode_budget == B
    return env, bc.BudgetOracle(lim, B)


def _keys(N, record):
    totals = tuple(k for k in bc.TOTALS if N or k != 'truncations')
    return totals, (tuple(k for k in bc.RECORDED if N or k != 'truncated') if record else ())


def _rollout(env, ref, w, source, n, **kw):
    """one launch of n steps and the reference's n steps (streamed: the reference runs first, its actions are what is streamed)"""
    refs = ref.run(w, source, n) if source == 'stream' else None
    actions = None
    if source == 'stream':
        actions = np.stack([r['actions'] for r in refs]).astype(np.uint8)
        if env.device_arrays:
            import torch
            actions = torch.from_numpy(actions).to('cuda')
    res = env.rollout(n, actions=actions, auto_reset=True, **kw)
    env.sync()
    return res, (refs if refs is not None else ref.run(w, source, n))


def _check(env, ref, res, refs, want, N, record, tag):
    totals, recorded = _keys(N, record)
    assert sorted(res) == sorted(totals + recorded), (tag, sorted(res))
    for key in recorded:
        for t, r in enumerate(refs):
            assert np.array_equal(raw_bytes(res[key][t]), raw_bytes(r[key])), (tag, key, t)
    for key in totals:
        assert np.array_equal(raw_bytes(res[key]), raw_bytes(want[key])), (tag, key)
    local, ages, left = env.get_state()[0], env.episode_steps(), env.episodes_left()
    env.sync()
    assert np.array_equal(to_np(local), ref.co.state) and np.array_equal(to_np(ages), ref.age) and np.array_equal(to_np(left), ref.left), tag
    assert env.t == ref.co.t, tag


def _run_pass(w, N, slip, B, criteria='Makespan', source='table', expect=(), **kw):
    """The 36 steps as launches of 5 (recording), 1 (totals only), 18 (accumulated into the 1's totals) and 12 (recording), then the 12
    once more into the same arrays (out=); everything compared after every launch.  Returns the reference."""
    env, ref = _budgeted(w, N, slip, B, criteria, source, **kw)
    tag = (w.A, w.E, N, slip, B, criteria, source)

    def name(kind):
        got = env.last_kernel('rollout')
        assert 'BUDGET' in got and '_budget_guarded<' in got and SOURCE_TAG[source] in got and kind in got and all(e in got for e in expect), (tag, got)

    res, refs = _rollout(env, ref, w, source, 5, record=True)
    name('RECORD')
    _check(env, ref, res, refs, bc.totals_of(refs), N, True, tag)
    res, refs = _rollout(env, ref, w, source, 1)
    name('TOTALS')
    base = bc.totals_of(refs)
    _check(env, ref, res, refs, base, N, False, tag)
    res, refs = _rollout(env, ref, w, source, 18, accumulate_into=res)
    name('TOTALS')
    _check(env, ref, res, refs, bc.totals_of(refs, base), N, False, tag)
    out, refs = _rollout(env, ref, w, source, 12, record=True)
    _check(env, ref, out, refs, bc.totals_of(refs), N, True, tag)
    got, refs = _rollout(env, ref, w, source, 12, record=True, out=out)
    assert got is out
    name('RECORD')
    _check(env, ref, out, refs, bc.totals_of(refs), N, True, (tag, 'out='))
    env.close()
    return ref


@pytest.mark.parametrize('A,E', bc.SHAPES)
def test_rollout_parity_over_shapes_budgets_and_sources(A, E):
    """every (N, slip, B) of the issue x the four action sources: L = 1, ghost slots, full groups, L = 16; ragged and whole batches"""
    L = max(1, 1 << ((A + 1) // 2 - 1).bit_length())
    for N, slip, B in bc.PASSES:
        w = ec.Workload(A, E, N or 4)
        for source in ec.SOURCES:
            ref = _run_pass(w, N, slip, B, source=source, expect=('L=%d,' % L, 'FULL' if A == 2 * L else 'RAGGED', 'MV_GLOBAL'))
            if B == 3:
                assert (ref.left == 0).all()


def test_both_criteria_at_eight_agents():
    w = ec.Workload(8, 64, 4)
    for source in ec.SOURCES:
        _run_pass(w, 4, 0.2, 3, 'SoC', source)


def test_the_move_table_in_lds_and_in_global_memory(monkeypatch):
    """a batch of at least 64 * 256 lanes stages the move table into LDS (the planner's rule); ragged last block"""
    w = ec.Workload(8, 4097, 4)
    for mv_lds in (True, False):
        set_tune(monkeypatch, mv_lds_max_bytes=None if mv_lds else 0)
        for source in ('table', 'stream'):
            ref = _run_pass(w, 4, 0.2, 3, source=source, expect=('MV_LDS' if mv_lds else 'MV_GLOBAL',))
            assert (ref.left == 0).sum() > 3000


def test_device_arrays_with_env_ids_beyond_32_bits():
    w = ec.Workload(8, 64, 4)
    for source in ec.SOURCES:
        _run_pass(w, 4, 0.2, 3, source=source, device_arrays=True, env_id_offset=(1 << 32) + 5)


def test_an_accumulated_negative_zero_survives_parked_steps():
    w = ec.Workload(3, 37, 4)
    env, ref = _budgeted(w, 4, 0.2, 1)
    res, refs = _rollout(env, ref, w, 'table', 8)
    assert not env.episodes_left().any()
    base = {k: (np.full(w.E, -0.0) if k == 'returns' else np.zeros(w.E, np.uint32)) for k in bc.TOTALS}
    res, refs = _rollout(env, ref, w, 'table', 3, accumulate_into={k: v.copy() for k, v in base.items()})
    _check(env, ref, res, refs, bc.totals_of(refs, base), 4, False, 'parked')
    assert np.signbit(res['returns']).all()
    env.close()


def test_rearming_single_envs_and_all_of_them():
    w = ec.Workload(8, 64, 4)
    env, ref = _budgeted(w, 4, 0.2, 3)
    per_env = (1 + np.arange(w.E) % 5).astype(np.uint32)
    assert np.array_equal(env.episodes_left(set=per_env), ref.left)          # (returns the counts before the set)
    ref.left = per_env.copy()
    assert np.array_equal(env.episodes_left(), per_env)
    res, refs = _rollout(env, ref, w, 'table', 7, record=True)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, True, 'per-env budgets')
    # mapf_reset(mask) leaves the counts alone (and zeroes the masked ages, as under the limit)
    mask = (np.arange(w.E) % 3 == 0).astype(np.uint8)
    env.reset(mask)
    ref.lim.reset(mask)
    assert np.array_equal(env.episodes_left(), ref.left)
    res, refs = _rollout(env, ref, w, 'table', 30)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, False, 'to all parked')
    assert not ref.left.any()
    env.set_episode_budget(2)                                               # re-arms every env; cells and ages stay
    ref.set_budget(2)
    assert (env.episodes_left() == 2).all()
    for n in (4, 9):
        res, refs = _rollout(env, ref, w, 'table', n, record=True)
        _check(env, ref, res, refs, bc.totals_of(refs), 4, True, ('re-armed', n))
    assert not ref.left.any()
    env.close()


def test_kernel_names_with_and_without_a_budget(monkeypatch):
    """BUDGET whatever the family flag and limit_packed; with the budget switched off again the limit instance and its results"""
    w = ec.Workload(8, 512, 4)              # (k=4, limit_packed=1: tests/limit_packed_cases.py's packed limit case at this shape)
    for tune, kw in (({'k': 4, 'limit_packed': 1}, {}), ({}, {'kernel': 'lane_group'}), ({}, {})):
        set_tune(monkeypatch, k=tune.get('k'), limit_packed=tune.get('limit_packed'))
        env, ref = _budgeted(w, 4, 0.2, 3, **kw)
        res, refs = _rollout(env, ref, w, 'table', 6)
        got = env.last_kernel('rollout')
        assert got.startswith('lg_rollout_kernel_table_budget_guarded<') and 'BUDGET' in got and 'episode budget' in got, got
        _check(env, ref, res, refs, bc.totals_of(refs), 4, False, (tune, kw))
        env.set_episode_budget(None)
        assert env.episode_budget == 0
        plain, lim = make(w, 4, 0.2, 'Makespan', 'table', **kw)
        env.reset()
        env.set_state(t=0)
        a, b = env.rollout(6, record=True), plain.rollout(6, record=True)
        assert 'BUDGET' not in env.last_kernel('rollout') and env.last_kernel('rollout') == plain.last_kernel('rollout')
        assert ('lq_rollout_kernel_table_limit' in env.last_kernel('rollout')) == bool(tune)
        assert sorted(a) == sorted(b) and 'live_steps' not in a
        for key in b:
            assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), key
        env.close()
        plain.close()


def test_refusals_under_a_budget():
    w = ec.Workload(3, 37, 4)
    env, _ = make(w, 4, 0.2, 'Makespan', 'policy')
    lib, E = env._lib, w.E
    buf = np.zeros(E, np.uint32)
    io = nat.MapfRolloutIO(struct_size=ctypes.sizeof(nat.MapfRolloutIO), n_steps=1, step_flags=nat.MAPF_STEP_AUTO_RESET)
    # without a budget: no live steps, no per-env counts to set
    assert lib.mapf_rollout_budgeted(env._h, ctypes.byref(io), None, None, buf.ctypes.data) == nat.MAPF_EINVAL and b'out_live_steps' in lib.mapf_last_error()
    assert lib.mapf_episodes_left(env._h, None, buf.ctypes.data) == nat.MAPF_EINVAL and b'set_left' in lib.mapf_last_error()
    assert lib.mapf_episodes_left(env._h, None, None) == nat.MAPF_EINVAL
    assert not env.episodes_left().any()
    env.set_episode_budget(2)
    io.step_flags = 0
    assert lib.mapf_rollout_budgeted(env._h, ctypes.byref(io), None, None, buf.ctypes.data) == nat.MAPF_EINVAL and b'MAPF_STEP_AUTO_RESET' in lib.mapf_last_error()
    assert lib.mapf_rollout(env._h, ctypes.byref(io)) == nat.MAPF_EINVAL
    with pytest.raises(ValueError):
        env.rollout(2, auto_reset=False)
    actions = np.zeros((E, 3), np.uint8)
    assert lib.mapf_step(env._h, actions.ctypes.data, None, None, None, None, None, None, None, 0) == nat.MAPF_EUNSUPPORTED
    assert lib.mapf_step_limited(env._h, actions.ctypes.data, None, None, None, None, None, None, None, None, 0) == nat.MAPF_EUNSUPPORTED
    assert env.last_kernel('rollout') == '' and env.last_kernel('step') == '' and env.t == 0
    assert (env.episodes_left() == 2).all()
    env.set_episode_limit(0)                                                # the truncation outputs need a limit, as without a budget
    io.step_flags = nat.MAPF_STEP_AUTO_RESET
    assert lib.mapf_rollout_budgeted(env._h, ctypes.byref(io), buf.ctypes.data, None, None) == nat.MAPF_EINVAL and b'episode limit' in lib.mapf_last_error()
    assert (env.episodes_left() == 2).all()                                 # mapf_set_episode_limit leaves the counts alone
    for bad in (-1, 1 << 32, 2.5, True):
        with pytest.raises(ValueError):
            env.set_episode_budget(bad)
    env.close()
    dev, _ = make(w, 4, 0.2, 'Makespan', 'policy', device_arrays=True)
    dev.set_episode_budget(2)
    with pytest.raises(nat.MapfNativeError) as err:
        dev.graph_begin()
    assert err.value.code == nat.MAPF_EUNSUPPORTED
    dev.set_episode_budget(0)
    dev.set_episode_limit(0)
    dev.graph_begin()
    kept = dev.rollout(2)
    graph = dev.graph_end()
    with pytest.raises(nat.MapfNativeError):
        dev.set_episode_budget(3)                                           # not under live graphs, as the limit
    assert dev.episode_budget == 0
    graph.close()
    del kept
    dev.set_episode_budget(3)
    dev.close()


@pytest.mark.parametrize('device_arrays', [False, True])
def test_policies_evaluate_against_the_oracle_run_to_all_parked(device_arrays):
    w = ec.Workload(8, 64, 4)
    env, _ = make(w, None, 0.2, 'Makespan', 'table', device_arrays=device_arrays)
    got = policies.evaluate(env, 3, 4, chunk=5)                             # ceil(12 / 5) = 3 launches of 5
    assert env.t == 15 and 'BUDGET' in env.last_kernel('rollout') and (env.episode_limit, env.episode_budget) == (4, 3)
    ref = bc.oracle(w, 4, 0.2, 3)
    want = bc.totals_of(ref.run(w, 'table', 15))
    assert not ref.left.any()
    assert sorted(got) == ['collisions', 'goal_ends', 'live_steps', 'returns', 'truncations']
    for key in ('returns', 'collisions', 'truncations', 'live_steps'):
        assert np.array_equal(raw_bytes(got[key]), raw_bytes(want[key])), key
    assert np.array_equal(got['goal_ends'], want['episodes'] - want['collisions'])
    assert (got['goal_ends'] + got['collisions'] + got['truncations'] == 3).all()
    env.close()
