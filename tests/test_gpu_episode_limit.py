"""GPU parity of the episode step limit (include/mapf_hip.h mapf_set_episode_limit; VecMapfEnv.set_episode_limit): fused rollouts
and single steps under a limit against the composition of the unchanged C oracle in tests/episode_limit_cases.py -- cells, flags,
the float64 bit patterns of reward / prob / returns, ages and truncation counts, bit for bit.  Every bad input here is one the
host rejects: nothing provokes a device fault."""
import numpy as np
import pytest

import episode_limit_cases as ec
from conftest import set_tune
from gym_mapf_amd import _native as nat
from parity_checks import RECORDED, SOURCE_TAG, TOTALS, check_handle, check_record, check_totals, make, raw_bytes

pytestmark = pytest.mark.gpu


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


def _run_pass(w, N, slip, criteria, source, expect=(), **kw):
    """The 36 steps as launches of 5 (recording), 1 (totals only), 18 (accumulated into the 1's totals) and 12 (recording), then the
    12 twice more into the same arrays (out=: in device mode the second reuses the cached argument block); returns the outcome
    counts of the 36."""
    env, ref = make(w, N, slip, criteria, source, **kw)
    tag = (w.A, w.E, N, slip, criteria, source)

    def name(kind):
        got = env.last_kernel('rollout')
        assert 'LIMIT' in got and SOURCE_TAG[source] in got and kind in got and all(e in got for e in expect), (tag, got)

    res, refs5 = _rollout(env, ref, w, source, 5, record=True)
    name('RECORD')
    assert sorted(res) == sorted(RECORDED + TOTALS)
    check_record(res, refs5, tag)
    check_totals(res, ec.totals_of(refs5), tag)
    check_handle(env, ref, tag)
    res, refs1 = _rollout(env, ref, w, source, 1)
    name('TOTALS')
    assert sorted(res) == sorted(TOTALS)
    base = ec.totals_of(refs1)
    check_totals(res, base, tag)
    res, refs18 = _rollout(env, ref, w, source, 18, accumulate_into=res)
    check_totals(res, ec.totals_of(refs18, base), tag)
    check_handle(env, ref, tag)
    out, refs12 = _rollout(env, ref, w, source, 12, record=True)
    check_record(out, refs12, tag)
    check_totals(out, ec.totals_of(refs12), tag)
    check_handle(env, ref, tag)
    for again in range(2):
        got, more = _rollout(env, ref, w, source, 12, record=True, out=out)
        assert got is out
        name('RECORD')
        check_record(out, more, (tag, 'out=', again))
        check_totals(out, ec.totals_of(more), (tag, 'out=', again))
        if env.device_arrays and source != 'stream':
            assert env._rollout_io is not None
    check_handle(env, ref, tag)
    env.close()
    return ec.outcome_counts(refs5 + refs1 + refs18 + refs12)


PARITY_CASES = [(A, E, 'Makespan') for A, E in ec.SHAPES] + [(A, E, 'SoC') for A, E in ec.SHAPES if A in (3, 8)]


@pytest.mark.parametrize('A,E,criteria', PARITY_CASES)
def test_rollout_parity_over_forms(A, E, criteria):
    """every (N, slip) of the issue x the four action sources: L = 1, ghost slots, full groups, L = 16; ragged and whole batches"""
    L = max(1, 1 << ((A + 1) // 2 - 1).bit_length())
    for N, slip in ec.LIMITS:
        w = ec.Workload(A, E, N)
        for source in ec.SOURCES:
            counts = _run_pass(w, N, slip, criteria, source, expect=('L=%d,' % L, 'FULL' if A == 2 * L else 'RAGGED', 'MV_GLOBAL'))
            ec.check_outcomes(A, E, N, slip, source, counts)


# batches of at least 64 * 256 lanes: the move table is staged into LDS (the planner's rule); ragged last blocks
LDS_CASES = [(2, 16390), (3, 8200), (8, 4097), (32, 1030)]


@pytest.mark.parametrize('A,E', LDS_CASES)
def test_rollout_parity_with_the_move_table_in_lds_and_in_global_memory(monkeypatch, A, E):
    w = ec.Workload(A, E, 4)
    for mv_lds in (True, False):
        set_tune(monkeypatch, mv_lds_max_bytes=None if mv_lds else 0)
        for source in ec.SOURCES:
            goals, colls, truncs, _ = _run_pass(w, 4, 0.2, 'Makespan', source, expect=('MV_LDS' if mv_lds else 'MV_GLOBAL',))
            assert truncs > 0 and colls > 0 and (goals > 0 or source == 'policy')


def _step_outputs(local, reward, done, info):
    return dict(local=local, reward=reward, done=done, **info)


@pytest.mark.parametrize('A,E', ec.SHAPES)
def test_single_steps_with_device_philox_and_caller_uniforms(A, E):
    """12 steps of the table-driven family through step(), auto-reset on and off; ages after every step"""
    w = ec.Workload(A, E, 4)
    rs = np.random.RandomState(A * 1000 + E)
    for ext in (False, True):
        for auto_reset in (True, False):
            env, ref = make(w, 4, 0.2, source='stream')
            truncs = 0
            for t in range(12):
                actions = w.actions('stream', ref)
                uniforms = rs.rand(E, A) if ext else None
                got = _step_outputs(*env.step(actions, uniforms=uniforms, auto_reset=auto_reset))
                want = ref.step(actions, uniforms, auto_reset=auto_reset)
                name = env.last_kernel('step')
                assert 'LIMIT' in name and ('EXT_UNIFORMS' if ext else 'PHILOX') in name, name
                assert sorted(got) == sorted(RECORDED + ('was_terminal',))
                for key in RECORDED + ('was_terminal',):
                    assert np.array_equal(raw_bytes(got[key]), raw_bytes(want[key])), (A, E, ext, auto_reset, t, key)
                check_handle(env, ref, (A, E, ext, auto_reset, t))
                truncs += int(want['truncated'].sum())
            assert truncs > 0
            env.close()


@pytest.mark.parametrize('A,E', [(2, 37), (3, 64), (8, 37), (32, 64)])
def test_without_auto_reset_truncated_repeats_until_a_reset_and_reset_zeroes_the_masked_ages(A, E):
    w = ec.Workload(A, E, 3)
    env, ref = make(w, 3, 0.2, source='stream')
    seen, repeats = np.zeros(E, bool), 0
    for t in range(8):
        actions = w.actions('stream', ref)
        local, reward, done, info = env.step(actions, auto_reset=False)
        want = ref.step(actions, auto_reset=False)
        assert np.array_equal(info['truncated'], want['truncated']) and np.array_equal(done, want['done']), t
        later = seen & (info['was_terminal'] == 0) & (done == 0)
        assert (info['truncated'][later] == 1).all()              # a truncated env goes on living, and says so on every live step
        repeats += int(later.sum())
        seen |= info['truncated'] != 0
    assert repeats > 0
    # ... also inside a rollout without auto-reset, which continues the same ages
    refs = ref.run(w, 'stream', 4, auto_reset=False)
    res = env.rollout(4, actions=np.stack([r['actions'] for r in refs]).astype(np.uint8), auto_reset=False, record=True)
    assert 'LIMIT' in env.last_kernel('rollout')
    check_record(res, refs, 'no auto-reset')
    check_totals(res, ec.totals_of(refs), 'no auto-reset')
    check_handle(env, ref, 'no auto-reset')
    ages = env.episode_steps()
    mask = (np.arange(E) % 3 == 0).astype(np.uint8)
    env.reset(mask)
    after = env.episode_steps()
    assert not after[mask != 0].any() and np.array_equal(after[mask == 0], ages[mask == 0]) and ages[mask != 0].any()
    ref.reset(mask)
    check_handle(env, ref, 'reset(mask)')
    env.reset()
    assert not env.episode_steps().any()
    env.close()


@pytest.mark.parametrize('A,E', [(3, 37), (8, 4096), (32, 1024), (2, 64)])
def test_a_limit_never_reached_changes_nothing(A, E):
    """N = 2^31 against a handle without a limit under default dispatch (which may be a packed or a thread-per-env kernel)"""
    w = ec.Workload(A, E, 4)
    for source in ec.SOURCES:
        limited, _ = make(w, 1 << 31, 0.2, source=source)
        plain, ref = make(w, None, 0.2, source=source)
        actions = None
        if source == 'stream':
            actions = np.stack([r['actions'] for r in ref.run(w, source, ec.T_TOTAL)]).astype(np.uint8)
        a = limited.rollout(ec.T_TOTAL, actions=actions, record=True)
        b = plain.rollout(ec.T_TOTAL, actions=actions, record=True)
        assert 'LIMIT' in limited.last_kernel('rollout') and 'LIMIT' not in plain.last_kernel('rollout')
        assert sorted(b) == sorted(k for k in RECORDED + TOTALS if not k.startswith('trunc'))      # exactly today's keys
        for key in b:
            assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), (A, E, source, key)
        assert not a['truncations'].any() and not a['truncated'].any()
        assert np.array_equal(limited.get_state()[0], plain.get_state()[0]) and limited.t == plain.t
        assert not plain.episode_steps().any()
        limited.close()
        plain.close()


def test_mixed_calls_against_the_reference():
    """rollout, step, set_state(t=...), set_episode_limit (zeroes the ages), rollout, set_state(cells) (zeroes them too), rollout"""
    w = ec.Workload(8, 64, 4)
    env, ref = make(w, 4, 0.2, source='table')
    res, refs = _rollout(env, ref, w, 'table', 7, record=True)
    check_record(res, refs, 'first')
    for t in range(3):
        actions = w.actions('table', ref)
        got = _step_outputs(*env.step(actions, auto_reset=True))
        want = ref.step(actions, auto_reset=True)
        for key in RECORDED:
            assert np.array_equal(raw_bytes(got[key]), raw_bytes(want[key])), (t, key)
    assert ref.age.any()
    check_handle(env, ref, 'steps')
    env.set_state(t=1000)                                         # only t: the ages stay
    ref.co.t = 1000
    check_handle(env, ref, 'set_state(t)')
    res, refs = _rollout(env, ref, w, 'table', 3, record=True)
    check_record(res, refs, 'after set_state(t)')
    env.set_episode_limit(2)
    ref.set_limit(2)
    check_handle(env, ref, 'set_episode_limit')
    res, refs = _rollout(env, ref, w, 'table', 9, record=True)
    check_record(res, refs, 'second limit')
    check_totals(res, ec.totals_of(refs), 'second limit')
    cells = np.ascontiguousarray(ref.co.state[::-1])
    env.set_state(cells)                                          # cells: new episodes
    ref.co.state[:] = cells
    ref.age[:] = 0
    check_handle(env, ref, 'set_state(cells)')
    res, refs = _rollout(env, ref, w, 'table', 6, record=True)
    check_record(res, refs, 'after set_state(cells)')
    ages = np.arange(64, dtype=np.uint32) % 3
    assert np.array_equal(env.episode_steps(set=ages), ref.age)  # (returns the ages before the set)
    ref.age = ages.copy()
    res, refs = _rollout(env, ref, w, 'table', 5, record=True)
    check_record(res, refs, 'after episode_steps(set=)')
    check_handle(env, ref, 'end')
    env.set_episode_limit(None)                                   # off: today's keys, today's kernels
    out = env.rollout(4, record=True)
    assert 'LIMIT' not in env.last_kernel('rollout') and 'truncations' not in out and 'truncated' not in out
    assert 'truncated' not in env.step(w.actions('table', ref))[3]
    env.close()


def test_device_arrays_with_env_ids_beyond_32_bits():
    w = ec.Workload(8, 64, 4)
    for source in ec.SOURCES:
        counts = _run_pass(w, 4, 0.2, 'Makespan', source, device_arrays=True, env_id_offset=(1 << 32) + 5)
        assert counts[2] > 0
    # a handle with a limit is not recorded into a graph, and the limit is not changed under live graphs
    env, _ = make(w, 4, 0.2, source='table', device_arrays=True)
    with pytest.raises(nat.MapfNativeError) as err:
        env.graph_begin()
    assert err.value.code == nat.MAPF_EUNSUPPORTED
    env.set_episode_limit(0)
    env.graph_begin()
    kept = env.rollout(2)
    graph = env.graph_end()
    with pytest.raises(nat.MapfNativeError):
        env.set_episode_limit(4)
    assert env.episode_limit == 0
    graph.close()
    del kept
    env.set_episode_limit(4)
    env.close()


def test_the_c_abi_refuses_truncation_outputs_without_a_limit():
    import ctypes
    w = ec.Workload(3, 37, 4)
    env, _ = make(w, None, 0.2, source='policy')
    lib, E = env._lib, w.E
    buf = np.zeros(E, np.uint32)
    io = nat.MapfRolloutIO(struct_size=ctypes.sizeof(nat.MapfRolloutIO), n_steps=1)
    for beside in ((buf.ctypes.data, None), (None, buf.ctypes.data)):
        assert lib.mapf_rollout_limited(env._h, ctypes.byref(io), *beside) == nat.MAPF_EINVAL and b'episode limit' in lib.mapf_last_error()
    actions = np.zeros((E, 3), np.uint8)
    assert lib.mapf_step_limited(env._h, actions.ctypes.data, None, None, None, None, None, None, None, buf.ctypes.data, 0) == nat.MAPF_EINVAL
    assert lib.mapf_episode_steps(env._h, None, buf.ctypes.data) == nat.MAPF_EINVAL
    assert lib.mapf_episode_steps(env._h, None, None) == nat.MAPF_EINVAL
    assert env.last_kernel('rollout') == '' and env.last_kernel('step') == '' and env.t == 0
    with pytest.raises(ValueError):
        env.set_episode_limit(-1)
    with pytest.raises(ValueError):
        env.set_episode_limit(1 << 32)
    with pytest.raises(ValueError):
        env.set_episode_limit(2.5)
    env.close()
