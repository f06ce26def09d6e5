"""GPU parity of the conflict matrix (include/mapf_hip.h mapf_set_conflict_pairs; VecMapfEnv.set_conflict_pairs): fused rollouts that
count which agent pairs collide, against the composition over the unchanged C oracle in tests/conflict_pairs_cases.py -- the matrix
with array_equal on uint64 after every launch, and every other output of the launch both against the oracle and bit for bit against
a second handle with the mode off that runs the same launches.  Every bad input here is one the host rejects: nothing provokes a
device fault."""
import numpy as np
import pytest

import conflict_pairs_cases as pc
import episode_budget_cases as bc
import episode_limit_cases as ec
from conftest import set_tune
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import policies
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from parity_checks import SOURCE_TAG, make, raw_bytes, to_np

pytestmark = pytest.mark.gpu

SLOTS = ('one', 'mod3', 'per_env')


def _slots(kind, E):
    """(n_slots, slot of every env or None)"""
    return {'one': (1, None), 'mod3': (3, np.arange(E) % 3), 'per_env': (E, np.arange(E))}[kind]


def _handles(w, N, slip, B, criteria='Makespan', source='table', slots='one', **kw):
    """a handle that counts, a second one with the mode off, and the reference: under the limit N (0: none) and the budget B (0: none)"""
    n_slots, slot_of = _slots(slots, w.E)
    env, inner = make(w, N, slip, criteria, source, **kw)
    twin, _ = make(w, N, slip, criteria, source, **kw)
    if B:
        env.set_episode_budget(B)
        twin.set_episode_budget(B)
        inner = bc.BudgetOracle(inner, B)
    elif not N:
        inner = inner.co                                                    # neither: the plain C oracle
    env.set_conflict_pairs(n_slots, slot_of)
    assert env.conflict_slots == n_slots and twin.conflict_slots == 0
    return env, twin, pc.PairsOracle(inner, n_slots, slot_of)


def _keys(N, B, record):
    totals = ('returns', 'episodes', 'collisions') + (('truncations',) if N else ()) + (('live_steps',) if B else ())
    recorded = ('local', 'reward', 'prob', 'done', 'collision') + (('truncated',) if N else ())
    return totals, (recorded if record else ())


def _totals_of(refs, N, B, base=None):
    """the totals of the reference steps, added in step order (to `base` when a call accumulates); parked steps add nothing"""
    E = refs[0]['reward'].shape[0]
    tot = {k: np.zeros(E, np.float64 if k == 'returns' else np.uint32) for k in _keys(N, B, False)[0]} if base is None else {k: v.copy() for k, v in base.items()}
    for r in refs:
        parked = r.get('parked', np.zeros(E, bool))
        tot['returns'] = np.where(parked, tot['returns'], tot['returns'] + r['reward'])
        tot['episodes'] = tot['episodes'] + r['done'].astype(np.uint32)
        tot['collisions'] = tot['collisions'] + r['collision'].astype(np.uint32)
        if N:
            tot['truncations'] = tot['truncations'] + r['truncated'].astype(np.uint32)
        if B:
            tot['live_steps'] = tot['live_steps'] + r['live'].astype(np.uint32)
    return tot


def _rollout(env, twin, ref, w, source, n, auto_reset=True, into=None, **kw):
    """one launch of n steps on both handles and the reference's n steps (which run first: streamed actions are the reference's).
    `into`: the (counting handle's, twin's) dicts the launch accumulates into.  Returns (results of both handles, reference steps)"""
    refs = ref.run(w, source, n, auto_reset=auto_reset)
    got = []
    for k, h in enumerate((env, twin)):
        actions = None
        if source == 'stream':
            actions = np.stack([r['actions'] for r in refs]).astype(np.uint8)
            if h.device_arrays:
                import torch
                actions = torch.from_numpy(actions).to('cuda')
        more = dict(kw, accumulate_into=into[k]) if into is not None else kw
        got.append(h.rollout(n, actions=actions, auto_reset=auto_reset, **more))
        h.sync()
    return got, refs


def _check(env, twin, ref, got, refs, want, N, B, record, tag):
    """the matrix against the reference; every other output against the reference AND against the handle with the mode off"""
    res, plain = got
    totals, recorded = _keys(N, B, record)
    assert sorted(res) == sorted(plain) == sorted(totals + recorded), (tag, sorted(res))
    for key in recorded:
        for t, r in enumerate(refs):
            assert np.array_equal(raw_bytes(res[key][t]), raw_bytes(r[key])), (tag, key, t)
    for key in totals:
        assert np.array_equal(raw_bytes(res[key]), raw_bytes(want[key])), (tag, key)
    for key in res:
        assert np.array_equal(raw_bytes(res[key]), raw_bytes(plain[key])), (tag, key, 'mode on / mode off')
    M = env.conflict_pairs()
    env.sync()
    M = to_np(M)
    assert M.dtype == np.uint64 and M.shape == ref.M.shape and np.array_equal(M, ref.M), (tag, 'conflict matrix', int(M.sum()), int(ref.M.sum()))
    for h in (env, twin):
        local, ages, left = h.get_state()[0], h.episode_steps(), h.episodes_left()
        h.sync()
        assert np.array_equal(to_np(local), ref.co.state) and h.t == ref.co.t, tag
        assert not N or np.array_equal(to_np(ages), ref.age), tag
        assert not B or np.array_equal(to_np(left), ref.left), tag


def _run_pass(w, N, slip, B, criteria='Makespan', source='table', slots='one', expect=(), auto_reset=True, **kw):
    """The 36 steps as launches of 5 (recording), 1 (totals only), 18 (accumulated into the 1's totals) and 12 (recording); everything
    compared after every launch.  Returns the reference."""
    env, twin, ref = _handles(w, N, slip, B, criteria, source, slots, **kw)
    tag = (w.A, w.E, N, slip, B, criteria, source, slots, auto_reset)
    form = 'BUDGET' if B else ('LIMIT' if N else 'GUARDED')

    def name(kind):
        got, off = env.last_kernel('rollout'), twin.last_kernel('rollout')
        assert '_pairs<' in got and ',%s,PAIRS>' % form in got and SOURCE_TAG[source] in got and kind in got and all(e in got for e in expect), (tag, got)
        assert 'PAIRS' not in off and 'pairs' not in off, (tag, off)

    got, refs = _rollout(env, twin, ref, w, source, 5, auto_reset, record=True)
    name('RECORD')
    _check(env, twin, ref, got, refs, _totals_of(refs, N, B), N, B, True, tag)
    got, refs = _rollout(env, twin, ref, w, source, 1, auto_reset)
    name('TOTALS')
    base = _totals_of(refs, N, B)
    _check(env, twin, ref, got, refs, base, N, B, False, tag)
    got, refs = _rollout(env, twin, ref, w, source, 18, auto_reset, into=got)
    name('TOTALS')
    _check(env, twin, ref, got, refs, _totals_of(refs, N, B, base), N, B, False, tag)
    got, refs = _rollout(env, twin, ref, w, source, 12, auto_reset, record=True)
    name('RECORD')
    _check(env, twin, ref, got, refs, _totals_of(refs, N, B), N, B, True, tag)
    env.close()
    twin.close()
    return ref


def _group(A):
    L = max(1, 1 << ((A + 1) // 2 - 1).bit_length())
    return 'L=%d,' % L, 'FULL' if A == 2 * L else 'RAGGED'


# ------------------------------------------------------------------- the scripted family: the matrix's values
@pytest.mark.parametrize('A', pc.EVERY_PAIR_AGENTS)
def test_every_pair_counts_every_pair_once_as_vertex_and_once_as_swap(A):
    """L = 1, ghost slots at L = 2 and L = 4, full L = 4, 8 and 16, the rolled loop ragged and full, L = 64"""
    w = pc.every_pair(A)
    env = VecMapfEnv(w.grid, A, None, None, 0.0, *w.REWARDS, OptimizationCriteria.Makespan, seed=ec.ORACLE_SEED, start_local=w.start, goal_local=w.goal)
    actions = w.actions1[None]
    upper = np.triu(np.ones((A, A), np.uint64), 1)
    # one slot: ones off the diagonal; every other output of the step is the oracle's
    env.set_conflict_pairs()
    ref = w.oracle()
    r = ref.step(w.actions1, auto_reset=True)
    res = env.rollout(1, actions=actions, auto_reset=True, record=True)
    got = env.last_kernel('rollout')
    assert got.startswith('lg_rollout_kernel_pairs<') and ',GUARDED,PAIRS>' in got and all(e in got for e in _group(A)), got
    M = env.conflict_pairs()
    assert np.array_equal(M, w.expected()) and np.array_equal(M, ref.M), (A, M[0])
    for key in ('local', 'reward', 'prob', 'done', 'collision'):
        assert np.array_equal(raw_bytes(res[key][0]), raw_bytes(r[key])), (A, key)
    assert np.array_equal(raw_bytes(res['returns']), raw_bytes(0.0 + r['reward'])) and (res['collisions'] == 1).all() and (res['episodes'] == 1).all()
    assert np.array_equal(env.get_state()[0], ref.co.state) and env.t == 1
    # slots e % 2: slot 0 holds the upper triangle's ones (the vertex envs), slot 1 the lower triangle's
    env.reset()
    env.set_conflict_pairs(2, np.arange(w.E) % 2)
    env.rollout(1, actions=actions, auto_reset=True)
    M = env.conflict_pairs()
    assert np.array_equal(M[0], upper) and np.array_equal(M[1], upper.T), (A, M)
    if A <= 16:                                                             # one slot per env: one entry each, its own pair's
        env.reset()
        env.set_conflict_pairs(w.E, np.arange(w.E))
        env.rollout(1, actions=actions, auto_reset=True)
        M = env.conflict_pairs()
        want = np.zeros((w.E, A, A), np.uint64)
        for p, (i, j) in enumerate(w.pairs):
            want[2 * p, i, j] = want[2 * p + 1, j, i] = 1
        assert np.array_equal(M, want), A
    env.close()


# ------------------------------------------------------------------- random workloads: the matrix against PairsOracle
@pytest.mark.parametrize('slots', SLOTS)
@pytest.mark.parametrize('A,E', pc.SHAPES)
def test_rollout_parity_over_shapes_budgets_sources_and_slots(A, E, slots):
    """every (N, slip, B) of the budget's passes x the four action sources, recording and totals-only launches"""
    for N, slip, B in bc.PASSES:
        w = ec.Workload(A, E, N or 4)
        for source in ec.SOURCES:
            ref = _run_pass(w, N, slip, B, source=source, slots=slots, expect=_group(A) + ('MV_GLOBAL',))
            if A >= 5:
                assert np.triu(ref.M.sum(axis=0), 1).any() and np.tril(ref.M.sum(axis=0), -1).any(), (A, E, N, slip, B, source)


@pytest.mark.parametrize('slots', SLOTS)
def test_a_limit_without_a_budget_at_eight_agents(slots):
    w = ec.Workload(8, 64, 4)
    for source in ec.SOURCES:
        for auto_reset in (True, False):
            ref = _run_pass(w, 4, 0.2, 0, source=source, slots=slots, auto_reset=auto_reset)
            assert ref.M.any()


@pytest.mark.parametrize('auto_reset', [True, False])
def test_neither_limit_nor_budget_at_eight_agents(auto_reset):
    """without auto-reset the steps after a vertex conflict are terminal no-ops and add nothing (the reference skips them too)"""
    w = ec.Workload(8, 64, 4)
    for source in ec.SOURCES:
        for slots in SLOTS:
            ref = _run_pass(w, 0, 0.2, 0, source=source, slots=slots, auto_reset=auto_reset)
            assert ref.M.any()
    if not auto_reset:                                                      # ... and such no-ops exist: far fewer counts than with auto-reset
        stay = _run_pass(w, 0, 0.2, 0, source='policy', auto_reset=False)
        back = _run_pass(w, 0, 0.2, 0, source='policy', auto_reset=True)
        assert 0 < stay.M.sum() < back.M.sum()


def test_both_criteria_at_eight_agents():
    w = ec.Workload(8, 64, 4)
    for source in ec.SOURCES:
        _run_pass(w, 4, 0.2, 3, 'SoC', source, slots='mod3')
    _run_pass(w, 0, 0.2, 0, 'SoC', 'policy')


def test_the_move_table_in_lds_and_in_global_memory(monkeypatch):
    """a batch of at least 64 * 256 lanes stages the move table into LDS (the planner's rule); ragged last block"""
    w = ec.Workload(8, 4097, 4)
    for mv_lds in (True, False):
        set_tune(monkeypatch, mv_lds_max_bytes=None if mv_lds else 0)
        for source in ('table', 'stream'):
            ref = _run_pass(w, 4, 0.2, 3, source=source, slots='mod3', expect=('MV_LDS' if mv_lds else 'MV_GLOBAL',))
            assert ref.M.sum() > 1000


def test_kernel_names_with_and_without_the_matrix(monkeypatch):
    """PAIRS whatever the family flag and limit_packed, next to LIMIT or BUDGET; with the mode off again today's names and results"""
    w = ec.Workload(8, 512, 4)              # (k=4, limit_packed=1: tests/limit_packed_cases.py's packed limit case at this shape)
    for tune, kw in (({'k': 4, 'limit_packed': 1}, {}), ({}, {'kernel': 'lane_group'}), ({}, {'kernel': 'thread_per_env'}), ({}, {})):
        set_tune(monkeypatch, k=tune.get('k'), limit_packed=tune.get('limit_packed'))
        for N, B, want in ((4, 3, 'lg_rollout_kernel_table_budget_guarded_pairs<'), (4, 0, 'lg_rollout_kernel_table_limit_guarded_pairs<'),
                           (0, 0, 'lg_rollout_kernel_table_pairs<')):
            env, twin, ref = _handles(w, N, 0.2, B, **kw)
            got, refs = _rollout(env, twin, ref, w, 'table', 6)
            name, off = env.last_kernel('rollout'), twin.last_kernel('rollout')
            assert name.startswith(want) and ('BUDGET,PAIRS>' if B else ('LIMIT,PAIRS>' if N else 'GUARDED,PAIRS>')) in name, name
            assert 'PAIRS' not in off, off
            _check(env, twin, ref, got, refs, _totals_of(refs, N, B), N, B, False, (tune, kw, N, B))
            # the mode off again: the names and the results of a handle that never had it
            env.set_conflict_pairs(None)
            assert env.conflict_slots == 0
            for h in (env, twin):
                h.reset()
                h.set_state(t=0)
                if B:
                    h.set_episode_budget(B)
            a, b = env.rollout(6, auto_reset=True, record=True), twin.rollout(6, auto_reset=True, record=True)
            assert env.last_kernel('rollout') == twin.last_kernel('rollout') and 'PAIRS' not in env.last_kernel('rollout')
            if tune and not B:                                              # what routes to a packed kernel today still does
                assert env.last_kernel('rollout').startswith('lq_rollout_kernel_table_limit<' if N else 'lq_rollout_kernel_table<'), (N, env.last_kernel('rollout'))
            assert sorted(a) == sorted(b)
            for key in b:
                assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), key
            env.close()
            twin.close()


def test_two_shards_by_env_id_sum_to_the_whole_batch():
    """two device-pointer handles over the env id halves of a batch; the second half's ids lie beyond 2^32"""
    import torch
    w = ec.Workload(8, 64, 4)
    off, half = (1 << 32) - 32, 32
    whole, twin, ref = _handles(w, 4, 0.2, 3, source='policy', device_arrays=True, env_id_offset=off)
    parts = []
    for k in range(2):
        rows = slice(k * half, (k + 1) * half)
        h = VecMapfEnv(w.grid, w.A, None, None, 0.2, *ec.INEXACT, OptimizationCriteria.Makespan, seed=ec.ORACLE_SEED, start_local=w.start[rows],
                       goal_local=w.goal[rows], device_arrays=True, env_id_offset=off + k * half)
        h.set_episode_limit(4)
        h.set_episode_budget(3)
        h.set_conflict_pairs()
        parts.append(h)
    ref.run(w, 'policy', 20)
    kept = []                                                               # (the launches are only enqueued: their totals must outlive them)
    for h in [whole] + parts:
        kept.append(h.rollout(20, auto_reset=True))
        assert 'PAIRS' in h.last_kernel('rollout')
    M = [h.conflict_pairs() for h in [whole] + parts]
    torch.cuda.synchronize()
    M = [to_np(m) for m in M]
    assert M[1].any() and M[2].any()
    assert np.array_equal(M[0], ref.M), (int(M[0].sum()), int(ref.M.sum()))
    assert np.array_equal(M[1] + M[2], M[0]), (int(M[1].sum()), int(M[2].sum()), int(M[0].sum()))
    del kept
    for h in [whole, twin] + parts:
        h.close()


def test_reading_clearing_and_setting_again():
    w = ec.Workload(8, 64, 4)
    env, twin, ref = _handles(w, 4, 0.2, 10, source='policy', slots='mod3')
    _rollout(env, twin, ref, w, 'policy', 9)
    first = ref.take(zero=True)
    assert first.any()
    assert np.array_equal(env.conflict_pairs(zero=True), first)             # reads, then clears
    assert not env.conflict_pairs().any()
    _rollout(env, twin, ref, w, 'policy', 9)                               # the next launch counts from zero
    assert ref.M.any() and np.array_equal(env.conflict_pairs(), ref.M)
    out = np.full(ref.M.shape, 7, np.uint64)
    assert env.conflict_pairs(out=out) is out and np.array_equal(out, ref.M)
    assert env._lib.mapf_conflict_pairs(env._h, None, 1) == nat.MAPF_OK     # out == NULL is allowed with zero
    assert not env.conflict_pairs().any()
    # reset, set_state, the limit and the budget leave M alone
    ref.M[:] = 0
    _rollout(env, twin, ref, w, 'policy', 5)
    kept = ref.M.copy()
    assert kept.any()
    env.reset()
    env.set_state(t=3)
    env.set_episode_limit(4)
    env.set_episode_budget(3)
    assert np.array_equal(env.conflict_pairs(), kept)
    env.set_conflict_pairs(1)                                               # every call zeroes M (and here regroups the envs)
    assert env.conflict_pairs().shape == (1, 8, 8) and not env.conflict_pairs().any()
    env.set_conflict_pairs(0)                                               # off: today's names
    twin.reset()
    twin.set_state(t=3)
    twin.set_episode_limit(4)
    twin.set_episode_budget(3)
    a, b = env.rollout(4, auto_reset=True), twin.rollout(4, auto_reset=True)
    assert env.last_kernel('rollout') == twin.last_kernel('rollout') and 'PAIRS' not in env.last_kernel('rollout')
    for key in b:
        assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), key
    with pytest.raises(ValueError):
        env.conflict_pairs()
    env.close()
    twin.close()


def test_refusals():
    w = ec.Workload(3, 37, 4)
    env, _ = make(w, 4, 0.2, 'Makespan', 'policy')
    lib, E = env._lib, w.E
    out = np.zeros(9, np.uint64)
    # the mode off: nothing to read or clear
    assert lib.mapf_conflict_pairs(env._h, out.ctypes.data, 0) == nat.MAPF_EINVAL and b'no conflict matrix' in lib.mapf_last_error()
    assert lib.mapf_conflict_pairs(env._h, None, 1) == nat.MAPF_EINVAL
    # a slot beyond n_slots, an oversize matrix: nothing is allocated, the mode stays off
    slots = np.zeros(E, np.uint32)
    slots[E - 1] = 2
    assert lib.mapf_set_conflict_pairs(env._h, 2, slots.ctypes.data) == nat.MAPF_EINVAL and b'not below n_slots' in lib.mapf_last_error()
    assert lib.mapf_set_conflict_pairs(env._h, (1 << 30) // (9 * 8) + 1, None) == nat.MAPF_EINVAL and b'2^30' in lib.mapf_last_error()
    assert lib.mapf_set_conflict_pairs(env._h, 0xFFFFFFFF, None) == nat.MAPF_EINVAL
    assert lib.mapf_conflict_pairs(env._h, out.ctypes.data, 0) == nat.MAPF_EINVAL
    with pytest.raises(nat.MapfNativeError):
        env.set_conflict_pairs(2, slots)
    for bad in (-1, 1 << 32, 2.5, True):
        with pytest.raises(ValueError):
            env.set_conflict_pairs(bad)
    for bad in (np.zeros(E + 1, np.uint32), -np.ones(E, np.int64), np.zeros(E)):
        with pytest.raises(ValueError):
            env.set_conflict_pairs(2, bad)
    assert env.conflict_slots == 0 and env.last_kernel('rollout') == ''
    slots[E - 1] = 1
    env.set_conflict_pairs(2, slots)                                        # (the largest slot allowed)
    assert lib.mapf_conflict_pairs(env._h, None, 0) == nat.MAPF_EINVAL and b'out is null' in lib.mapf_last_error()
    # the single step counts nothing and stays as it is
    actions = np.zeros((E, 3), np.uint8)
    env.step(actions, auto_reset=True)
    assert 'PAIRS' not in env.last_kernel('step') and not env.conflict_pairs().any()
    env.close()
    dev, _ = make(w, None, 0.2, 'Makespan', 'policy', device_arrays=True)
    dev.set_conflict_pairs()
    with pytest.raises(nat.MapfNativeError) as err:
        dev.graph_begin()
    assert err.value.code == nat.MAPF_EUNSUPPORTED
    dev.set_conflict_pairs(0)
    dev.graph_begin()
    with pytest.raises(nat.MapfNativeError) as err:
        dev.set_conflict_pairs()                                            # not while recording
    assert err.value.code == nat.MAPF_EINVAL
    kept = dev.rollout(2)
    graph = dev.graph_end()
    with pytest.raises(nat.MapfNativeError):
        dev.set_conflict_pairs()                                            # not under live graphs, as the limit
    assert dev.conflict_slots == 0
    graph.close()
    del kept
    dev.set_conflict_pairs()
    dev.close()


@pytest.mark.parametrize('device_arrays', [False, True])
def test_policies_evaluate_returns_the_matrix_of_the_run_to_all_parked(device_arrays):
    w = ec.Workload(8, 64, 4)
    env, _ = make(w, None, 0.2, 'Makespan', 'table', device_arrays=device_arrays)
    plain = policies.evaluate(env, 3, 4, chunk=5)                           # the mode off: today's keys
    assert sorted(plain) == ['collisions', 'goal_ends', 'live_steps', 'returns', 'truncations']
    env.set_conflict_pairs(3, np.arange(w.E) % 3)
    env.set_episode_budget(3)                                               # (the first evaluate left every env parked)
    warm = env.rollout(12, auto_reset=True)                                 # counts that evaluate must not report
    before = env.conflict_pairs()
    env.sync()
    assert to_np(before).any()
    del warm
    got = policies.evaluate(env, 3, 4, chunk=5)
    assert 'BUDGET,PAIRS>' in env.last_kernel('rollout')
    assert sorted(got) == ['collisions', 'goal_ends', 'live_steps', 'pair_conflicts', 'returns', 'truncations']
    ref = pc.PairsOracle(bc.oracle(w, 4, 0.2, 3), 3, np.arange(w.E) % 3)
    ref.co.t = env.t - 15                                                   # (evaluate resets the cells, not the step index)
    want = bc.totals_of(ref.run(w, 'table', 15))
    assert not ref.left.any()
    assert got['pair_conflicts'].dtype == np.uint64 and np.array_equal(got['pair_conflicts'], ref.M) and ref.M.any()
    for key in ('returns', 'collisions', 'truncations', 'live_steps'):
        assert np.array_equal(raw_bytes(got[key]), raw_bytes(want[key])), key
    # a count per collision-ended episode at least; the helpers read the matrix
    both = policies.conflicts(got['pair_conflicts'])
    assert both.shape == (3, 8, 8) and np.array_equal(both, np.swapaxes(both, 1, 2)) and int(both.sum()) == 2 * int(ref.M.sum())
    assert int(ref.M.sum()) >= int(want['collisions'].sum())
    rows = policies.conflicting_pairs(got['pair_conflicts'])
    total = ref.M.sum(axis=0)
    assert rows == sorted(rows) and all(i < j and (v, s) == (int(total[i, j]), int(total[j, i])) and v + s > 0 for i, j, v, s in rows)
    assert sum(v + s for _, _, v, s in rows) == int(ref.M.sum())
    env.close()
