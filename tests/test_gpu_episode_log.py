"""GPU parity of the episode log (include/mapf_hip.h mapf_set_episode_log; VecMapfEnv.set_episode_log): fused rollouts that record
every finished episode per env against the composition in tests/episode_log_cases.py -- records and counts bit for bit (the float64
bit patterns of the returns), and everything else of the launch -- recorded rows, totals with live_steps, ages, episodes left,
cells, the step index, the conflict matrix -- bit for bit what the mode-off reference gives.  Every bad input here is one the host
rejects: nothing provokes a device fault."""
import numpy as np
import pytest

import conflict_pairs_cases as pc
import episode_budget_cases as bc
import episode_limit_cases as ec
import episode_log_cases as lc
import joint_policy_cases as jc
from conftest import set_tune
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import policies
from parity_checks import SOURCE_TAG, make, raw_bytes, to_np

pytestmark = pytest.mark.gpu

# bc.SHAPES and two teams beyond them, so that every group size L = 1 .. 64 runs once
SHAPES = bc.SHAPES + ((64, 5), (128, 3))
SOURCES = ec.SOURCES + ('joint',)
TAGS = dict(SOURCE_TAG, joint='JOINT')
# (N, slip, B, C): a log that overflows in every env (C = 2 under B = 3), one that holds every episode and does not fill (C = B = 10)
PASSES = ((4, 0.2, 3, 2), (4, 0.2, 10, 10))


class OnePair:
    """The workload's per-agent shortest-path plan with ONE merged pair: agents 0 and 1 follow a random [V, V] table each, shared
    by all envs; every other agent keeps its own row."""

    def __init__(self, w):
        V, A, E = w.table.shape[1], w.A, w.E
        rs = np.random.RandomState(7 * A + E)
        pair = rs.randint(0, 5, size=2 * V * V).astype(np.uint8)
        self.table = np.concatenate([w.table.ravel(), pair])
        offsets = w.rows.astype(np.int64) * V
        offsets[:, 0], offsets[:, 1] = w.table.size, w.table.size + V * V
        partners = np.tile(np.arange(A), (E, 1))
        partners[:, 0], partners[:, 1] = 1, 0
        self.offsets, self.partners, self.V = offsets.astype(np.uint32), partners.astype(np.uint16), V

    def plan(self):
        return dict(table=self.table, offsets=self.offsets, partners=self.partners)


_workloads = {}


def workload(A, E, N=4):
    """(computed once, shared, left unchanged) the budget tests' workload with the one-pair joint plan beside it"""
    if (A, E, N) not in _workloads:
        w = ec.Workload(A, E, N)
        w.one_pair = OnePair(w)
        shared = w.actions
        w.actions = lambda source, ref, w=w, shared=shared: (jc.joint_actions(w.one_pair.table, w.one_pair.offsets, w.one_pair.partners, ref.co.state, w.one_pair.V)
                                                              if source == 'joint' else shared(source, ref))
        _workloads[A, E, N] = w
    return _workloads[A, E, N]


def _logged(w, N, slip, B, C, source='table', pairs=None, **kw):
    """a handle under the limit N (0: none), the budget B and a log of capacity C (with a conflict matrix: pairs = (n_slots, slots)),
    and its reference"""
    env, lim = make(w, N, slip, 'Makespan', 'policy' if source == 'joint' else source, **kw)
    if source == 'joint':
        env.set_policy('joint', **w.one_pair.plan())
    env.set_episode_budget(B)
    inner = bc.BudgetOracle(lim, B)
    if pairs is not None:
        env.set_conflict_pairs(*pairs)
        inner = pc.PairsOracle(inner, *pairs)
    env.set_episode_log(C)
    assert env.episode_log_capacity == C
    return env, lc.LogOracle(inner, C)


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


def _records(got):
    rec = to_np(got['records'])
    return np.ascontiguousarray(rec).view(lc.RECORD).reshape(rec.shape[:2]) if rec.dtype == np.uint8 else rec


def _check_log(env, ref, tag, clear=False):
    got = env.episode_log(clear=clear)
    env.sync()
    rec = _records(got)
    assert rec.shape == (ref.co.E, ref.C) and np.array_equal(to_np(got['count']), ref.count), (tag, to_np(got['count']), ref.count)
    assert np.array_equal(raw_bytes(rec), raw_bytes(ref.records)), (tag, 'records')
    # the columns are the records' fields
    assert np.array_equal(raw_bytes(got['returns']), raw_bytes(ref.records['ret'])) and np.array_equal(to_np(got['steps']), ref.records['steps']), tag
    assert np.array_equal(to_np(got['outcome']), ref.records['outcome'].astype(np.uint8)), tag
    if clear:
        ref.clear()


def _check(env, ref, res, refs, want, N, record, tag):
    """everything but the log against the mode-off reference, then the log against its own"""
    totals = tuple(k for k in bc.TOTALS if N or k != 'truncations')
    recorded = tuple(k for k in bc.RECORDED if N or k != 'truncated') if record else ()
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
    if env.conflict_slots:
        M = env.conflict_pairs()
        env.sync()
        assert np.array_equal(to_np(M), ref.M), (tag, 'conflict matrix')
    _check_log(env, ref, tag)


def _run_pass(w, N, slip, B, C, source='table', expect=(), pairs=None, **kw):
    """The 36 steps as launches of 5 (recording), 1 (totals only), 18 (accumulated into the 1's totals) and 12 (recording); everything
    compared after every launch.  Returns the reference."""
    env, ref = _logged(w, N, slip, B, C, source, pairs, **kw)
    tag = (w.A, w.E, N, slip, B, C, source)

    def name(kind):
        got = env.last_kernel('rollout')
        family = '_budget_guarded_log_pairs<' if pairs else '_budget_guarded_log<'
        assert ',BUDGET,LOG' in got and family in got and TAGS[source] in got and kind in got and all(e in got for e in expect), (tag, got)

    res, refs = _rollout(env, ref, w, source, ec.LAUNCHES[0], record=True)
    name('RECORD')
    _check(env, ref, res, refs, bc.totals_of(refs), N, True, tag)
    res, refs = _rollout(env, ref, w, source, ec.LAUNCHES[1])
    name('TOTALS')
    base = bc.totals_of(refs)
    _check(env, ref, res, refs, base, N, False, tag)
    res, refs = _rollout(env, ref, w, source, ec.LAUNCHES[2], accumulate_into=res)
    name('TOTALS')
    _check(env, ref, res, refs, bc.totals_of(refs, base), N, False, tag)
    res, refs = _rollout(env, ref, w, source, ec.LAUNCHES[3], record=True)
    name('RECORD')
    _check(env, ref, res, refs, bc.totals_of(refs), N, True, tag)
    env.close()
    return ref


def _group(A):
    L = max(1, 1 << ((A + 1) // 2 - 1).bit_length())
    return ('L=%d,' % L, 'FULL' if A == 2 * L else 'RAGGED')


@pytest.mark.parametrize('A,E', SHAPES)
def test_log_parity_over_group_sizes_sources_and_capacities(A, E):
    """every source across the four launches, totals-only and recording; C = 2 under B = 3 overflows everywhere, C = B = 10 does not fill"""
    w = workload(A, E)
    for N, slip, B, C in PASSES:
        for source in SOURCES:
            ref = _run_pass(w, N, slip, B, C, source=source, expect=_group(A) + ('MV_GLOBAL',))
            if B == 3:
                assert (ref.count == 3).all() and C < 3
    assert (ref.count <= 10).all()


@pytest.mark.parametrize('A,E', ((2, 37), (8, 64)))
def test_a_budget_without_a_limit_and_no_slip(A, E):
    """the other two passes of the budget tests: N = 0 (nothing truncates, the ages stay zero) and slip 0 under N = 2"""
    for N, slip, B in ((0, 0.2, 2), (2, 0.0, 3)):
        w = workload(A, E, N or 4)
        for source in ('table', 'stream'):
            _run_pass(w, N, slip, B, B, source=source)


def test_the_move_table_in_global_memory_by_tuning_and_in_lds(monkeypatch):
    """mv_lds_max_bytes=0 keeps the table in global memory; a batch of 64 * 256 lanes stages it into LDS beside the log's block"""
    small = workload(8, 64)
    set_tune(monkeypatch, mv_lds_max_bytes=0)
    _run_pass(small, 4, 0.2, 3, 2, source='table', expect=('MV_GLOBAL',))
    w = workload(8, 4097)
    for mv_lds in (True, False):
        set_tune(monkeypatch, mv_lds_max_bytes=None if mv_lds else 0)
        for source, pairs in (('table', None), ('stream', (1, None))):
            ref = _run_pass(w, 4, 0.2, 3, 2, source=source, pairs=pairs, expect=('MV_LDS' if mv_lds else 'MV_GLOBAL',))
            assert (ref.count == 3).all()


@pytest.mark.parametrize('A,E', ((3, 64), (8, 64), (32, 64)))
def test_with_the_conflict_matrix_on(A, E):
    w = workload(A, E)
    for source, pairs in (('table', (1, None)), ('joint', (E, np.arange(E))), ('policy', (1, None))):
        ref = _run_pass(w, 4, 0.2, 10, 10, source=source, pairs=pairs, expect=(',PAIRS>',))
        assert ref.M.any() or source == 'table'


def test_a_clear_between_launches_logs_the_spanning_episode_whole():
    w = workload(8, 64)
    env, ref = _logged(w, 4, 0.2, 10, 10)
    res, refs = _rollout(env, ref, w, 'table', 5)
    spanning = ref.len > 0
    assert spanning.sum() >= 4
    acc, steps = ref.acc.copy(), ref.len.copy()
    _check_log(env, ref, 'before the clear', clear=True)
    assert not ref.count.any() and np.array_equal(ref.len, steps)
    _check_log(env, ref, 'cleared')
    res, refs = _rollout(env, ref, w, 'table', 4)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, False, 'after the clear')
    first = ref.records[:, 0]
    assert (ref.count[spanning] >= 1).all() and (first['steps'][spanning] > steps[spanning]).all()      # whole: the steps before the clear count
    assert (first['ret'][spanning] != acc[spanning]).all()
    env.close()


def test_reset_and_set_state_drop_the_partials():
    w = workload(8, 64)
    env, ref = _logged(w, 4, 0.2, 10, 10)
    res, refs = _rollout(env, ref, w, 'table', 5)
    assert (ref.len > 0).sum() >= 4
    mask = (np.arange(w.E) % 3 == 0).astype(np.uint8)
    assert (ref.len[mask != 0] > 0).any() and (ref.len[mask == 0] > 0).any()
    env.reset(mask)
    ref.reset(mask)
    res, refs = _rollout(env, ref, w, 'table', 6, record=True)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, True, 'after reset(mask)')
    res, refs = _rollout(env, ref, w, 'table', 2)
    assert (ref.len > 0).any()
    cells = np.ascontiguousarray(w.start[::-1])                              # (other cells for every env, in mid-episode)
    env.set_state(cells)
    ref.set_state(cells)
    res, refs = _rollout(env, ref, w, 'table', 7, record=True)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, True, 'after set_state')
    env.reset()
    ref.reset()
    res, refs = _rollout(env, ref, w, 'table', 3)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, False, 'after reset()')
    env.close()


def test_rearming_keeps_the_partials_and_the_log():
    w = workload(8, 64)
    env, ref = _logged(w, 4, 0.2, 3, 6)
    res, refs = _rollout(env, ref, w, 'table', 5)
    per_env = (1 + np.arange(w.E) % 4).astype(np.uint32)
    assert np.array_equal(env.episodes_left(set=per_env), ref.left) and (ref.len > 0).any()
    ref.left = per_env.copy()
    res, refs = _rollout(env, ref, w, 'table', 20, record=True)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, True, 'per-env budgets')
    assert not ref.left.any()
    env.set_episode_budget(2)                                               # re-arms every env; cells, ages, partials and the log stay
    ref.set_budget(2)
    _check_log(env, ref, 're-armed')
    res, refs = _rollout(env, ref, w, 'table', 9, record=True)
    _check(env, ref, res, refs, bc.totals_of(refs), 4, True, 'second budget')
    assert not ref.left.any() and (ref.count > 4).any()
    env.set_episode_limit(3)                                                # zeroes the ages, leaves the log and the partials alone
    ref.lim.set_limit(3)
    ref.set_budget(2)
    env.set_episode_budget(2)
    res, refs = _rollout(env, ref, w, 'table', 7)
    _check(env, ref, res, refs, bc.totals_of(refs), 3, False, 'another limit')
    assert (ref.count > 6).any()                                            # counted beyond the capacity, not stored
    env.close()


def test_a_device_pointer_handle_with_env_ids_beyond_32_bits():
    w = workload(8, 64)
    for source in SOURCES:
        _run_pass(w, 4, 0.2, 3, 2, source=source, device_arrays=True, env_id_offset=(1 << 32) + 5)
    import torch
    env, ref = _logged(w, 4, 0.2, 10, 10, device_arrays=True)
    res, refs = _rollout(env, ref, w, 'table', 9)
    out = {'records': torch.zeros((w.E, 10, 16), dtype=torch.uint8, device='cuda'), 'count': torch.zeros(w.E, dtype=torch.uint32, device='cuda')}
    got = env.episode_log(out=out)
    assert got['records'] is out['records'] and got['count'] is out['count'] and got['returns'].is_cuda
    assert np.array_equal(raw_bytes(_records(got)), raw_bytes(ref.records)) and np.array_equal(to_np(got['count']), ref.count)
    env.close()


def test_two_shards_concatenate_to_the_whole_batch():
    w = workload(8, 64)
    whole = _run_pass(w, 4, 0.2, 10, 10)
    cut = 27
    parts = []
    for lo, hi in ((0, cut), (cut, w.E)):
        part = ec.Workload.__new__(ec.Workload)
        part.__dict__.update(w.__dict__)
        part.E, part.start, part.goal, part.rows = hi - lo, w.start[lo:hi], w.goal[lo:hi], w.rows[lo:hi]
        part.actions = lambda source, ref, part=part: part.table[part.rows.astype(np.int64), ref.co.state.astype(np.int64)]
        env, ref = _logged(part, 4, 0.2, 10, 10, env_id_offset=lo)
        for n in ec.LAUNCHES:
            res, refs = _rollout(env, ref, part, 'table', n)
        _check_log(env, ref, ('shard', lo))
        got = env.episode_log()
        parts.append((got['records'].copy(), got['count'].copy()))
        env.close()
    assert np.array_equal(raw_bytes(np.concatenate([p[0] for p in parts])), raw_bytes(whole.records))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole.count)


def test_kernel_names_with_the_log_on_and_off(monkeypatch):
    """LOG next to BUDGET whatever the family flag and limit_packed; with the log off again the budget instance, its name and its results"""
    w = workload(8, 64)
    for tune, kw in (({'k': 4, 'limit_packed': 1}, {}), ({}, {'kernel': 'lane_group'}), ({}, {'kernel': 'thread_per_env'})):
        set_tune(monkeypatch, k=tune.get('k'), limit_packed=tune.get('limit_packed'))
        env, ref = _logged(w, 4, 0.2, 3, 3, **kw)
        res, refs = _rollout(env, ref, w, 'table', 6)
        got = env.last_kernel('rollout')
        assert got.startswith('lg_rollout_kernel_table_budget_guarded_log<') and 'BUDGET,LOG>' in got and 'episode log' in got, got
        _check(env, ref, res, refs, bc.totals_of(refs), 4, False, (tune, kw))
        env.set_episode_log(None)
        assert env.episode_log_capacity == 0
        with pytest.raises(ValueError):
            env.episode_log()
        plain, _ = make(w, 4, 0.2, 'Makespan', 'table', **kw)
        plain.set_episode_budget(3)
        env.reset()
        env.set_state(t=0)
        env.set_episode_budget(3)
        a, b = env.rollout(6, record=True), plain.rollout(6, record=True)
        assert 'LOG' not in env.last_kernel('rollout') and env.last_kernel('rollout') == plain.last_kernel('rollout')
        assert env.last_kernel('rollout').startswith('lg_rollout_kernel_table_budget_guarded<')
        assert sorted(a) == sorted(b)
        for key in b:
            assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), key
        env.close()
        plain.close()


def test_refusals():
    w = workload(3, 37)
    env, _ = make(w, 4, 0.2, 'Makespan', 'policy')
    lib, E = env._lib, w.E
    rec, count = np.zeros((E, 2), nat.EPISODE_RECORD_DTYPE), np.zeros(E, np.uint32)
    # without a budget: no log; without a log: nothing to read
    assert lib.mapf_set_episode_log(env._h, 2) == nat.MAPF_EINVAL and b'without an episode budget' in lib.mapf_last_error()
    assert lib.mapf_set_episode_log(env._h, 0) == 0
    assert lib.mapf_episode_log(env._h, rec.ctypes.data, count.ctypes.data, 0) == nat.MAPF_EINVAL and b'no episode log' in lib.mapf_last_error()
    with pytest.raises(ValueError):
        env.episode_log()
    env.set_episode_budget(2)
    assert lib.mapf_set_episode_log(env._h, (1 << 27) // E + 1) == nat.MAPF_EINVAL and b'2^31' in lib.mapf_last_error()
    for bad in (-1, 1 << 32, 2.5, True):
        with pytest.raises(ValueError):
            env.set_episode_log(bad)
    env.set_episode_log(2)
    assert lib.mapf_episode_log(env._h, None, None, 0) == nat.MAPF_EINVAL
    assert lib.mapf_episode_log(env._h, None, None, 1) == 0 and lib.mapf_episode_log(env._h, None, count.ctypes.data, 0) == 0 and not count.any()
    assert lib.mapf_set_episode_budget(env._h, 0) == nat.MAPF_EINVAL and b'mapf_set_episode_log(h, 0) first' in lib.mapf_last_error()
    with pytest.raises(nat.MapfNativeError):
        env.set_episode_budget(None)
    assert env.episode_budget == 2 and (env.episodes_left() == 2).all()
    with pytest.raises(ValueError):
        env.episode_log(out={'records': np.zeros((E, 2, 16), np.uint8)})
    env.set_episode_log(0)
    env.set_episode_budget(None)
    env.close()
    dev, _ = make(w, 4, 0.2, 'Makespan', 'policy', device_arrays=True)
    dev.set_episode_budget(2)
    dev.set_episode_log(2)
    with pytest.raises(nat.MapfNativeError) as err:
        dev.graph_begin()
    assert err.value.code == nat.MAPF_EUNSUPPORTED
    dev.set_episode_log(0)
    dev.set_episode_budget(0)
    dev.set_episode_limit(0)
    dev.graph_begin()
    kept = dev.rollout(2)
    graph = dev.graph_end()
    with pytest.raises(nat.MapfNativeError):
        dev.set_episode_log(0)                                              # not under live graphs, as the budget
    graph.close()
    del kept
    dev.close()


@pytest.mark.parametrize('device_arrays', [False, True])
def test_policies_evaluate_with_the_log_end_to_end(device_arrays):
    w = workload(8, 64)
    env, _ = make(w, None, 0.2, 'Makespan', 'table', device_arrays=device_arrays)
    got = policies.evaluate(env, 3, 4, chunk=5, log=True)                   # ceil(12 / 5) = 3 launches of 5
    assert env.t == 15 and 'BUDGET,LOG' in env.last_kernel('rollout') and (env.episode_limit, env.episode_budget, env.episode_log_capacity) == (4, 3, 3)
    ref = lc.oracle(w, 4, 0.2, 3, 3)
    want = bc.totals_of(ref.run(w, 'table', 15))
    assert not ref.left.any() and (ref.count == 3).all()
    assert sorted(got) == ['collisions', 'episode_outcomes', 'episode_returns', 'episode_steps', 'goal_ends', 'live_steps', 'returns', 'truncations']
    for key in ('returns', 'collisions', 'truncations', 'live_steps'):
        assert np.array_equal(raw_bytes(got[key]), raw_bytes(want[key])), key
    assert np.array_equal(raw_bytes(got['episode_returns']), raw_bytes(ref.records['ret']))
    assert np.array_equal(got['episode_steps'], ref.records['steps']) and np.array_equal(got['episode_outcomes'], ref.records['outcome'])
    assert got['episode_returns'].shape == got['episode_steps'].shape == got['episode_outcomes'].shape == (w.E, 3)
    # per env: the lengths sum to the live steps, the outcome counts are the three totals
    assert np.array_equal(got['episode_steps'].sum(axis=1), got['live_steps'])
    for code, key in ((lc.GOAL, 'goal_ends'), (lc.COLLISION, 'collisions'), (lc.TRUNCATED, 'truncations')):
        assert np.array_equal((got['episode_outcomes'] == code).sum(axis=1), got[key]), key
    stats = policies.episode_statistics(got)
    assert stats['pooled']['n'] == 3 * w.E and np.allclose(stats['per_env']['mean'] * 3, got['returns'], rtol=0, atol=1e-12)
    env.close()
