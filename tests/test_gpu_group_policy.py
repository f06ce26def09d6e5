"""GPU parity of the group policy (include/mapf_hip.h MAPF_POLICY_GROUP; VecMapfEnv.set_policy('group')): fused rollouts whose merged
groups of two to four agents follow sparse books over their joint cells, against the composition of tests/group_policy_cases.py --
group_actions by the definition, then the unchanged COracle / LimitOracle / BudgetOracle / PairsOracle / LogOracle stepped with them
-- bit for bit: cells, flags, the bit patterns of reward and prob, totals, final state, step index, ages, counts, the conflict matrix
and the episode log.  The rewards are episode_limit_cases.INEXACT throughout.  Every bad input here is one the host rejects: nothing
provokes a device fault."""
import numpy as np
import pytest

import episode_limit_cases as ec
import episode_log_cases as lc
import group_policy_cases as gc
import joint_policy_cases as jc
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import policies
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from parity_checks import raw_bytes, to_np

pytestmark = pytest.mark.gpu

TOTALS = ('returns', 'episodes', 'collisions')
RECORDED = ('local', 'reward', 'prob', 'done', 'collision')
N, B, C = 5, 3, 2                               # the episode limit, the episode budget and the log's capacity of the form tests
FORMS = ((N, 0, 0), (N, B, 0), (N, B, C))       # beside the plain form (0, 0, 0)
SLOTS = (None, 'one', 'per_env')


def _env(w, slip=0.2, plan='group', first=0, count=None, **kw):
    part = slice(first, None if count is None else first + count)
    env = VecMapfEnv(w.grid, w.A, None, None, slip, *ec.INEXACT, OptimizationCriteria.Makespan, seed=ec.ORACLE_SEED, start_local=w.start[part],
                     goal_local=w.goal[part], env_id_offset=first, **kw)
    if plan == 'group':
        env.set_policy('group', **w.plan())
        assert env.policy == 'group'
    return env


def _keys(n, b, record):
    totals = TOTALS + (('truncations',) if n else ()) + (('live_steps',) if b else ())
    return totals, ((RECORDED + (('truncated',) if n else ())) if record else ())


def _name(env, L, full, n, b, c, pairs, kind, tag, mv=None):
    got = env.last_kernel('rollout')
    family = ('_budget_guarded_log' if c else '_budget_guarded') if b else ('_limit_guarded' if n else '')
    form = ('BUDGET,LOG' if c else 'BUDGET') if b else ('LIMIT' if n else 'GUARDED')
    assert got.startswith('lg_rollout_kernel_group%s%s<L=%d,%s,' % (family, '_pairs' if pairs else '', L, full)), (tag, got)
    assert ',%s,GROUP,%s%s>' % (kind, form, ',PAIRS' if pairs else '') in got and not any(s in got for s in ('TABLE', 'STREAM', 'POLICY', 'JOINT')), (tag, got)
    assert mv is None or mv in got, (tag, got)


def _check(env, ref, res, refs, want, n, b, record, tag):
    totals, recorded = _keys(n, b, record)
    assert sorted(res) == sorted(totals + recorded), (tag, sorted(res))
    for key in recorded:
        for t, r in enumerate(refs):
            assert np.array_equal(raw_bytes(res[key][t]), raw_bytes(r[key])), (tag, key, t)
    for key in totals:
        assert np.array_equal(raw_bytes(res[key]), raw_bytes(want[key].astype(to_np(res[key]).dtype))), (tag, key)
    local, ages, left = env.get_state()[0], env.episode_steps(), env.episodes_left()
    env.sync()
    assert np.array_equal(to_np(local), ref.co.state) and env.t == ref.co.t, tag
    assert not n or np.array_equal(to_np(ages), ref.age), tag
    assert not b or np.array_equal(to_np(left), ref.left), tag
    if hasattr(ref, 'M'):
        M = env.conflict_pairs()
        env.sync()
        assert np.array_equal(to_np(M), ref.M), (tag, 'conflict matrix', int(to_np(M).sum()), int(ref.M.sum()))
    if isinstance(ref, lc.LogOracle):
        got = env.episode_log()
        env.sync()
        rec = to_np(got['records'])
        rec = np.ascontiguousarray(rec).view(lc.RECORD).reshape(rec.shape[:2]) if rec.dtype == np.uint8 else rec
        assert np.array_equal(to_np(got['count']), ref.count), (tag, 'log counts')
        assert np.array_equal(raw_bytes(rec), raw_bytes(ref.records)), (tag, 'log records')


def _run(env, ref, w, L, full, n=0, b=0, c=0, tag=(), steps=(gc.T, 10, 5), mv=None, source='group'):
    """a recording rollout, a totals-only one and one that accumulates into the second's totals; everything compared after each"""
    pairs = hasattr(ref, 'M')
    refs = ref.run(w, source, steps[0])
    res = env.rollout(steps[0], auto_reset=True, record=True)
    _name(env, L, full, n, b, c, pairs, 'RECORD', tag, mv)
    _check(env, ref, res, refs, jc.totals_of(refs), n, b, True, tag + ('record',))
    refs = ref.run(w, source, steps[1])
    res = env.rollout(steps[1], auto_reset=True)
    _name(env, L, full, n, b, c, pairs, 'TOTALS', tag, mv)
    base = jc.totals_of(refs)
    _check(env, ref, res, refs, base, n, b, False, tag + ('totals',))
    refs = ref.run(w, source, steps[2])
    res = env.rollout(steps[2], auto_reset=True, accumulate_into=res)
    _check(env, ref, res, refs, jc.totals_of(refs, base), n, b, False, tag + ('accumulate',))


def _group(A):
    L = max(1, 1 << ((A + 1) // 2 - 1).bit_length())
    return L, 'FULL' if A == 2 * L else 'RAGGED'


def _same_results(a, b, tag):
    assert sorted(a) == sorted(b), tag
    for key in b:
        assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), (tag, key)


# ------------------------------------------------------------------- random plans, bit for bit
@pytest.mark.parametrize('A,E,kw,L,full', gc.SHAPES)
def test_random_groups_over_the_lane_group_sizes(A, E, kw, L, full):
    w = gc.random_groups(A, E)
    env = _env(w, **kw)
    _run(env, w.oracle(), w, L, full, tag=(A, E), mv='MV_GLOBAL')
    slots, chain = env.policy_group_stats()
    assert slots & (slots - 1) == 0 and slots >= 2 * w.entry_cells.shape[0] and chain >= 1
    env.close()


def test_a_table_of_four_thousand_entries_with_probe_chains():
    A, E = gc.BIG_SHAPE
    w = gc.random_groups(A, E, big=True)
    env = _env(w)
    slots, chain = env.policy_group_stats()
    assert w.entry_cells.shape[0] >= gc.BIG_ENTRIES and slots >= 2 * w.entry_cells.shape[0] and chain >= 2
    _run(env, w.oracle(), w, *_group(A), tag=('big',))
    env.close()


@pytest.mark.parametrize('kw', gc.BROADCAST_CASES)
def test_broadcast_arrays_against_the_same_plan_per_env(kw):
    """[A] arrays shared by all envs: against the reference, and against the same plan given as [E, A]"""
    A, E = gc.BROADCAST_SHAPE
    w = gc.random_groups(A, E, **kw)
    assert w.plan()['rows'].shape == (A,) and w.plan()['members'].shape == (A, 4) and w.per_env_plan()['members'].shape == (E, A, 4)
    env = _env(w)
    _run(env, w.oracle(), w, *_group(A), tag=('broadcast', kw['round']))
    per_env = _env(w, plan=None)
    per_env.set_policy('group', **w.per_env_plan())
    for h in (env, per_env):
        h.reset()
        h.set_state(t=0)
    _same_results(env.rollout(gc.T, auto_reset=True, record=True), per_env.rollout(gc.T, auto_reset=True, record=True), 'per env')
    assert env.last_kernel('rollout') == per_env.last_kernel('rollout')
    env.close()
    per_env.close()


# ------------------------------------------------------------------- routing
def test_a_group_launch_takes_the_lane_group_instance_whatever_the_family():
    """(8, 8192): under the group policy the lane-group group instance, also on a thread_per_env handle; at this size the move table
    is staged into LDS"""
    w = gc.random_groups(8, 8192, empty_books=True)
    ref = w.oracle()
    refs = ref.run(w, 'group', 6)
    want = jc.totals_of(refs)
    for kernel in ('auto', 'thread_per_env', 'lane_group'):
        env = _env(w, kernel=kernel)
        res = env.rollout(6, auto_reset=True)
        _name(env, 4, 'FULL', 0, 0, 0, False, 'TOTALS', kernel, 'MV_LDS')
        for key in TOTALS:
            assert np.array_equal(raw_bytes(res[key]), raw_bytes(want[key].astype(res[key].dtype))), (kernel, key)
        assert np.array_equal(env.get_state()[0], ref.co.state)
        env.close()


# ------------------------------------------------------------------- every form
@pytest.mark.parametrize('slots', SLOTS)
@pytest.mark.parametrize('A,E', gc.FORM_SHAPES)
def test_every_form_under_the_limit_the_budget_the_matrix_and_the_log(A, E, slots):
    """the limit, limit + budget, limit + budget + log, and with a conflict matrix (one slot, a slot per env) the plain form as well
    (the plain form without the matrix: the tests above); each recording and totals-only"""
    w = gc.random_groups(A, E, seed=1)
    pairs = None if slots is None else ((1, None) if slots == 'one' else (E, np.arange(E)))
    for n, b, c in (FORMS if slots is None else ((0, 0, 0),) + FORMS):
        env = _env(w)
        if n:
            env.set_episode_limit(n)
        if b:
            env.set_episode_budget(b)
        if pairs:
            env.set_conflict_pairs(*pairs)
        if c:
            env.set_episode_log(c)
        ref = w.oracle(n, 0.2, b, pairs, C=c)
        _run(env, ref, w, *_group(A), n=n, b=b, c=c, tag=(A, E, n, b, c, slots))
        if pairs:
            assert ref.M.any()
        env.close()


# ------------------------------------------------------------------- split launches and shards
def test_a_split_launch_equals_one_launch():
    w = gc.random_groups(7, 300)
    whole, split = _env(w), _env(w)
    want = whole.rollout(gc.T, auto_reset=True, record=True)
    parts, totals = [], None
    for steps in (1, 2, 7, 14):
        res = split.rollout(steps, auto_reset=True, record=True, accumulate_into=totals)
        parts.append({k: np.array(to_np(res[k])) for k in RECORDED})
        totals = {k: res[k] for k in TOTALS}
    for key in RECORDED:
        assert np.array_equal(raw_bytes(np.concatenate([p[key] for p in parts])), raw_bytes(want[key])), key
    for key in TOTALS:
        assert np.array_equal(raw_bytes(totals[key]), raw_bytes(want[key])), key
    assert np.array_equal(whole.get_state()[0], split.get_state()[0]) and whole.t == split.t == gc.T
    whole.close()
    split.close()


def test_two_shards_by_env_id_offset_equal_the_whole_batch():
    A, E = 7, 300
    w = gc.random_groups(A, E)
    whole = _env(w)
    want = whole.rollout(gc.T, auto_reset=True, record=True)
    cut, got = 129, []
    for first, count in ((0, cut), (cut, E - cut)):
        shard = _env(w, plan=None, first=first, count=count)
        plan = w.plan()
        shard.set_policy('group', **dict(plan, rows=plan['rows'][first:first + count], members=plan['members'][first:first + count],
                                         book=plan['book'][first:first + count]))
        got.append(shard.rollout(gc.T, auto_reset=True, record=True))
        shard.close()
    for key in want:
        axis = 1 if key in RECORDED else 0
        assert np.array_equal(raw_bytes(np.concatenate([to_np(g[key]) for g in got], axis=axis)), raw_bytes(want[key])), key
    whole.close()


# ------------------------------------------------------------------- against the other table policies
@pytest.mark.parametrize('books', ('none', 'no match'))
def test_empty_books_equal_the_table_policy(books):
    """n_books = 0, and books in which no entry ever matches (every entry at another arity): the SAME launch under set_policy('table')"""
    A, E = 8, 64
    w = gc.random_groups(A, E, empty_books=True)
    plan = w.plan()
    assert gc.groups_of(plan['members'], plan['book'], E, A)
    if books == 'none':
        plan = dict(plan, entry_cells=None, entry_actions=None, book_begin=None)                 # (book is not read then)
    else:
        rs = np.random.RandomState(4)
        cells = np.full((500, 4), gc.PAD, np.uint16)
        cells[:, 0] = rs.permutation(w.V)[:500] if w.V >= 500 else rs.randint(0, w.V, 500)      # arity 1: no group has it
        cells = np.unique(cells, axis=0)
        begin = np.zeros(w.n_books + 1, np.uint32)
        begin[1:] = cells.shape[0]                                                               # all in book 0, which env 0 names
        plan = dict(plan, entry_cells=cells, entry_actions=np.where(cells == gc.PAD, 0, 3).astype(np.uint8), book_begin=begin)
    env, table = _env(w, plan=None), _env(w, plan=None)
    env.set_policy('group', **plan)
    assert (env.policy_group_stats() == (1, 0)) == (books == 'none')
    table.set_policy('table', table=w.table, rows=w.rows)
    for n, b in ((0, 0), (N, B)):
        for h in (env, table):
            h.set_episode_limit(n)
            h.set_episode_budget(b)
            h.reset()
            h.set_state(t=0)
        _same_results(env.rollout(gc.T, auto_reset=True, record=True), table.rollout(gc.T, auto_reset=True, record=True), (books, n, b))
        assert 'GROUP' in env.last_kernel('rollout') and 'TABLE' in table.last_kernel('rollout')
        assert np.array_equal(env.get_state()[0], table.get_state()[0]) and env.t == table.t
    env.close()
    table.close()


def test_pair_groups_with_complete_books_equal_the_joint_policy():
    w = gc.complete_pairs()
    assert 50 <= w.V <= 64
    env, joint = _env(w), _env(w, plan=None)
    joint.set_policy('joint', **w.joint)
    for h in (env, joint):
        h.set_conflict_pairs()
    _same_results(env.rollout(gc.T, auto_reset=True, record=True), joint.rollout(gc.T, auto_reset=True, record=True), 'joint')
    assert 'GROUP' in env.last_kernel('rollout') and 'JOINT' in joint.last_kernel('rollout')
    assert np.array_equal(env.get_state()[0], joint.get_state()[0]) and np.array_equal(env.conflict_pairs(), joint.conflict_pairs())
    ref = w.oracle(pairs=(1, None))
    refs = ref.run(w, 'group', gc.T)
    assert np.array_equal(env.get_state()[0], ref.co.state) and np.array_equal(env.conflict_pairs(), ref.M) and len(refs) == gc.T
    env.close()
    joint.close()


def test_a_group_of_four_on_a_large_map():
    """Berlin_1_256: the move table stays in global memory, cells above 32767 in keys and in rows"""
    w = gc.large_map()
    env = _env(w)
    _run(env, w.oracle(), w, 2, 'FULL', tag=('berlin',), mv='MV_GLOBAL')
    assert w.start.min() > 32767
    env.close()


# ------------------------------------------------------------------- the planner's loop, end to end
def _same(got, want, M, tag):
    for key in ('returns', 'collisions', 'truncations', 'live_steps', 'goal_ends'):
        assert np.array_equal(raw_bytes(got[key]), raw_bytes(want[key].astype(got[key].dtype))), (tag, key)
    assert np.array_equal(got['pair_conflicts'], M), tag


@pytest.mark.parametrize('A', gc.THREE_AGENTS)
def test_evaluate_finds_the_group_and_the_group_plan_ends_its_conflicts(A):
    w = gc.three_way(A)
    n, E = gc.THREE_EPISODES, w.E
    evaluate = lambda env: policies.evaluate(env, n, gc.THREE_MAX_STEPS, chunk=gc.THREE_CHUNK)
    # the solo plan: the group (0, 1, 2) and nothing else
    env = _env(w, slip=0.0, plan=None)
    env.set_policy('table', table=w.table, rows=w.rows)
    env.set_conflict_pairs()
    solo = evaluate(env)
    groups, too_large = policies.conflicting_groups(solo['pair_conflicts'])
    assert groups == [(0, 1, 2)] and not too_large and (solo['collisions'] == n).all()
    _same(solo, *w.evaluated('table'), ('solo', A))
    # merge it: the group replanned on the junction, everybody's rows as they were
    table, rows_of = policies.shortest_path_table(w.grid, w.goal[0])
    rows = {k: table[rows_of[int(w.goal[0, k])]] for k in range(A)}
    group, = groups
    plan = policies.join_group_plan(w.V, A, rows, {group: policies.group_shortest_path_entries(w.grid, [w.goal[0, k] for k in group], w.region)})
    assert all(np.array_equal(plan[k], w.group[k]) for k in plan)
    env.set_policy('group', **plan)
    merged = evaluate(env)
    assert 'group_budget_guarded_pairs<' in env.last_kernel('rollout') and 'GROUP,BUDGET,PAIRS>' in env.last_kernel('rollout')
    assert not merged['collisions'].any() and (merged['goal_ends'] == n).all() and not merged['pair_conflicts'].any()
    want, M = w.evaluated('group')
    _same(merged, want, M, ('merged', A))
    env.close()
    # with slip: compared with the oracle only (a slot per env)
    env = _env(w, slip=0.2)
    env.set_conflict_pairs(E, np.arange(E))
    slipped = evaluate(env)
    _same(slipped, *w.evaluated('group', slip=0.2, slots=np.arange(E)), ('slip', A))
    env.close()


# ------------------------------------------------------------------- mode changes and refusals
def test_mode_changes_group_table_group_joint_random():
    w = gc.random_groups(8, 64)
    wj = jc.RandomJoint(8, 64)                                               # (the same map, starts and goals)
    assert np.array_equal(w.start, wj.start) and np.array_equal(w.goal, wj.goal)
    env, fresh = _env(w), _env(w, plan=None)

    def restart():
        for h in (env, fresh):
            h.reset()
            h.set_state(t=0)

    def group_again(tag):
        restart()
        ref = w.oracle()
        refs = ref.run(w, 'group', 6)
        res = env.rollout(6, auto_reset=True, record=True)
        _name(env, 4, 'FULL', 0, 0, 0, False, 'RECORD', tag)
        _check(env, ref, res, refs, jc.totals_of(refs), 0, 0, True, tag)

    group_again('group')
    table, rows = policies.shortest_path_policy(env)
    env.set_policy('table', table=table, rows=rows)
    fresh.set_policy('table', table=table, rows=rows)
    restart()
    _same_results(env.rollout(6, auto_reset=True, record=True), fresh.rollout(6, auto_reset=True, record=True), 'table')
    assert env.last_kernel('rollout') == fresh.last_kernel('rollout') and 'TABLE' in env.last_kernel('rollout')
    env.set_policy('group', **w.plan())
    group_again('group after table')
    env.set_policy('joint', **wj.plan())
    fresh.set_policy('joint', **wj.plan())
    restart()
    _same_results(env.rollout(6, auto_reset=True, record=True), fresh.rollout(6, auto_reset=True, record=True), 'joint')
    assert env.last_kernel('rollout') == fresh.last_kernel('rollout') and 'JOINT' in env.last_kernel('rollout')
    with pytest.raises(nat.MapfNativeError):
        env.policy_group_stats()                                            # (not in the mode any more)
    env.set_policy('group', **w.plan())
    env.set_policy('random')
    fresh.set_policy('random')
    restart()
    _same_results(env.rollout(6, auto_reset=True, record=True), fresh.rollout(6, auto_reset=True, record=True), 'random')
    assert env.last_kernel('rollout') == fresh.last_kernel('rollout') and 'POLICY' in env.last_kernel('rollout') and 'GROUP' not in env.last_kernel('rollout')
    # streamed actions ignore the plan, as they ignore the table
    env.set_policy('group', **w.plan())
    acts = np.random.RandomState(1).randint(0, 5, size=(2, 64, 8)).astype(np.uint8)
    restart()
    _same_results(env.rollout(2, actions=acts, auto_reset=True, record=True), fresh.rollout(2, actions=acts, auto_reset=True, record=True), 'streamed')
    assert 'STREAM' in env.last_kernel('rollout') and 'GROUP' not in env.last_kernel('rollout')
    group_again('group after a streamed launch')
    env.close()
    fresh.close()


def test_refusals_leave_the_previous_plan_running():
    w = gc.random_groups(8, 37)
    env = _env(w)
    lib, A = env._lib, w.A
    args = VecMapfEnv._group_arguments(w.V, w.E, A, **w.plan())

    def refused(says, code=nat.MAPF_EINVAL, flags=0, **change):
        table8, rows16, members16, book32, entries, begin32 = (change.get(k, a) for k, a in zip(('table', 'rows', 'members', 'book', 'entries', 'begin'), args))
        rc = lib.mapf_set_policy_group(env._h, table8.ctypes.data, table8.shape[0], rows16.ctypes.data, members16.ctypes.data, book32.ctypes.data,
                                       entries.ctypes.data, entries.size, begin32.ctypes.data, begin32.size - 1, flags)
        assert rc == code and all(s in lib.mapf_last_error() for s in says), lib.mapf_last_error()

    e = 9
    group = next(g for env_of, g, _ in w._groups if env_of == e)
    i = group[0]
    bad = args[2].copy()
    bad[e, i, 1] = A
    refused((b'members[%d] = %d' % ((e * A + i) * 4 + 1, A), b'not below n_agents'), members=bad)
    bad = args[3].copy()
    bad[e, i] = args[5].size - 1
    refused((b'book[', b'n_books'), book=bad)
    bad = args[4].copy()
    bad['action'][3, 0] = 5
    refused((b'entries[3].action[0] = 5',), entries=bad)
    refused((b'unknown bits',), flags=4)
    assert lib.mapf_set_policy(env._h, nat.MAPF_POLICY_GROUP, None) == nat.MAPF_EINVAL and b'mapf_set_policy_group' in lib.mapf_last_error()
    with pytest.raises(ValueError):
        env.set_policy('group', **dict(w.plan(), book=np.full_like(w.plan()['book'], args[5].size - 1)))
    assert env.policy == 'group'
    # the previous plan is in force: the oracle's results under the workload's plan
    ref = w.oracle()
    refs = ref.run(w, 'group', 8)
    res = env.rollout(8, auto_reset=True, record=True)
    _name(env, 4, 'FULL', 0, 0, 0, False, 'RECORD', 'kept')
    _check(env, ref, res, refs, jc.totals_of(refs), 0, 0, True, 'kept')
    # step() in the mode is the step it was
    plain = _env(w, plan=None)
    for h in (env, plain):
        h.set_state(local=ref.co.state, t=ref.co.t)
    acts = np.random.RandomState(2).randint(0, 5, size=(w.E, A)).astype(np.uint8)
    a, b = env.step(acts, auto_reset=True), plain.step(acts, auto_reset=True)
    assert env.last_kernel('step') == plain.last_kernel('step') and 'GROUP' not in env.last_kernel('step')
    for x, y in zip(a, b):
        if isinstance(y, dict):
            assert all(np.array_equal(raw_bytes(x[k]), raw_bytes(y[k])) for k in y)
        else:
            assert np.array_equal(raw_bytes(x), raw_bytes(y))
    env.close()
    plain.close()


def test_graph_begin_is_refused_in_the_mode():
    w = gc.random_groups(8, 64)
    dev = _env(w, device_arrays=True)
    with pytest.raises(nat.MapfNativeError) as err:
        dev.graph_begin()
    assert err.value.code == nat.MAPF_EUNSUPPORTED
    dev.set_policy('random')
    dev.graph_begin()
    with pytest.raises(nat.MapfNativeError) as err:
        dev.set_policy('group', **w.plan())                                 # not while recording
    assert err.value.code == nat.MAPF_EINVAL
    kept = dev.rollout(2)
    graph = dev.graph_end()
    with pytest.raises(nat.MapfNativeError):
        dev.set_policy('group', **w.plan())                                 # not under live graphs
    assert dev.policy == 'random'
    graph.close()
    del kept
    dev.set_policy('group', **w.plan())
    dev.close()
