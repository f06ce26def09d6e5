"""GPU parity of the joint table policy (include/mapf_hip.h MAPF_POLICY_JOINT; VecMapfEnv.set_policy('joint')): fused rollouts whose
merged agent pairs follow a table over both cells, against the composition of tests/joint_policy_cases.py -- joint_actions by the
definition, then the unchanged COracle / LimitOracle / BudgetOracle / PairsOracle stepped with them -- bit for bit: cells, flags, the
bit patterns of reward and prob, totals, final state, step index, ages, counts and the conflict matrix.  The rewards are
episode_limit_cases.INEXACT throughout.  Every bad input here is one the host rejects: nothing provokes a device fault."""
import numpy as np
import pytest

import episode_limit_cases as ec
import joint_policy_cases as jc
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import policies
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from parity_checks import raw_bytes, to_np

pytestmark = pytest.mark.gpu

TOTALS = ('returns', 'episodes', 'collisions')
RECORDED = ('local', 'reward', 'prob', 'done', 'collision')
FORMS = ((7, 0), (7, 3))                        # (episode limit, episode budget) beside the plain form (0, 0)
SLOTS = (None, 'one', 'per_env')


def _env(w, slip=0.2, joint=True, **kw):
    env = VecMapfEnv(w.grid, w.A, None, None, slip, *ec.INEXACT, OptimizationCriteria.Makespan, seed=ec.ORACLE_SEED, start_local=w.start, goal_local=w.goal, **kw)
    if joint:
        env.set_policy('joint', **w.plan())
        assert env.policy == 'joint'
    return env


def _keys(N, B, record):
    totals = TOTALS + (('truncations',) if N else ()) + (('live_steps',) if B else ())
    return totals, ((RECORDED + (('truncated',) if N else ())) if record else ())


def _name(env, L, full, N, B, pairs, kind, tag, mv=None):
    got = env.last_kernel('rollout')
    family = '_budget_guarded' if B else ('_limit_guarded' if N else '')
    form = 'BUDGET' if B else ('LIMIT' if N else 'GUARDED')
    assert got.startswith('lg_rollout_kernel_joint%s%s<L=%d,%s,' % (family, '_pairs' if pairs else '', L, full)), (tag, got)
    assert ',%s,JOINT,%s%s>' % (kind, form, ',PAIRS' if pairs else '') in got and not any(s in got for s in ('TABLE', 'STREAM', 'POLICY')), (tag, got)
    assert mv is None or mv in got, (tag, got)


def _check(env, ref, res, refs, want, N, B, record, tag):
    totals, recorded = _keys(N, B, record)
    assert sorted(res) == sorted(totals + recorded), (tag, sorted(res))
    for key in recorded:
        for t, r in enumerate(refs):
            assert np.array_equal(raw_bytes(res[key][t]), raw_bytes(r[key])), (tag, key, t)
    for key in totals:
        assert np.array_equal(raw_bytes(res[key]), raw_bytes(want[key].astype(to_np(res[key]).dtype))), (tag, key)
    local, ages, left = env.get_state()[0], env.episode_steps(), env.episodes_left()
    env.sync()
    assert np.array_equal(to_np(local), ref.co.state) and env.t == ref.co.t, tag
    assert not N or np.array_equal(to_np(ages), ref.age), tag
    assert not B or np.array_equal(to_np(left), ref.left), tag
    if hasattr(ref, 'M'):
        M = env.conflict_pairs()
        env.sync()
        assert np.array_equal(to_np(M), ref.M), (tag, 'conflict matrix', int(to_np(M).sum()), int(ref.M.sum()))


def _run(env, ref, w, L, full, N=0, B=0, tag=(), steps=(20, 10, 5), mv=None):
    """a recording rollout, a totals-only one and one that accumulates into the second's totals; everything compared after each"""
    pairs = hasattr(ref, 'M')
    refs = ref.run(w, 'joint', steps[0])
    res = env.rollout(steps[0], auto_reset=True, record=True)
    _name(env, L, full, N, B, pairs, 'RECORD', tag, mv)
    _check(env, ref, res, refs, jc.totals_of(refs), N, B, True, tag + ('record',))
    refs = ref.run(w, 'joint', steps[1])
    res = env.rollout(steps[1], auto_reset=True)
    _name(env, L, full, N, B, pairs, 'TOTALS', tag, mv)
    base = jc.totals_of(refs)
    _check(env, ref, res, refs, base, N, B, False, tag + ('totals',))
    refs = ref.run(w, 'joint', steps[2])
    res = env.rollout(steps[2], auto_reset=True, accumulate_into=res)
    _check(env, ref, res, refs, jc.totals_of(refs, base), N, B, False, tag + ('accumulate',))


def _group(A):
    L = max(1, 1 << ((A + 1) // 2 - 1).bit_length())
    return L, 'FULL' if A == 2 * L else 'RAGGED'


# ------------------------------------------------------------------- random tables, bit for bit
@pytest.mark.parametrize('A,E,kw,L,full', jc.SHAPES)
def test_random_joint_tables_over_the_group_sizes(A, E, kw, L, full):
    w = jc.RandomJoint(A, E)
    env = _env(w, **kw)
    _run(env, w.oracle(), w, L, full, tag=(A, E), mv='MV_GLOBAL')
    env.close()


def test_broadcast_offsets_and_partners():
    """[A] arrays shared by all envs; one matching cannot hold every geometry of five agents, so two plans"""
    A, E = jc.BROADCAST_SHAPE
    for round in range(2):
        w = jc.RandomJoint(A, E, broadcast=True, round=round)
        assert w.offsets.shape == w.partners.shape == (A,)
        env = _env(w)
        _run(env, w.oracle(), w, *_group(A), tag=('broadcast', round))
        env.close()


# ------------------------------------------------------------------- routing
def test_a_joint_launch_takes_the_lane_group_instance_whatever_the_family():
    """(8, 8192): under the table policy the launch is the packed table kernel it was; under the joint policy the lane-group joint
    instance, also on a thread_per_env handle; at this size the move table is staged into LDS"""
    w = jc.RandomJoint(8, 8192)
    ref = w.oracle()
    refs = ref.run(w, 'joint', 6)
    want = jc.totals_of(refs)
    for kernel in ('auto', 'thread_per_env', 'lane_group'):
        env = _env(w, joint=False, kernel=kernel)
        if kernel == 'auto':
            table, rows = policies.shortest_path_policy(env)
            env.set_policy('table', table=table, rows=rows)
            env.rollout(2, auto_reset=True)
            assert env.last_kernel('rollout').startswith('lq_rollout_kernel_table<'), env.last_kernel('rollout')
            env.reset()
            env.set_state(t=0)
        env.set_policy('joint', **w.plan())
        res = env.rollout(6, auto_reset=True)
        _name(env, 4, 'FULL', 0, 0, False, 'TOTALS', kernel, 'MV_LDS')
        for key in TOTALS:
            assert np.array_equal(raw_bytes(res[key]), raw_bytes(want[key].astype(res[key].dtype))), (kernel, key)
        assert np.array_equal(env.get_state()[0], ref.co.state)
        env.close()


# ------------------------------------------------------------------- every form
@pytest.mark.parametrize('slots', SLOTS)
@pytest.mark.parametrize('A,E', jc.FORM_SHAPES)
def test_every_form_under_the_limit_the_budget_and_the_matrix(A, E, slots):
    """the limit, limit + budget, and with a conflict matrix (one slot, a slot per env) the plain form as well (the plain form
    without the matrix: the tests above)"""
    w = jc.RandomJoint(A, E, seed=1)
    pairs = None if slots is None else ((1, None) if slots == 'one' else (E, np.arange(E)))
    for N, B in (FORMS if slots is None else ((0, 0),) + FORMS):
        env = _env(w)
        if N:
            env.set_episode_limit(N)
        if B:
            env.set_episode_budget(B)
        if pairs:
            env.set_conflict_pairs(*pairs)
        ref = w.oracle(N, 0.2, B, pairs)
        _run(env, ref, w, *_group(A), N=N, B=B, tag=(A, E, N, B, slots))
        if pairs:
            assert ref.M.any()
        env.close()


# ------------------------------------------------------------------- 64-bit counters
def test_step_indices_and_env_ids_beyond_32_bits():
    """the step index crosses 2^32 inside the launch, and the env ids' high word changes inside the batch"""
    w = jc.RandomJoint(8, 64)
    off, t0 = (1 << 32) - 32, (1 << 32) - 8
    env = _env(w, env_id_offset=off)
    env.set_state(t=t0)
    ref = w.oracle(offset=off)
    ref.co.t = t0
    refs = ref.run(w, 'joint', 20)
    res = env.rollout(20, auto_reset=True, record=True)
    _check(env, ref, res, refs, jc.totals_of(refs), 0, 0, True, 'wide')
    assert env.t == t0 + 20 > 1 << 32
    env.close()


# ------------------------------------------------------------------- the planner's loop, end to end
def _same(got, want, M, tag):
    for key in ('returns', 'collisions', 'truncations', 'live_steps', 'goal_ends'):
        assert np.array_equal(raw_bytes(got[key]), raw_bytes(want[key].astype(got[key].dtype))), (tag, key)
    assert np.array_equal(got['pair_conflicts'], M), tag


@pytest.mark.parametrize('W', jc.MERGE_WIDTHS)
@pytest.mark.parametrize('A', jc.MERGE_AGENTS)
def test_evaluate_finds_the_pair_and_the_merged_plan_ends_its_conflicts(A, W):
    w = jc.merge(W, A)
    n, E = jc.MERGE_EPISODES, w.E
    evaluate = lambda env: policies.evaluate(env, n, jc.MERGE_MAX_STEPS, chunk=jc.MERGE_CHUNK)
    # the solo plan: the pair (0, 1) and nothing else
    env = _env(w, slip=0.0, joint=False)
    env.set_policy('table', table=w.table, rows=w.rows)
    env.set_conflict_pairs()
    solo = evaluate(env)
    assert 'table_budget_guarded_pairs<' in env.last_kernel('rollout')
    rows = policies.conflicting_pairs(solo['pair_conflicts'])
    assert [r[:2] for r in rows] == [(0, 1)] and rows[0][2] + rows[0][3] == n * E and (solo['collisions'] == n).all()
    _same(solo, *w.evaluated('table'), ('solo', A, W))
    # merge it: the pair replanned jointly, the bystanders as they were
    (i, j, _, _), = rows
    table, rows_of = policies.shortest_path_table(w.grid, w.goal[0])
    solo_rows = {k: table[rows_of[int(w.goal[0, k])]] for k in range(A) if k not in (i, j)}
    plan = policies.join_plan(w.V, A, solo_rows, {(i, j): policies.pair_shortest_path_rows(w.grid, w.goal[0, i], w.goal[0, j])})
    assert all(np.array_equal(a, b) for a, b in zip(plan, w.joint))
    env.set_policy('joint', table=plan[0], offsets=plan[1], partners=plan[2])
    merged = evaluate(env)
    assert 'joint_budget_guarded_pairs<' in env.last_kernel('rollout') and 'JOINT,BUDGET,PAIRS>' in env.last_kernel('rollout')
    assert not merged['collisions'].any() and (merged['goal_ends'] == n).all() and not merged['pair_conflicts'].any()
    want, M = w.evaluated('joint')
    _same(merged, want, M, ('merged', A, W))
    env.close()
    # with slip: compared with the oracle only (a slot per env)
    env = _env(w, slip=0.2, joint=False)
    env.set_policy('joint', **w.plan())
    env.set_conflict_pairs(E, np.arange(E))
    slipped = evaluate(env)
    _same(slipped, *w.evaluated('joint', slip=0.2, slots=np.arange(E)), ('slip', A, W))
    env.close()


# ------------------------------------------------------------------- mode changes and refusals
def test_mode_changes():
    w = jc.RandomJoint(8, 64)
    env, fresh = _env(w), _env(w, joint=False)
    env.rollout(3, auto_reset=True)
    # 'random' after 'joint': the policy-stream kernel again, with a fresh env's results
    env.set_policy('random')
    env.reset()
    env.set_state(t=0)
    a, b = env.rollout(6, auto_reset=True, record=True), fresh.rollout(6, auto_reset=True, record=True)
    assert env.last_kernel('rollout') == fresh.last_kernel('rollout') and 'POLICY' in env.last_kernel('rollout') and 'JOINT' not in env.last_kernel('rollout')
    for key in b:
        assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), key
    # 'table' after 'joint', and back
    table, rows = policies.shortest_path_policy(env)
    for h in (env, fresh):
        h.reset()
        h.set_state(t=0)
    env.set_policy('joint', **w.plan())
    env.set_policy('table', table=table, rows=rows)
    fresh.set_policy('table', table=table, rows=rows)
    a, b = env.rollout(6, auto_reset=True, record=True), fresh.rollout(6, auto_reset=True, record=True)
    assert env.last_kernel('rollout') == fresh.last_kernel('rollout') and 'TABLE' in env.last_kernel('rollout')
    for key in b:
        assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), key
    env.set_policy('joint', **w.plan())
    env.reset()
    env.set_state(t=0)
    ref = w.oracle()
    refs = ref.run(w, 'joint', 6)
    res = env.rollout(6, auto_reset=True, record=True)
    _name(env, 4, 'FULL', 0, 0, False, 'RECORD', 'back')
    _check(env, ref, res, refs, jc.totals_of(refs), 0, 0, True, 'back')
    # streamed actions ignore the policy, as they ignore the table
    acts = np.zeros((2, 64, 8), np.uint8)
    env.rollout(2, actions=acts, auto_reset=True)
    assert 'STREAM' in env.last_kernel('rollout') and 'JOINT' not in env.last_kernel('rollout')
    env.close()
    fresh.close()


def test_refusals_leave_the_previous_policy_in_force():
    w = jc.RandomJoint(8, 37)
    env = _env(w)
    lib, A, V = env._lib, w.A, w.V
    table, offsets, partners = w.table.copy(), w.offsets.copy(), w.partners.copy()

    def refused(table, offsets, partners, says, size=None, flags=0):
        rc = lib.mapf_set_policy_joint(env._h, table.ctypes.data, table.size if size is None else size, offsets.ctypes.data, partners.ctypes.data, flags)
        assert rc == nat.MAPF_EINVAL and all(s in lib.mapf_last_error() for s in says), lib.mapf_last_error()

    e = 9                                                                   # an env whose agents 3 and 4 are tampered with
    solo = partners.copy()
    solo[e] = np.arange(A)
    one_way = solo.copy()
    one_way[e, 3] = 4                                                       # ... 4 does not name 3 back
    refused(table, offsets, one_way, (b'partner[%d]' % (e * A + 3), b'not mutual'))
    bad = solo.copy()
    bad[e, 3] = A
    refused(table, offsets, bad, (b'partner[%d] = %d' % (e * A + 3, A), b'not below n_agents'))
    bad = offsets.copy()
    bad[e, 3] = table.size - (V if partners[e, 3] == 3 else V * V) + 1
    refused(table, bad, partners, (b'offset[%d]' % (e * A + 3), b'ends past table_bytes'))
    five = table.copy()
    five[12345] = 5
    refused(five, offsets, partners, (b'table[12345] = 5',))
    refused(table, offsets, partners, (b'unknown bits',), flags=4)
    assert lib.mapf_set_policy(env._h, nat.MAPF_POLICY_JOINT, None) == nat.MAPF_EINVAL and b'mapf_set_policy_joint' in lib.mapf_last_error()
    for kw in (dict(partners=one_way), dict(table=five)):
        with pytest.raises(ValueError):
            env.set_policy('joint', **dict(w.plan(), **kw))
    assert env.policy == 'joint'
    # the previous policy is in force: the oracle's results under the workload's plan
    ref = w.oracle()
    refs = ref.run(w, 'joint', 8)
    res = env.rollout(8, auto_reset=True, record=True)
    _name(env, 4, 'FULL', 0, 0, False, 'RECORD', 'kept')
    _check(env, ref, res, refs, jc.totals_of(refs), 0, 0, True, 'kept')
    # step() in joint mode is the step it was
    plain = _env(w, joint=False)
    for h in (env, plain):
        h.set_state(local=ref.co.state, t=ref.co.t)
    acts = np.random.RandomState(2).randint(0, 5, size=(w.E, A)).astype(np.uint8)
    a, b = env.step(acts, auto_reset=True), plain.step(acts, auto_reset=True)
    assert env.last_kernel('step') == plain.last_kernel('step') and 'JOINT' not in env.last_kernel('step')
    for x, y in zip(a, b):
        if isinstance(y, dict):
            assert all(np.array_equal(raw_bytes(x[k]), raw_bytes(y[k])) for k in y)
        else:
            assert np.array_equal(raw_bytes(x), raw_bytes(y))
    env.close()
    plain.close()


def test_graph_begin_is_refused_in_joint_mode():
    w = jc.RandomJoint(8, 64)
    dev = _env(w, device_arrays=True)
    with pytest.raises(nat.MapfNativeError) as err:
        dev.graph_begin()
    assert err.value.code == nat.MAPF_EUNSUPPORTED
    dev.set_policy('random')
    dev.graph_begin()
    with pytest.raises(nat.MapfNativeError) as err:
        dev.set_policy('joint', **w.plan())                                 # not while recording
    assert err.value.code == nat.MAPF_EINVAL
    kept = dev.rollout(2)
    graph = dev.graph_end()
    with pytest.raises(nat.MapfNativeError):
        dev.set_policy('joint', **w.plan())                                 # not under live graphs
    assert dev.policy == 'random'
    graph.close()
    del kept
    dev.set_policy('joint', **w.plan())
    dev.close()
