"""What the parity tests share when they compare the library's outputs with a reference, no test in it: bit views of arrays, the
reward constants, the names of a rollout's outputs, and the handle maker and checks of the episode-limit family of GPU modules
(tests/test_gpu_episode_limit.py, tests/test_gpu_episode_budget.py, tests/test_gpu_limit_packed.py).  Importing it needs no GPU."""
import numpy as np

import episode_limit_cases as ec
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv

# reward constants (clash, goal, living): EXACT -- every product n * living and every sum of rewards is exact in float64, in
# any order; INEXACT -- they round: fl(fl(n * living) + goal) differs from the correctly rounded n * living + goal at
# n = 3, 5, 6, 7, 9, 10, 12, 15, 20, 23..26, 28, 30, 31 (the same with clash), n-fold addition of living differs from n * living
# from n = 6 on, ten left-to-right additions of -0.1 give -0.9999999999999999: a fused multiply-add, a repeated add, a
# reordered or re-associated sum each change bits (tests/golden/inexact_* were recorded from the reference with such constants)
EXACT, INEXACT = (-1000.0, 100.0, -1.0), (-0.3, 0.7, -0.1)
CRIT = {'Makespan': OptimizationCriteria.Makespan, 'SoC': OptimizationCriteria.SoC}
SOURCE_TAG = {'stream': 'STREAM', 'policy': 'POLICY', 'greedy': 'POLICY', 'table': 'TABLE'}
RECORDED = ('local', 'reward', 'prob', 'done', 'collision', 'truncated')
TOTALS = ('returns', 'episodes', 'collisions', 'truncations')


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# not bits(): the bytes of an array of ANY dtype, host or device -- bits() would convert integers and flags to float64 first
def raw_bytes(x):
    return np.ascontiguousarray(to_np(x)).view(np.uint8)


def to_np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


def make(w, N, slip, criteria='Makespan', source='table', **kw):
    """a handle and its reference over the workload, under the action source and the limit N (0 / None: no limit)"""
    env = VecMapfEnv(w.grid, w.A, None, None, slip, *ec.INEXACT, CRIT[criteria], seed=ec.ORACLE_SEED, start_local=w.start, goal_local=w.goal, **kw)
    if source == 'greedy':
        env.set_policy('greedy')
    elif source == 'table':
        env.set_policy('table', table=w.table, rows=w.rows)
    if N:
        env.set_episode_limit(N)
        assert env.episode_limit == N
    return env, w.oracle(N or 0, slip, criteria, offset=kw.get('env_id_offset', 0))


def _state(env):
    local = env.get_state()[0]
    ages = env.episode_steps()
    env.sync()
    return to_np(local), to_np(ages)


def check_record(res, refs, tag):
    for key in RECORDED:
        for t, r in enumerate(refs):
            assert np.array_equal(raw_bytes(res[key][t]), raw_bytes(r[key])), (tag, key, t)


def check_totals(res, want, tag):
    for key in TOTALS:
        assert np.array_equal(raw_bytes(res[key]), raw_bytes(want[key])), (tag, key)


def check_handle(env, ref, tag):
    local, ages = _state(env)
    assert np.array_equal(local, ref.co.state) and np.array_equal(ages, ref.age) and env.t == ref.co.t, tag


def check_compact_against_reserved(env, local, acts, env_index, res, first=0, window=None):
    """mapf_transitions_compact: the same rows as the reserved form (already checked against the oracle), back to back
    behind the exclusive scan of the windows' lengths; a capacity that is too small drops rows instead of overrunning."""
    N = local.shape[0]
    kw = dict(env_index=env_index, first_branch=first)
    if window is not None:
        kw['max_branches'] = window
    cmp = env.transitions_compact(local, acts, **kw)
    M = res['prob'].shape[1]
    rows = np.minimum(np.maximum(res['count'].astype(np.int64) - first, 0), M)
    assert np.array_equal(cmp['count'], res['count'])
    assert np.array_equal(cmp['offset'].astype(np.int64), np.concatenate([[0], np.cumsum(rows)]))
    for q in range(N):
        o, n = int(cmp['offset'][q]), int(rows[q])
        assert np.array_equal(cmp['next'][o:o + n], res['next'][q, :n]), q
        assert np.array_equal(bits(cmp['prob'][o:o + n]), bits(res['prob'][q, :n])), q
        assert np.array_equal(bits(cmp['reward'][o:o + n]), bits(res['reward'][q, :n])), q
        assert np.array_equal(cmp['done'][o:o + n], res['done'][q, :n]) and np.array_equal(cmp['collision'][o:o + n], res['collision'][q, :n]), q
    total = int(cmp['offset'][N])
    if total > 3:                                                 # too small a capacity: the needed size is reported, nothing overruns
        cap = total // 2
        part = env.transitions_compact(local, acts, capacity=cap, **kw)
        assert int(part['offset'][N]) == total and part['prob'].shape[0] == cap
        assert np.array_equal(bits(part['prob']), bits(cmp['prob'][:cap])) and np.array_equal(part['next'], cmp['next'][:cap])
