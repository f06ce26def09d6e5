"""The reference and the workload of the episode-limit tests (include/mapf_hip.h, mapf_set_episode_limit).

The reference is a COMPOSITION of the unchanged C oracle, following the definition's rules literally:
  1. co.step(actions, auto_reset=False);
  2. live = was_terminal == 0, age[live] += 1 (saturating at 2^32 - 1);
  3. truncated = live & ~done & (age >= N);
  4. with auto-reset: co.reset(done | truncated), age[done | truncated] = 0.

The workload is chosen so that the reference alone shows every outcome -- episodes that end at the goal, episodes that end in a
collision, truncated episodes, and steps from a terminal state: a random 20 x 20 map (V = 341), starts on random cells, every env's
goals 3 - e % 3 noise-free moves from its starts, the agents driven by their shortest-path rows.  tests/test_episode_limit_cases.py
recomputes the outcome counts on the CPU, so a seed that stops providing an outcome fails there and not on the GPU."""
import numpy as np

import c_oracle
import mapf_oracle as mo
import philox
from gym_mapf_amd.envs.grid import MapfGrid
from gym_mapf_amd.envs.policies import shortest_path_table

INEXACT = (-0.3, 0.7, -0.1)                    # rewards on which float64 rounds (tests/test_gpu_parity.py)
ORACLE_SEED = 21
T_TOTAL, LAUNCHES = 36, (5, 1, 18, 12)         # ages cross launch boundaries and every phase of the four-step Philox block
SOURCES = ('stream', 'policy', 'greedy', 'table')
CRITERIA = {'Makespan': mo.MAKESPAN, 'SoC': mo.SOC}
# (n_agents, n_envs): L = 1, ghost slots, full groups, L = 16; a ragged and a whole batch
SHAPES = tuple((A, E) for A in (2, 3, 8, 16, 32) for E in (37, 64))
# (N, slip): every live step that is not done truncates; the limit and the goals' distance interleave; no slip (N = 4 would
# never truncate there: every goal is at most three moves away)
LIMITS = ((1, 0.2), (4, 0.2), (2, 0.0))
AGE_MAX = 0xFFFFFFFF
# Passes whose workload cannot show one of the outcomes, whatever runs it (the other passes of the same shape show it):
#   three agents without slip walk disjoint shortest paths of at most three moves and never meet in these 64 envs;
#   32 agents under N = 1 are back on their start cells after every step, and no team of 32 stands one move from all its goals.
WITHOUT = {(3, 64, 2, 0.0): 'collisions', (32, 37, 1, 0.2): 'goals'}


def check_outcomes(A, E, N, slip, source, counts):
    """What every pass asserts on the oracle's side: truncations always; collision ends except at two agents; goal ends wherever the
    agents follow their shortest paths (the random policy stream reaches almost no goal)."""
    goals, colls, truncs = counts[:3]
    missing = WITHOUT.get((A, E, N, slip))
    assert truncs > 0, (A, E, N, slip, source, counts)
    assert colls > 0 or A == 2 or missing == 'collisions', (A, E, N, slip, source, counts)
    assert goals > 0 or source == 'policy' or missing == 'goals', (A, E, N, slip, source, counts)


def random_map(seed, size=20, p=0.15):
    rs = np.random.RandomState(seed)
    return MapfGrid([''.join('@' if rs.rand() < p else '.' for _ in range(size)) for _ in range(size)])


def family(nbr, E, A, seed):
    rs = np.random.RandomState(seed); V = nbr.shape[0]
    start = np.argsort(rs.rand(E, V), axis=1)[:, :A].astype(np.uint16)
    goal = start.astype(np.int64).copy()
    for k in range(3):                       # env e walks its goals 3 - e % 3 noise-free moves away from the starts
        mv = rs.randint(1, 5, size=(E, A))
        nxt = nbr[goal, mv].astype(np.int64)
        goal = np.where((np.arange(E) % 3 >= k)[:, None], nxt, goal)
    return start, goal.astype(np.uint16)


class Workload:
    """Map, starts, goals and the shortest-path table of one (A, E, N) case."""

    def __init__(self, A, E, N):
        self.A, self.E, self.N = A, E, N
        self.grid = random_map(3)
        valid, _, nbr = self.grid.tables()
        self.nbr = np.asarray(nbr)
        self.cell_rc = np.asarray([r | (c << 16) for r, c in valid], np.uint32)
        self.start, self.goal = family(self.nbr, E, A, A * 100 + N)
        self.table, row_of = shortest_path_table(self.grid, self.goal)
        self.rows = np.vectorize(row_of.get)(self.goal.astype(np.int64)).astype(np.uint16)

    def oracle(self, N, slip, criteria='Makespan', seed=ORACLE_SEED, offset=0):
        co = c_oracle.COracle(self.nbr, self.A, self.start, self.goal, slip, *INEXACT, CRITERIA[criteria], seed=seed, env_id_offset=offset)
        return LimitOracle(co, N)

    def actions(self, source, ref):
        """The joint actions of the step the oracle is about to take, u8 [E, A]: what the kernel's action source produces."""
        co = ref.co
        if source in ('stream', 'table'):      # the agents' shortest-path rows (streamed: the same bytes computed on the host)
            return self.table[self.rows.astype(np.int64), co.state.astype(np.int64)]
        if source == 'greedy':
            return co.greedy_actions(self.cell_rc)
        assert source == 'policy'
        return philox.random_actions_np(co.seed, co.off + np.arange(self.E, dtype=np.uint64), co.t, self.A)


class LimitOracle:
    """The C oracle stepped under an episode limit N (0 = none): see the module's docstring."""

    def __init__(self, co, N):
        self.co, self.N = co, int(N)
        self.age = np.zeros(co.E, np.uint32)

    def set_limit(self, N):
        self.N = int(N)
        self.age[:] = 0                        # every mapf_set_episode_limit call zeroes the ages

    def reset(self, mask=None):
        self.co.reset(mask)
        if self.N:
            self.age[slice(None) if mask is None else np.asarray(mask).astype(bool)] = 0

    def step(self, actions, uniforms=None, auto_reset=True):
        ref = self.co.step(actions, uniforms, auto_reset=False)
        done = ref['done'] != 0
        trunc = np.zeros(self.co.E, bool)
        if self.N:
            live = ref['was_terminal'] == 0
            age = self.age.astype(np.uint64)
            age[live] += 1
            age = np.minimum(age, AGE_MAX)
            trunc = live & ~done & (age >= self.N)
            self.age = age.astype(np.uint32)
        if auto_reset:
            back = done | trunc
            self.co.reset(back)
            self.age[back] = 0
        ref['truncated'] = trunc.astype(np.uint8)
        return ref

    def run(self, workload, source, n_steps, auto_reset=True):
        """n_steps reference steps under the action source; every step's dict also keeps its joint `actions`"""
        refs = []
        for _ in range(n_steps):
            actions = workload.actions(source, self)
            refs.append(dict(self.step(actions, auto_reset=auto_reset), actions=actions))
        return refs


def outcome_counts(refs):
    """(goal ends, collision ends, truncations, terminal-start no-ops) of a list of reference steps"""
    goals = sum(int(((r['done'] != 0) & (r['collision'] == 0) & (r['was_terminal'] == 0)).sum()) for r in refs)
    colls = sum(int((r['collision'] != 0).sum()) for r in refs)
    truncs = sum(int(r['truncated'].sum()) for r in refs)
    noops = sum(int(r['was_terminal'].sum()) for r in refs)
    return goals, colls, truncs, noops


def totals_of(refs, base=None):
    """returns / episodes / collisions / truncations of the steps, added in step order (to `base` when a call accumulates)"""
    E = refs[0]['reward'].shape[0]
    tot = dict(returns=np.zeros(E), episodes=np.zeros(E, np.uint32), collisions=np.zeros(E, np.uint32), truncations=np.zeros(E, np.uint32)) \
        if base is None else {k: v.copy() for k, v in base.items()}
    for r in refs:
        tot['returns'] = tot['returns'] + r['reward']
        tot['episodes'] = tot['episodes'] + r['done'].astype(np.uint32)
        tot['collisions'] = tot['collisions'] + r['collision'].astype(np.uint32)
        tot['truncations'] = tot['truncations'] + r['truncated'].astype(np.uint32)
    return tot
