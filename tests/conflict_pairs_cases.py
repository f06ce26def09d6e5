"""The reference and the scripted workload of the conflict-matrix tests (include/mapf_hip.h, mapf_set_conflict_pairs).

The reference is a COMPOSITION over tests/episode_budget_cases.py's BudgetOracle, tests/episode_limit_cases.py's LimitOracle or the
plain C oracle, all unchanged, following the definition literally.  Per reference step:
  1. prev = a copy of co.state, the cells on entry;
  2. the wrapped oracle's step; next = ref['local'], the sampled cells before any reset;
  3. for the envs that were neither parked nor terminal on entry and every i < j: next[i] == next[j] adds one to M[slot][i][j],
     prev[i] == next[j] and prev[j] == next[i] adds one to M[slot][j][i].

The random workload is episode_limit_cases.Workload under episode_budget_cases.PASSES; the scripted family every_pair(A) makes every
agent pair conflict exactly once, as a vertex conflict in one env and as a swap in another.  tests/test_conflict_pairs_cases.py
recomputes on the CPU that the reference alone shows what the GPU tests rely on."""
import itertools

import numpy as np

import c_oracle
import episode_budget_cases as bc
import episode_limit_cases as ec
import mapf_oracle as mo
from gym_mapf_amd.envs import ACTIONS
from gym_mapf_amd.envs.grid import MapfGrid

SHAPES = bc.SHAPES + ((5, 64), (40, 37), (128, 37))
EVERY_PAIR_AGENTS = (2, 3, 5, 8, 16, 32, 40, 64, 128)
STAY, RIGHT, LEFT = (ACTIONS.index(name) for name in ('STAY', 'RIGHT', 'LEFT'))


def pair_counts(prev, nxt):
    """u64 [E, A, A]: per env the step's matrix -- [i][j], i < j, is 1 for a vertex conflict of (i, j), [j][i] is 1 for a swap"""
    prev, nxt = prev.astype(np.int64), nxt.astype(np.int64)
    A = prev.shape[1]
    upper = np.triu(np.ones((A, A), bool), 1)
    vertex = nxt[:, :, None] == nxt[:, None, :]
    swap = (prev[:, :, None] == nxt[:, None, :]) & (prev[:, None, :] == nxt[:, :, None])      # symmetric in (i, j)
    return ((vertex & upper) | (swap & upper.T)).astype(np.uint64)


def add_pairs(M, slots, prev, nxt, live, chunk=1 << 22):
    """M[slots[e]] += pair_counts of the live envs, a few envs at a time (128 agents: 16384 entries per env)"""
    rows = np.flatnonzero(live)
    per = max(1, chunk // (prev.shape[1] ** 2))
    for at in range(0, rows.size, per):
        r = rows[at:at + per]
        np.add.at(M, slots[r], pair_counts(prev[r], nxt[r]))


class PairsOracle:
    """A BudgetOracle, a LimitOracle or a COracle stepped under a conflict matrix: see the module's docstring.  Everything the
    wrapped reference has (co, age, left, set_limit, ...) reads through."""

    def __init__(self, inner, n_slots=1, slots=None):
        self.inner = inner
        self.co = getattr(inner, 'co', inner)
        self.set_pairs(n_slots, slots)

    def __getattr__(self, name):                # (only what the wrapper itself lacks)
        return getattr(self.inner, name)

    def set_pairs(self, n_slots=1, slots=None):
        """every mapf_set_conflict_pairs call zeroes M"""
        self.slots = np.zeros(self.co.E, np.int64) if slots is None else np.asarray(slots, np.int64)
        assert self.slots.shape == (self.co.E,) and (self.slots < n_slots).all()
        self.M = np.zeros((n_slots, self.co.A, self.co.A), np.uint64)

    def take(self, zero=False):
        M = self.M.copy()
        if zero:
            self.M[:] = 0
        return M

    def step(self, actions, auto_reset=True):
        prev = self.co.state.copy()
        if isinstance(self.inner, bc.BudgetOracle):
            assert auto_reset
            ref = self.inner.step(actions)
        elif isinstance(self.inner, ec.LimitOracle):
            ref = self.inner.step(actions, auto_reset=auto_reset)
        else:
            ref = self.inner.step(actions, None, auto_reset=auto_reset)
        live = (ref['was_terminal'] == 0) & ~ref.get('parked', np.zeros(self.co.E, bool))
        add_pairs(self.M, self.slots, prev, ref['local'], live)
        ref['prev'], ref['counted'] = prev, live
        return ref

    def run(self, workload, source, n_steps, auto_reset=True):
        """n_steps reference steps under the action source; every step's dict also keeps its joint `actions`"""
        refs = []
        for _ in range(n_steps):
            actions = workload.actions(source, self)
            refs.append(dict(self.step(actions, auto_reset=auto_reset), actions=actions))
        return refs


def pair_facts(refs):
    """Of a list of PairsOracle steps: (vertex counts, swap counts, steps of an env with two or more conflicting pairs, steps of an
    env with three agents on one cell)"""
    vertex = swap = multi = triple = 0
    for r in refs:
        rows = np.flatnonzero(r['counted'] & (r['collision'] != 0))
        if not rows.size:
            continue
        c = pair_counts(r['prev'][rows], r['local'][rows])
        A = c.shape[1]
        upper = np.triu(np.ones((A, A), bool), 1)
        vertex += int(c[:, upper].sum())
        swap += int(c[:, upper.T].sum())
        multi += int((c.sum(axis=(1, 2)) >= 2).sum())
        nxt = np.sort(r['local'][rows].astype(np.int64), axis=1)
        if A >= 3:
            triple += int(((nxt[:, 2:] == nxt[:, :-2]).any(axis=1)).sum())
    return vertex, swap, multi, triple


class EveryPair:
    """The scripted family every_pair(A): an open map of 3 rows x max(2A, 3) columns, slip 0, streamed actions, ONE step,
    E = A (A - 1) envs.  Env 2p + s belongs to the p-th pair (i, j) of itertools.combinations(range(A), 2): every agent k starts at
    (row 2, column 2k) with its goal at (row 1, column 2k) and STAYs, but agent i starts at (0, 0) and moves RIGHT, and agent j starts
    at (0, 1) if s is 1 -- a swap -- or at (0, 2) if s is 0 -- a vertex conflict -- and moves LEFT.  With one slot every off-diagonal
    entry of M is exactly 1 and the diagonal 0: a pair met twice shows a 2, a pair never met a 0."""

    REWARDS = ec.INEXACT

    def __init__(self, A):
        self.A, self.E = A, A * (A - 1)
        W = max(2 * A, 3)
        self.grid = MapfGrid(['.' * W] * 3)
        _, loc_to_int, nbr = self.grid.tables()
        self.nbr = np.asarray(nbr)
        cell = lambda r, c: loc_to_int[(r, c)]
        self.pairs = list(itertools.combinations(range(A), 2))
        start = np.tile(np.asarray([cell(2, 2 * k) for k in range(A)], np.uint16), (self.E, 1))
        self.goal = np.tile(np.asarray([cell(1, 2 * k) for k in range(A)], np.uint16), (self.E, 1))
        actions = np.full((self.E, A), STAY, np.uint8)
        for p, (i, j) in enumerate(self.pairs):
            for s in (0, 1):
                e = 2 * p + s
                start[e, i], start[e, j] = cell(0, 0), cell(0, 1 if s else 2)
                actions[e, i], actions[e, j] = RIGHT, LEFT
        self.start, self.actions1 = start, actions
        self.is_swap = (np.arange(self.E) % 2).astype(bool)

    def oracle(self, n_slots=1, slots=None, seed=ec.ORACLE_SEED):
        co = c_oracle.COracle(self.nbr, self.A, self.start, self.goal, 0.0, *self.REWARDS, mo.MAKESPAN, seed=seed)
        return PairsOracle(co, n_slots, slots)

    def expected(self):
        """one slot: ones off the diagonal"""
        return (1 - np.eye(self.A, dtype=np.uint64))[None]


def every_pair(A):
    return EveryPair(A)
