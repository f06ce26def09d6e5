"""The reference and the workloads of the joint-table-policy tests (include/mapf_hip.h MAPF_POLICY_JOINT, mapf_set_policy_joint).

The reference is a COMPOSITION, as in tests/conflict_pairs_cases.py: joint_actions computes the [E, A] actions of a step from the
cells on entry by the definition -- a solo agent takes table[offset + c], an agent merged with j takes table[offset + c_i * V + c_j]
-- and the unchanged COracle, LimitOracle, BudgetOracle and PairsOracle are stepped with them: their `run(workload, source, n)`
asks the workload for the step's actions, and the workloads here answer the source 'joint' with joint_actions.

RandomJoint is the random workload: the 20 x 20 random map, a table of a few shared segments of uniform bytes 0..4 (three of V
bytes, four of V * V), offsets picked at random -- half on a segment's start, half anywhere a segment still fits, so segments
overlap -- and a random matching per env, in which the first envs carry the partner geometries a lane-group kernel tells apart.

Merge is the scripted family of the planner's loop, slip 0: a corridor with a one-cell pocket in which two agents meet head on.
tests/test_joint_policy_cases.py recomputes on the CPU that the reference alone shows what the GPU tests rely on."""
import numpy as np

import c_oracle
import conflict_pairs_cases as pc
import episode_budget_cases as bc
import episode_limit_cases as ec
import mapf_oracle as mo
from gym_mapf_amd.envs import policies
from gym_mapf_amd.envs.grid import MapfGrid

# (A, E, what the test sets, the group size the kernel's name shows, FULL / RAGGED)
SHAPES = ((2, 37, {'kernel': 'lane_group'}, 1, 'FULL'), (3, 257, {}, 2, 'RAGGED'), (7, 300, {}, 4, 'RAGGED'), (8, 64, {}, 4, 'FULL'),
          (16, 37, {}, 8, 'FULL'), (32, 37, {}, 16, 'FULL'), (40, 37, {}, 32, 'RAGGED'), (128, 16, {}, 64, 'FULL'))
BROADCAST_SHAPE = (5, 64)
FORM_SHAPES = ((3, 257), (8, 64), (40, 37))
MERGE_AGENTS = (3, 8)
MERGE_WIDTHS = (5, 4)                     # a vertex conflict on step 2, a swap on step 2
MERGE_ENVS, MERGE_EPISODES, MERGE_MAX_STEPS, MERGE_CHUNK = 64, 3, 12, 16


def joint_actions(table, offsets, partners, state, V):
    """u8 [E, A]: the actions of a step whose cells on entry are `state` [E, A], by the definition (offsets, partners: [E, A] or [A])"""
    state = np.asarray(state, np.int64)
    E, A = state.shape
    off = np.broadcast_to(np.asarray(offsets, np.int64).reshape(-1, A), (E, A))
    part = np.broadcast_to(np.asarray(partners, np.int64).reshape(-1, A), (E, A))
    other = np.take_along_axis(state, part, axis=1)
    merged = part != np.arange(A)[None, :]
    return np.asarray(table)[off + np.where(merged, state * V + other, state)].astype(np.uint8)


def geometries(A):
    """the partner geometries of a team of A, as lists of pairs that can stand in ONE matching: a pair inside one lane (2g, 2g + 1),
    a pair in adjacent lanes, the pair (0, A - 1) -- for odd A the last real agent, alone in its lane, merged with agent 0"""
    found = [[(0, 1)]]
    if A >= 4:
        found = [[(A - 2 - A % 2, A - 1 - A % 2)], [(1, 2)], [(0, A - 1)], [(0, A - 1), (2, 3)]]
    elif A == 3:
        found = [[(0, 1)], [(1, 2)], [(0, 2)]]
    return found


def matching(A, forced, rs):
    """partners [A]: the forced pairs, then every remaining agent solo or merged with another remaining one"""
    part = np.arange(A)
    for i, j in forced:
        part[i], part[j] = j, i
    rest = [int(k) for k in rs.permutation(A) if part[k] == k and not any(k in pair for pair in forced)]
    while len(rest) >= 2:
        i, j = rest.pop(), rest.pop()
        if rs.rand() < 0.6:
            part[i], part[j] = j, i
    return part


class RandomJoint:
    """Map, starts, goals and a random joint plan of one (A, E) case; `broadcast`: one matching and one offset row for all envs,
    with the forced pairs of geometries(A)[round]"""

    def __init__(self, A, E, broadcast=False, round=0, seed=0):
        self.A, self.E = A, E
        self.grid = ec.random_map(3)
        _, _, nbr = self.grid.tables()
        self.nbr = np.asarray(nbr)
        self.V = V = self.nbr.shape[0]
        self.start, self.goal = ec.family(self.nbr, E, A, A * 100 + 7)
        rs = np.random.RandomState(1000 * A + E + seed)
        solo_at = [k * V for k in range(3)]
        pair_at = [3 * V + k * V * V for k in range(4)]
        self.table = rs.randint(0, 5, size=3 * V + 4 * V * V).astype(np.uint8)
        geo = geometries(A)
        rows = 1 if broadcast else E
        self.partners = np.stack([matching(A, geo[(round if broadcast else e) % len(geo)] if (broadcast or e < 2 * len(geo)) else [], rs) for e in range(rows)])
        merged = self.partners != np.arange(A)[None, :]
        on_start = rs.rand(rows, A) < 0.5
        start_of = np.where(merged, np.asarray(pair_at)[rs.randint(0, 4, size=(rows, A))], np.asarray(solo_at)[rs.randint(0, 3, size=(rows, A))])
        room = self.table.size - np.where(merged, V * V, V)
        anywhere = (rs.rand(rows, A) * (room + 1)).astype(np.int64)
        self.offsets = np.where(on_start, start_of, np.minimum(anywhere, room)).astype(np.uint32)
        self.partners = self.partners.astype(np.uint16)
        if broadcast:
            self.offsets, self.partners = self.offsets[0], self.partners[0]

    def plan(self):
        return dict(table=self.table, offsets=self.offsets, partners=self.partners)

    def actions(self, source, ref):
        assert source == 'joint'
        return joint_actions(self.table, self.offsets, self.partners, ref.co.state, self.V)

    def oracle(self, N=0, slip=0.2, B=0, pairs=None, offset=0, seed=ec.ORACLE_SEED):
        """the composition: LimitOracle (N = 0: a plain step with a zero `truncated`), under B a BudgetOracle, under `pairs` =
        (n_slots, slots) a PairsOracle around either"""
        return compose(c_oracle.COracle(self.nbr, self.A, self.start, self.goal, slip, *ec.INEXACT, mo.MAKESPAN, seed=seed, env_id_offset=offset), N, B, pairs)


def compose(co, N, B, pairs):
    ref = ec.LimitOracle(co, N)
    if B:
        ref = bc.BudgetOracle(ref, B)
    if pairs is not None:
        ref = pc.PairsOracle(ref, *pairs)
    return ref


def totals_of(refs, base=None):
    """the five totals of reference steps (episode_budget_cases.totals_of), also of steps without a budget"""
    E = refs[0]['reward'].shape[0]
    filled = [dict(r, parked=r.get('parked', np.zeros(E, bool)), live=r.get('live', (r['was_terminal'] == 0).astype(np.uint8))) for r in refs]
    return bc.totals_of(filled, base)


class Merge:
    """The scripted family merge(W, A), slip 0: row 0 is a corridor of W free cells with a one-cell pocket below its middle (row 1,
    column W // 2); agent 0 goes from its left end to its right end and agent 1 the other way.  Under the per-agent shortest-path
    plan they meet on step 2 -- W = 5: both enter the middle cell, a vertex conflict; W = 4: they trade cells, a swap.  The A - 2
    bystanders walk left to right along rows of their own (rows 3, 5, ...: walls between), out of everybody's way.  Every env is
    the same."""

    def __init__(self, W, A, E=MERGE_ENVS):
        assert W >= 4 and A >= 2
        self.W, self.A, self.E = W, A, E
        wall = '@' * W
        rows = ['.' * W, '@' * (W // 2) + '.' + '@' * (W - W // 2 - 1)]
        for _ in range(A - 2):
            rows += [wall, '.' * W]
        self.grid = MapfGrid(rows)
        _, loc_to_int, nbr = self.grid.tables()
        self.nbr = np.asarray(nbr)
        self.V = self.nbr.shape[0]
        cell = lambda r, c: loc_to_int[(r, c)]
        start = [cell(0, 0), cell(0, W - 1)] + [cell(3 + 2 * k, 0) for k in range(A - 2)]
        goal = [cell(0, W - 1), cell(0, 0)] + [cell(3 + 2 * k, W - 1) for k in range(A - 2)]
        self.start = np.tile(np.asarray(start, np.uint16), (E, 1))
        self.goal = np.tile(np.asarray(goal, np.uint16), (E, 1))
        # the solo plan: every agent's shortest path, as set_policy('table') takes it
        self.table, row_of = policies.shortest_path_table(self.grid, goal)
        self.rows = np.asarray([row_of[g] for g in goal], np.uint16)
        # the merged plan: (0, 1) replanned jointly, the bystanders as they were
        self.joint = policies.join_plan(self.V, A, {k: self.table[self.rows[k]] for k in range(2, A)},
                                        {(0, 1): policies.pair_shortest_path_rows(self.grid, goal[0], goal[1])})

    def plan(self):
        table, offsets, partners = self.joint
        return dict(table=table, offsets=offsets, partners=partners)

    def actions(self, source, ref):
        state = ref.co.state.astype(np.int64)
        if source == 'table':
            return self.table[self.rows.astype(np.int64)[None, :], state]
        assert source == 'joint'
        return joint_actions(*self.joint, state, self.V)

    def evaluated(self, source, slip=0.0, slots=None):
        """the reference of policies.evaluate(env, MERGE_EPISODES, MERGE_MAX_STEPS, chunk=MERGE_CHUNK) on a fresh env that counts pairs
        in one slot (slots: per env): (the run's totals with goal_ends, the matrix)"""
        co = c_oracle.COracle(self.nbr, self.A, self.start, self.goal, slip, *ec.INEXACT, mo.MAKESPAN, seed=ec.ORACLE_SEED)
        ref = compose(co, MERGE_MAX_STEPS, MERGE_EPISODES, (1, None) if slots is None else (self.E, slots))
        launches = -(-MERGE_EPISODES * MERGE_MAX_STEPS // MERGE_CHUNK)
        tot = bc.totals_of(ref.run(self, source, launches * MERGE_CHUNK))
        assert not ref.left.any()
        tot['goal_ends'] = tot['episodes'] - tot['collisions']
        return tot, ref.M


_merges = {}


def merge(W, A):
    """(computed once, shared, left unchanged)"""
    if (W, A) not in _merges:
        _merges[W, A] = Merge(W, A)
    return _merges[W, A]
