"""The table policy's host side (no GPU): the shortest-path tables of envs/policies.py against a breadth-first search
restated here, the row of a single-agent local-view policy, the reason the feature exists (through the C oracle: on the
bench workload the shortest-path plan reaches goals, the greedy policy reaches none), and the argument checks of
mapf_set_policy_table that need no device."""
import collections
import ctypes

import numpy as np
import pytest

import c_oracle
import mapf_oracle as mo
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import ACTIONS, map_name_to_files
from gym_mapf_amd.envs.grid import MapfGrid
from gym_mapf_amd.envs.mapf_env import MapfEnv
from gym_mapf_amd.envs.policies import row_from_policy, shortest_path_table
from gym_mapf_amd.envs.utils import get_local_view, parse_map_file
from gym_mapf_amd.envs.vec_env import OptimizationCriteria

STAY, UP, RIGHT, DOWN, LEFT = (ACTIONS.index(n) for n in ('STAY', 'UP', 'RIGHT', 'DOWN', 'LEFT'))


def _bfs(nbr, goal):
    """Distance of every cell to `goal` over the four noise-free moves, by the textbook queue (-1: unreachable).
    Searched BACKWARDS over explicit predecessor lists, so it does not lean on the moves being symmetric."""
    V = nbr.shape[0]
    pred = [[] for _ in range(V)]
    for c in range(V):
        for a in (UP, RIGHT, DOWN, LEFT):
            if int(nbr[c, a]) != c:
                pred[int(nbr[c, a])].append(c)
    dist = [-1] * V
    dist[goal] = 0
    queue = collections.deque([goal])
    while queue:
        v = queue.popleft()
        for c in pred[v]:
            if dist[c] < 0:
                dist[c] = dist[v] + 1
                queue.append(c)
    return dist


def _check_rows(grid, goals):
    _, _, nbr = grid.tables()
    V = nbr.shape[0]
    table, row_of = shortest_path_table(grid, goals)
    assert table.dtype == np.uint8 and table.shape == (len(set(int(g) for g in goals)), V)
    assert sorted(row_of) == sorted(set(int(g) for g in goals)) and sorted(row_of.values()) == list(range(table.shape[0]))
    n_unreachable = 0
    for goal, r in row_of.items():
        dist = _bfs(nbr, goal)
        row = table[r]
        assert row[goal] == STAY
        for c in range(V):
            if dist[c] < 0:
                n_unreachable += 1
                assert row[c] == STAY, (goal, c)
                continue
            if c == goal:
                continue
            # the ACTIONS-order tie-break, restated: the FIRST of UP, RIGHT, DOWN, LEFT that lands one step closer
            want = next(a for a in (UP, RIGHT, DOWN, LEFT) if dist[int(nbr[c, a])] == dist[c] - 1)
            assert row[c] == want, (goal, c, row[c], want)
        # following the row noise-free arrives in exactly the BFS distance
        for c in range(V):
            if dist[c] > 0:
                at, steps = c, 0
                while at != goal:
                    at = int(nbr[at, row[at]])
                    steps += 1
                    assert steps <= dist[c], (goal, c)
                assert steps == dist[c]
    return table, row_of, n_unreachable


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_shortest_path_table_matches_a_restated_bfs_on_random_maps(seed):
    rs = np.random.RandomState(900 + seed)
    lines = [''.join('@' if rs.rand() < 0.15 else '.' for _ in range(20)) for _ in range(20)]
    grid = MapfGrid(lines)
    V = len(grid.tables()[0])
    goals = rs.choice(V, size=12, replace=False)
    _check_rows(grid, list(goals) + [int(goals[0])])              # (a repeated goal makes one row)


def test_unreachable_cells_stay_and_ties_break_in_actions_order():
    # two rooms without a door: the right room cannot reach a goal in the left one
    grid = MapfGrid(['...@..', '...@..', '...@..'])
    valid, l2i, nbr = grid.tables()
    goal = l2i[(1, 1)]
    table, row_of, n_unreachable = _check_rows(grid, [goal])
    assert n_unreachable == 6
    row = table[row_of[goal]]
    assert row[l2i[(0, 5)]] == STAY and row[l2i[(2, 4)]] == STAY
    # from a corner both a vertical and a horizontal move are one step closer: UP comes before RIGHT, RIGHT before DOWN,
    # DOWN before LEFT
    assert row[l2i[(2, 0)]] == UP and row[l2i[(0, 0)]] == RIGHT and row[l2i[(0, 2)]] == DOWN and row[l2i[(2, 2)]] == UP
    assert row[l2i[(1, 0)]] == RIGHT and row[l2i[(1, 2)]] == LEFT and row[l2i[(0, 1)]] == DOWN and row[l2i[(2, 1)]] == UP
    with pytest.raises(ValueError):
        shortest_path_table(grid, [len(valid)])


def test_shortest_path_table_on_room_32_32_4():
    import bench
    grid, _, nbr, start, goal = bench.workload_tables(bench.CONFIGS['c3'], 6, 0)
    assert nbr.shape[0] == 682
    goals = np.unique(goal)
    assert goals.size == 46                                       # the six bench scenarios: 46 distinct goals, a 31 KB table
    table, row_of, n_unreachable = _check_rows(grid, goals)
    assert table.nbytes == 46 * 682 and n_unreachable == 0


def test_row_from_policy_of_a_one_agent_local_view():
    grid = MapfGrid(['....', '.@..', '....'])
    env = MapfEnv(grid, 2, ((0, 0), (2, 3)), ((2, 0), (0, 3)), 0.1, -1.0, 1.0, -1.0, OptimizationCriteria.SoC)
    view = get_local_view(env, [1])
    assert view.n_agents == 1
    table, row_of = shortest_path_table(grid, [view.loc_to_int[view.agents_goals[0]]])
    planned = table[0]
    row = row_from_policy(view, lambda s: int(planned[s]))        # a policy(s) -> a in the reference's sense
    assert row.dtype == np.uint8 and np.array_equal(row, planned)
    # the state integer of a one-agent env IS the cell's local id
    for c, loc in enumerate(view.valid_locations):
        assert view.locations_to_state((loc,)) == c
    with pytest.raises(ValueError):
        row_from_policy(view, lambda s: 5)
    with pytest.raises(ValueError):
        row_from_policy(env, lambda s: 0)


def test_shortest_path_plan_reaches_goals_on_the_bench_workload_where_greedy_reaches_none():
    """Why the feature exists, through the C oracle alone: room-32-32-4, 8 agents, slip 0.2, the six bench scenarios,
    1536 envs x 256 steps with auto-reset, seed 21.  The Manhattan-greedy policy sticks at the room walls (no episode ends
    at its goal); the shortest-path table finishes episodes at the goal -- and collides, its agents ignore each other."""
    import bench
    E, A, T = 1536, 8, 256
    grid, _, nbr, start, goal = bench.workload_tables(bench.CONFIGS['c3'], E, 0)
    valid = grid.tables()[0]
    rc = np.asarray([r | (c << 16) for r, c in valid], np.uint32)
    table, row_of = shortest_path_table(grid, goal)
    lookup = np.zeros(nbr.shape[0], np.int64)
    for g, r in row_of.items():
        lookup[g] = r
    rows = lookup[goal.astype(np.int64)]
    counts = {}
    for name in ('table', 'greedy'):
        co = c_oracle.COracle(nbr, A, start, goal, 0.2, -1000.0, 100.0, -1.0, mo.MAKESPAN, seed=21)
        goals_reached = collisions = 0
        for t in range(T):
            act = table[rows, co.state.astype(np.int64)] if name == 'table' else co.greedy_actions(rc)
            ref = co.step(act, auto_reset=True)
            goals_reached += int(((ref['done'] != 0) & (ref['collision'] == 0)).sum())
            collisions += int((ref['collision'] != 0).sum())
        counts[name] = (goals_reached, collisions)
    print('goal / collision episodes:', counts)
    assert counts['greedy'] == (0, 660), counts
    assert counts['table'] == (1504, 18906), counts


def test_set_policy_table_validates_its_arguments_without_a_device():
    lib = nat.load()
    assert nat.MAPF_POLICY_TABLE == 2 and nat.MAPF_POLICY_ROWS_BROADCAST == 1
    table = np.zeros(8, np.uint8)
    rows = np.zeros(2, np.uint16)
    assert lib.mapf_set_policy_table(None, table.ctypes.data, 1, rows.ctypes.data, 0) == nat.MAPF_EINVAL
    assert b'null handle' in lib.mapf_last_error()
    # the other argument checks come before the handle is touched, so a value that is never dereferenced shows them
    fake = ctypes.c_void_p(0x1000)
    for args, word in (((None, 1, rows.ctypes.data, 0), b'table'), ((table.ctypes.data, 1, None, 0), b'row_index'),
                       ((table.ctypes.data, 0, rows.ctypes.data, 0), b'n_rows'), ((table.ctypes.data, 65537, rows.ctypes.data, 0), b'n_rows'),
                       ((table.ctypes.data, 1, rows.ctypes.data, 2), b'flags')):
        assert lib.mapf_set_policy_table(fake, *args) == nat.MAPF_EINVAL, args
        assert word in lib.mapf_last_error(), (args, lib.mapf_last_error())
