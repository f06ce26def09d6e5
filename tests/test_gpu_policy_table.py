"""GPU parity of the table policy (MAPF_POLICY_TABLE, VecMapfEnv.set_policy('table', ...)): fused rollouts that follow a
per-agent lookup table, in every kernel family, against the C oracle stepped with table[rows, oracle state] -- cells,
flags and the float64 bit patterns of reward and prob, bit for bit.  Every bad input here is one the host rejects:
nothing provokes a device fault."""
import numpy as np
import pytest

import c_oracle
from conftest import set_tune
import mapf_oracle as mo
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs.grid import MapfGrid
from gym_mapf_amd.envs.policies import shortest_path_policy, shortest_path_table
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from parity_checks import bits, to_np

pytestmark = pytest.mark.gpu
R = (-1000.0, 100.0, -1.0)
# constants on which float64 rounds (see tests/test_gpu_parity.py): n * living, r_x + living and the returns' sums have one
# admissible operation order each, and any other changes bits
INEXACT = (-0.3, 0.7, -0.1)
CRIT = {'Makespan': (OptimizationCriteria.Makespan, mo.MAKESPAN), 'SoC': (OptimizationCriteria.SoC, mo.SOC)}


def _state(env):
    """the handle's state on the host: in device mode get_state only ENQUEUES its copy on the env's stream, which the reader's stream
    does not wait for"""
    local = env.get_state()[0]
    env.sync()
    return to_np(local)


def _random_map(seed, size=20, p=0.15):
    rs = np.random.RandomState(seed)
    return MapfGrid([''.join('@' if rs.rand() < p else '.' for _ in range(size)) for _ in range(size)])


def _random_cells(rs, E, V, A):
    return np.argsort(rs.rand(E, V), axis=1)[:, :A].astype(np.uint16)


def _bench_tables(name, E, offset=0):
    import bench
    grid, _, nbr, start, goal = bench.workload_tables(bench.CONFIGS[name], E, offset)
    return grid, nbr, start, goal


def _full_rows(rows, E, A):
    return np.broadcast_to(np.asarray(rows, np.int64).reshape(-1, A), (E, A))


def _oracle_steps(co, table, rows, T, auto_reset=True):
    """T oracle steps under the table policy: the action of agent i of env e is table[rows[e, i], state[e, i]]."""
    out, goals, colls = [], 0, 0
    for _ in range(T):
        ref = co.step(table[rows, co.state.astype(np.int64)], auto_reset=auto_reset)
        goals += int(((ref['done'] != 0) & (ref['collision'] == 0) & (ref['was_terminal'] == 0)).sum())
        colls += int((ref['collision'] != 0).sum())
        out.append(ref)
    return out, goals, colls


def _check_record(res, refs, tag, t0=0):
    for t, ref in enumerate(refs):
        assert np.array_equal(to_np(res['local'][t0 + t]), ref['local']), (tag, t)
        assert np.array_equal(bits(to_np(res['reward'][t0 + t])), bits(ref['reward'])), (tag, t)
        assert np.array_equal(bits(to_np(res['prob'][t0 + t])), bits(ref['prob'])), (tag, t)
        assert np.array_equal(to_np(res['done'][t0 + t]), ref['done']) and np.array_equal(to_np(res['collision'][t0 + t]), ref['collision']), (tag, t)


def _check_totals(res, refs, tag, base=None):
    ret = np.zeros(refs[0]['reward'].shape[0]) if base is None else base['returns'].copy()
    epi = np.zeros(ret.shape[0], np.uint32) if base is None else base['episodes'].copy()
    col = np.zeros(ret.shape[0], np.uint32) if base is None else base['collisions'].copy()
    for ref in refs:
        ret = ret + ref['reward']                                 # float64 adds in step order, as the kernels do
        epi = epi + ref['done'].astype(np.uint32)
        col = col + ref['collision'].astype(np.uint32)
    assert np.array_equal(bits(to_np(res['returns'])), bits(ret)), tag
    assert np.array_equal(to_np(res['episodes']), epi) and np.array_equal(to_np(res['collisions']), col), tag
    return dict(returns=ret, episodes=epi, collisions=col)


def _run_parity(grid, nbr, start, goal, A, table, rows, criteria='Makespan', kernel='auto', T=24, fail_prob=0.2, seed=21,
                expect=None, device_arrays=False, offset=0, rewards=R):
    """record rollout + totals-only rollout + accumulate, all against the oracle; returns (goal episodes, collision episodes)."""
    crit, ocrit = CRIT[criteria]
    E = max(start.shape[0], goal.shape[0]) if start.ndim == 2 else 1
    env = VecMapfEnv(grid, A, None, None, fail_prob, *rewards, crit, seed=seed, start_local=start, goal_local=goal, kernel=kernel,
                     device_arrays=device_arrays, env_id_offset=offset)
    co = c_oracle.COracle(nbr, A, start, goal, fail_prob, *rewards, ocrit, seed=seed, env_id_offset=offset)
    E = env.n_envs
    env.set_policy('table', table=table, rows=rows)
    assert env.policy == 'table'
    full = _full_rows(rows, E, A)
    res = env.rollout(T, auto_reset=True, record=True)
    env.sync()
    name = env.last_kernel('rollout')
    assert 'TABLE' in name and 'STREAM' not in name and 'POLICY' not in name, name
    if expect:
        assert expect in name, name
    refs, goals, colls = _oracle_steps(co, table, full, T)
    _check_record(res, refs, name)
    totals = _check_totals(res, refs, name)
    assert np.array_equal(_state(env), co.state), name
    # totals only, then accumulated into the same arrays
    res2 = env.rollout(T // 2, auto_reset=True)
    env.sync()
    name2 = env.last_kernel('rollout')                            # (the thread-per-env kernel is one instance for both)
    assert 'TABLE' in name2 and ('TOTALS' in name2 or name2.startswith('rollout_kernel_table')), name2
    refs2, g2, c2 = _oracle_steps(co, table, full, T // 2)
    base = _check_totals(res2, refs2, 'totals ' + name)
    res3 = env.rollout(5, auto_reset=True, accumulate_into=res2)
    env.sync()
    refs3, g3, c3 = _oracle_steps(co, table, full, 5)
    _check_totals(res3, refs3, 'accumulate ' + name, base=base)
    assert np.array_equal(_state(env), co.state) and env.t == co.t
    env.close()
    del totals
    return goals + g2 + g3, colls + c2 + c3, name


def _random_case(A, E, seed, broadcast_rows=False, n_rows=9):
    grid = _random_map(seed)
    nbr = grid.tables()[2]
    V = nbr.shape[0]
    rs = np.random.RandomState(seed + 1)
    start, goal = _random_cells(rs, E, V, A), _random_cells(rs, E, V, A)
    table = rs.randint(0, 5, size=(n_rows, V)).astype(np.uint8)   # uniform bytes 0..4: rows no shortest path produces
    rows = rs.randint(0, n_rows, size=(A,) if broadcast_rows else (E, A)).astype(np.uint16)
    return grid, nbr, start, goal, table, rows


TABLE_CASES = [
    (2, 300, 'thread_per_env', 'Makespan', 'rollout_kernel_table<A=2'), (5, 300, 'thread_per_env', 'SoC', 'rollout_kernel_table<A=5'),
    (3, 257, 'lane_group', 'Makespan', 'lg_rollout_kernel_table<L=2,RAGGED'), (40, 64, 'lane_group', 'SoC', 'lg_rollout_kernel_table<L=32'),
    (128, 16, 'lane_group', 'Makespan', 'lg_rollout_kernel_table<L=64'), (7, 1000, 'auto', 'SoC', 'lg_rollout_kernel_table<L=4,RAGGED'),
]


@pytest.mark.parametrize('n_agents,n_envs,kernel,criteria,expect', TABLE_CASES)
def test_random_table_in_the_thread_per_env_and_lane_group_kernels(n_agents, n_envs, kernel, criteria, expect, rewards=R):
    grid, nbr, start, goal, table, rows = _random_case(n_agents, n_envs, 800 + n_agents, broadcast_rows=(n_agents == 5))
    _run_parity(grid, nbr, start, goal, n_agents, table, rows, criteria=criteria, kernel=kernel, expect=expect, T=20, rewards=rewards)


@pytest.mark.parametrize('n_agents,n_envs,kernel,criteria,expect', TABLE_CASES)
def test_random_table_with_inexact_constants_in_the_thread_per_env_and_lane_group_kernels(n_agents, n_envs, kernel, criteria, expect):
    test_random_table_in_the_thread_per_env_and_lane_group_kernels(n_agents, n_envs, kernel, criteria, expect, rewards=INEXACT)


PACKED_TABLE_CASES = [
    (8, 8192, 'Makespan', 'lq_rollout_kernel_table<Q=4,K=2'), (8, 16448, 'SoC', 'lq_rollout_kernel_table<Q=4,K=2'),
    (16, 4096, 'Makespan', 'lq_rollout_kernel_table<Q=8,K=2'),
]


@pytest.mark.parametrize('lds', [0, 1])
@pytest.mark.parametrize('n_agents,n_envs,criteria,expect', PACKED_TABLE_CASES)
def test_random_table_in_the_packed_kernels_both_table_forms(monkeypatch, n_agents, n_envs, criteria, expect, lds, rewards=R):
    set_tune(monkeypatch, policy_table_lds=lds)
    grid, nbr, start, goal, table, rows = _random_case(n_agents, n_envs, 820 + n_agents, broadcast_rows=(n_envs == 16448))
    _, _, name = _run_parity(grid, nbr, start, goal, n_agents, table, rows, criteria=criteria, expect=expect, T=20, rewards=rewards)
    assert ('TABLE_LDS' if lds else 'TABLE_GLOBAL') in name, name


@pytest.mark.parametrize('lds', [0, 1])
@pytest.mark.parametrize('n_agents,n_envs,criteria,expect', PACKED_TABLE_CASES)
def test_random_table_with_inexact_constants_in_the_packed_kernels_both_table_forms(monkeypatch, n_agents, n_envs, criteria, expect, lds):
    test_random_table_in_the_packed_kernels_both_table_forms(monkeypatch, n_agents, n_envs, criteria, expect, lds, rewards=INEXACT)


@pytest.mark.parametrize('k', [2, 4])
def test_shortest_path_on_room_32_32_4_packed(monkeypatch, k):
    """The bench map and scenarios, 8 agents x 8192 envs, two and four agents per lane; both outcomes occur in the oracle's
    own run (episodes that end at the goal, episodes that end in a collision)."""
    set_tune(monkeypatch, k=k)
    E, A = 8192, 8
    grid, nbr, start, goal = _bench_tables('c3', E)
    table, row_of = shortest_path_table(grid, goal)
    rows = np.vectorize(row_of.get)(goal.astype(np.int64)).astype(np.uint16)
    goals, colls, _ = _run_parity(grid, nbr, start, goal, A, table, rows, T=96, expect='lq_rollout_kernel_table<Q=%d,K=%d' % (A // k, k))
    assert goals > 0 and colls > 0, (goals, colls)


def test_c2_shape_shortest_path_on_empty_16_16_with_its_25_scenarios():
    """BASELINE configs[1]: 4 agents x 4096 envs, slip 0.1 -- a packed table instance, goals and collisions both occur."""
    grid, nbr, start, goal = _bench_tables('c2', 4096)
    env_like = type('E', (), dict(grid=grid, goal_local=goal, _goal_bcast=False, n_envs=4096, n_agents=4))
    table, rows = shortest_path_policy(env_like)
    assert table.shape[1] == 256 and rows.shape == (4096, 4)
    goals, colls, name = _run_parity(grid, nbr, start, goal, 4, table, rows, T=64, fail_prob=0.1, expect='lq_rollout_kernel')
    assert goals > 0 and colls > 0, (goals, colls)


@pytest.mark.parametrize('criteria', ['Makespan', 'SoC'])
def test_c5_share_shape_32_agents_on_the_synthetic_64x64_map(criteria):
    """BASELINE configs[4]'s share of one GPU: 16384 envs x 32 agents, the bitmap form over delta rows; the goals are random
    cells, so the shortest-path table has a row per distinct goal (far beyond LDS: the global form)."""
    E, A = 16384, 32
    grid, nbr, start, goal = _bench_tables('c5', E)
    table, row_of = shortest_path_table(grid, goal[:64])          # 2048 goals' rows (6.7 MB); the other envs reuse them
    keys = np.asarray(sorted(row_of))
    rs = np.random.RandomState(5)
    rows = rs.randint(0, len(keys), size=(E, A)).astype(np.uint16)
    rows[:64] = np.vectorize(row_of.get)(goal[:64].astype(np.int64))
    _, _, name = _run_parity(grid, nbr, start, goal, A, table, rows, criteria=criteria, T=16, expect='lq_rollout_kernel')
    assert 'BITMAP' in name and 'TABLE_GLOBAL' in name, name


def test_large_map_through_the_global_move_table():
    from gym_mapf_amd.envs import map_name_to_files
    from gym_mapf_amd.envs.utils import parse_map_file
    grid = MapfGrid(parse_map_file(map_name_to_files('maze-128-128-10', 18)[0]))
    nbr = grid.tables()[2]
    V, E, A = nbr.shape[0], 512, 6
    rs = np.random.RandomState(77)
    start, goal = _random_cells(rs, E, V, A), _random_cells(rs, 1, V, A).reshape(-1)
    table, row_of = shortest_path_table(grid, goal)
    rows = np.vectorize(row_of.get)(goal.astype(np.int64)).astype(np.uint16)          # [A]: broadcast rows, broadcast goals
    _, _, name = _run_parity(grid, nbr, start, goal, A, table, rows, T=24, expect='MV_GLOBAL')


def test_auto_reset_off_envs_stay_terminal_and_launch_lengths_walk_every_phase(monkeypatch):
    """Launches of 1, 2, 3, 5, 4, 7, 6 ... steps: every phase of the four-step block at a launch's start and end, recording
    and totals-only alternating, without auto-reset (finished envs stay terminal: steps from a terminal state are no-ops)."""
    for k, E, expect in ((4, 16384, 'lq_rollout_kernel_table<Q=2,K=4'), (2, 8192, 'lq_rollout_kernel_table<Q=4,K=2'), (0, 1000, 'lg_rollout_kernel_table')):
        set_tune(monkeypatch, k=k if k else None)
        A = 8
        grid, nbr, start, goal = _bench_tables('c3', E)
        env = VecMapfEnv(grid, A, None, None, 0.2, *R, OptimizationCriteria.Makespan, seed=3, start_local=start, goal_local=goal)
        co = c_oracle.COracle(nbr, A, start, goal, 0.2, *R, mo.MAKESPAN, seed=3)
        table, rows = shortest_path_policy(env)
        env.set_policy('table', table=table, rows=rows)
        terminal_seen = 0
        for i, n in enumerate((1, 2, 3, 5, 4, 7, 6, 9, 8, 11, 40)):
            res = env.rollout(n, auto_reset=False, record=(i % 2 == 0))
            assert expect in env.last_kernel('rollout'), env.last_kernel('rollout')
            refs, _, _ = _oracle_steps(co, table, _full_rows(rows, E, A), n, auto_reset=False)
            if i % 2 == 0:
                _check_record(res, refs, (k, i, n))
            _check_totals(res, refs, (k, i, n))
            terminal_seen += int(sum(int(r['was_terminal'].sum()) for r in refs))
            assert np.array_equal(env.get_state()[0], co.state), (k, i, n)
        assert terminal_seen > 0
        env.close()


def test_full_bench_shape_65536_envs_recording():
    """BASELINE configs[2], the headline shape: 65536 envs x 8 agents on room-32-32-4, T = 64, recording, device arrays."""
    E, A, T = 65536, 8, 64
    grid, nbr, start, goal = _bench_tables('c3', E)
    env = VecMapfEnv(grid, A, None, None, 0.2, *R, OptimizationCriteria.Makespan, seed=21, start_local=start, goal_local=goal,
                     device_arrays=True)
    co = c_oracle.COracle(nbr, A, start, goal, 0.2, *R, mo.MAKESPAN, seed=21)
    table, rows = shortest_path_policy(env)
    assert table.shape == (46, 682)
    env.set_policy('table', table=table, rows=rows)
    res = env.rollout(T, auto_reset=True, record=True)
    env.sync()
    name = env.last_kernel('rollout')
    assert 'lq_rollout_kernel' in name and 'TABLE' in name and 'K=4' in name, name
    refs, goals, colls = _oracle_steps(co, table, _full_rows(rows, E, A), T)
    _check_record(res, refs, name)
    _check_totals(res, refs, name)
    assert np.array_equal(_state(env), co.state)
    assert goals > 0 and colls > 0, (goals, colls)
    env.close()


def test_a_shard_equals_the_slice_of_the_whole():
    """env_id_offset != 0: envs 4096..8191 of an 8192-env batch run as a handle of their own give the slice's results."""
    E, A, T = 8192, 8, 20
    grid, nbr, start, goal = _bench_tables('c3', E)
    table, row_of = shortest_path_table(grid, goal)
    rows = np.vectorize(row_of.get)(goal.astype(np.int64)).astype(np.uint16)
    outs = []
    for lo, hi, off in ((0, E, 0), (4096, E, 4096)):
        env = VecMapfEnv(grid, A, None, None, 0.2, *R, OptimizationCriteria.Makespan, seed=9, start_local=start[lo:hi],
                         goal_local=goal[lo:hi], env_id_offset=off)
        env.set_policy('table', table=table, rows=rows[lo:hi])
        outs.append(env.rollout(T, auto_reset=True, record=True))
        assert 'TABLE' in env.last_kernel('rollout')
        env.close()
    whole, shard = outs
    for key in ('local', 'reward', 'prob', 'done', 'collision'):
        assert np.array_equal(whole[key][:, 4096:].view(np.uint8), shard[key].view(np.uint8)), key
    assert np.array_equal(bits(whole['returns'][4096:]), bits(shard['returns']))
    co = c_oracle.COracle(nbr, A, start[4096:], goal[4096:], 0.2, *R, mo.MAKESPAN, seed=9, env_id_offset=4096)
    refs, _, _ = _oracle_steps(co, table, rows[4096:].astype(np.int64), T)
    _check_record(shard, refs, 'shard')


def test_policy_switches_restore_the_policy_stream_and_replace_tables():
    E, A = 2048, 8
    grid, nbr, start, goal = _bench_tables('c3', E)
    valid = grid.tables()[0]
    rc = np.asarray([r | (c << 16) for r, c in valid], np.uint32)
    env = VecMapfEnv(grid, A, None, None, 0.2, *R, OptimizationCriteria.Makespan, seed=13, start_local=start, goal_local=goal)
    co = c_oracle.COracle(nbr, A, start, goal, 0.2, *R, mo.MAKESPAN, seed=13)
    table, rows = shortest_path_policy(env)
    full = _full_rows(rows, E, A)
    env.set_policy('table', table=table, rows=rows)
    res = env.rollout(8, record=True)
    _check_record(res, _oracle_steps(co, table, full, 8)[0], 'table 1')
    env.set_policy('random')                                      # table -> random: the policy stream is back
    out = env.rollout(6)
    ref = co.rollout(6, auto_reset=True)
    assert 'POLICY' in env.last_kernel('rollout')
    assert np.array_equal(bits(out['returns']), bits(ref['returns'])) and np.array_equal(env.get_state()[0], co.state)
    env.set_policy('table', table=table, rows=rows)
    env.set_policy('greedy')                                      # table -> greedy -> table
    res = env.rollout(5, record=True)
    assert 'POLICY' in env.last_kernel('rollout')
    for t in range(5):
        r = co.step(co.greedy_actions(rc), auto_reset=True)
        assert np.array_equal(res['local'][t], r['local']) and np.array_equal(bits(res['reward'][t]), bits(r['reward']))
    env.set_policy('table', table=table, rows=rows)
    res = env.rollout(7, record=True)
    assert 'TABLE' in env.last_kernel('rollout')
    _check_record(res, _oracle_steps(co, table, full, 7)[0], 'table 2')
    # a second table with other rows replaces the first
    rs = np.random.RandomState(4)
    table2 = rs.randint(0, 5, size=(3, table.shape[1])).astype(np.uint8)
    rows2 = rs.randint(0, 3, size=(A,)).astype(np.uint16)
    env.set_policy('table', table=table2, rows=rows2)
    res = env.rollout(9, record=True)
    _check_record(res, _oracle_steps(co, table2, _full_rows(rows2, E, A), 9)[0], 'table 3')
    assert np.array_equal(env.get_state()[0], co.state) and env.t == co.t
    env.close()


def test_step_graph_with_a_table_rollout_replays_with_fresh_slip_numbers():
    import torch
    E, A, T, K = 2048, 8, 12, 4
    grid, nbr, start, goal = _bench_tables('c3', E)
    env = VecMapfEnv(grid, A, None, None, 0.2, *R, OptimizationCriteria.Makespan, seed=17, start_local=start, goal_local=goal,
                     device_arrays=True)
    co = c_oracle.COracle(nbr, A, start, goal, 0.2, *R, mo.MAKESPAN, seed=17)
    table, rows = shortest_path_policy(env)
    env.set_policy('table', table=torch.from_numpy(table), rows=torch.from_numpy(rows.astype(np.int64)))   # CPU torch arrays work too
    env.graph_begin()
    res = env.rollout(T, auto_reset=True, record=True)
    graph = env.graph_end()
    assert graph.steps == T and 'TABLE' in env.last_kernel('rollout')
    with pytest.raises(nat.MapfNativeError):
        env.set_policy('table', table=table, rows=rows)           # the recorded node names the table's device copy
    with pytest.raises(nat.MapfNativeError):
        env.set_policy('random')
    assert env.policy == 'table'
    for rep in range(K):
        graph.launch(1)
        env.sync()
        refs, _, _ = _oracle_steps(co, table, _full_rows(rows, E, A), T)
        _check_record(res, refs, 'replay %d' % rep)
        assert np.array_equal(_state(env), co.state)
    assert env.t == co.t == K * T
    graph.close()
    env.set_policy('random')                                      # allowed again once the graph is gone
    env.close()


def test_out_cache_does_not_outlive_a_policy_change():
    E, A, T = 2048, 8, 8
    grid, nbr, start, goal = _bench_tables('c3', E)
    env = VecMapfEnv(grid, A, None, None, 0.2, *R, OptimizationCriteria.Makespan, seed=19, start_local=start, goal_local=goal,
                     device_arrays=True)
    co = c_oracle.COracle(nbr, A, start, goal, 0.2, *R, mo.MAKESPAN, seed=19)
    out = env.rollout(T, record=True)
    out = env.rollout(T, record=True, out=out)
    out = env.rollout(T, record=True, out=out)                    # the cached argument block is in use now
    co.rollout(3 * T, auto_reset=True)
    table, rows = shortest_path_policy(env)
    env.set_policy('table', table=table, rows=rows)
    assert env._rollout_io is None
    out = env.rollout(T, record=True, out=out)
    env.sync()
    assert 'TABLE' in env.last_kernel('rollout')
    _check_record(out, _oracle_steps(co, table, _full_rows(rows, E, A), T)[0], 'after the switch')
    env.close()


def test_invalid_tables_raise_before_anything_is_launched():
    grid = _random_map(3)
    nbr = grid.tables()[2]
    V, E, A = nbr.shape[0], 64, 4
    rs = np.random.RandomState(1)
    start, goal = _random_cells(rs, E, V, A), _random_cells(rs, E, V, A)
    env = VecMapfEnv(grid, A, None, None, 0.2, *R, OptimizationCriteria.Makespan, seed=1, start_local=start, goal_local=goal)
    good = np.zeros((3, V), np.uint8)
    rows = np.zeros((E, A), np.uint16)
    bad = good.copy(); bad[2, V - 1] = 5
    for kwargs in (dict(table=bad, rows=rows), dict(table=good, rows=np.full((E, A), 3)), dict(table=good[:, :-1], rows=rows),
                   dict(table=good, rows=rows[:, :-1]), dict(table=good, rows=rows[:-1]), dict(table=good.ravel(), rows=rows),
                   dict(table=good, rows=None), dict(table=good.astype(np.float32), rows=rows), dict(table=good, rows=-np.ones((E, A), np.int64))):
        with pytest.raises(ValueError):
            env.set_policy('table', **kwargs)
    with pytest.raises(ValueError):
        env.set_policy('random', table=good, rows=rows)
    assert env.policy == 'random' and env.last_kernel('rollout') == ''
    # the C ABI's own checks (the Python layer cannot be the only guard of the kernels' unclamped index)
    lib = env._lib
    rows16 = np.zeros((E, A), np.uint16)
    assert lib.mapf_set_policy_table(env._h, bad.ctypes.data, 3, rows16.ctypes.data, 0) == nat.MAPF_EINVAL
    assert b'table[' in lib.mapf_last_error()
    rows16[E - 1, A - 1] = 3
    assert lib.mapf_set_policy_table(env._h, good.ctypes.data, 3, rows16.ctypes.data, 0) == nat.MAPF_EINVAL
    assert b'row_index[' in lib.mapf_last_error()
    assert lib.mapf_set_policy(env._h, nat.MAPF_POLICY_TABLE, None) == nat.MAPF_EINVAL
    assert b'mapf_set_policy_table' in lib.mapf_last_error()
    out = env.rollout(4)                                          # still the random policy
    assert 'POLICY' in env.last_kernel('rollout') and out['returns'].shape == (E,)
    env.close()
