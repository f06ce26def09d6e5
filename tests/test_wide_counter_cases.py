"""The wide-counter case tables (tests/wide_counter_cases.py), checked without a GPU: the C oracle, the pure-Python oracle and
oracle/philox.py agree on every window (the reference is sound where no kernel has been compared with it before), every narrowing
of a 64-bit quantity to 32 bits changes the oracle's own output at the first step it applies to (the inputs can show the error),
and the tables are a ledger: every form once, at a batch and under MAPF_TUNE keys with which the planner chooses it --
tests/test_gpu_wide_counters.py then compares the kernels with the same runs."""
import ctypes
import re

import numpy as np
import pytest

import c_oracle
import mapf_oracle as mo
import philox
import wide_counter_cases as wc
from host_shim import move_tables
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from parity_checks import bits
from plan_sweeps import KERNEL_NAME_BYTES, N_CU
from totals_cases import _random_map_tables


@pytest.mark.parametrize('n_agents', [8, 5])
@pytest.mark.parametrize('X', wc.CROSSINGS, ids=lambda X: '2^%d' % (X.bit_length() - 1))
def test_the_three_oracles_agree_on_every_window(X, n_agents):
    """64 envs whose ids carry into their high word at env 37, twelve steps from X - 6, every seed: the C oracle on its own stream ==
    the C oracle with uniforms injected from philox.slip_uniform (the scalar definition) and actions from philox.random_actions_np
    == the pure-Python oracle with the same uniforms; the vectorised philox functions == the scalar ones; and the C oracle's own
    policy stream (oracle_rollout without actions) == the sum over the steps above."""
    A, E, T = n_agents, 64, 12
    grid, nbr, rc, start, goal, near = _random_map_tables(A, E, 700)
    lines = [''.join('@' if f else '.' for f in row) for row in grid.obstacles.tolist()]
    assert np.array_equal(nbr, np.asarray(mo.neighbour_table(lines), np.uint16))
    cells = mo.free_cells_column_major(lines)[1]
    ids = [wc.OFFSET + e for e in range(E)]
    assert ids[36] >> 32 == 0 and ids[37] >> 32 == 1
    for seed in wc.SEEDS:
        own = c_oracle.COracle(nbr, A, start, goal, wc.SLIP, *wc.REWARDS, mo.MAKESPAN, seed=seed, env_id_offset=wc.OFFSET)
        fed = c_oracle.COracle(nbr, A, start, goal, wc.SLIP, *wc.REWARDS, mo.MAKESPAN)          # (seed, offset and t unused: uniforms are given)
        whole = c_oracle.COracle(nbr, A, start, goal, wc.SLIP, *wc.REWARDS, mo.MAKESPAN, seed=seed, env_id_offset=wc.OFFSET)
        envs = [mo.OracleEnv(lines, A, [cells[c] for c in start[e]], [cells[c] for c in goal[e]], wc.SLIP, *wc.REWARDS, mo.MAKESPAN) for e in range(E)]
        own.t = whole.t = X - 6
        ret, done_total = np.zeros(E), 0
        for t in range(X - 6, X + 6):
            acts = philox.random_actions_np(seed, ids, t, A)
            assert acts.tolist() == [[philox.random_action(seed, i, t, a) for a in range(A)] for i in ids], (seed, t)
            u = np.asarray([[philox.slip_uniform(seed, i, t, a) for a in range(A)] for i in ids])
            assert np.array_equal(bits(u), bits(philox.slip_uniforms_np(seed, ids, t, A))), (seed, t)
            a, b = own.step(acts, auto_reset=True), fed.step(acts, uniforms=u, auto_reset=True)
            for name in a:
                assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), (seed, t, name)
            for e, env in enumerate(envs):
                local, reward, done, collision, prob, was_terminal = env.step(acts[e].tolist(), u[e].tolist())
                assert list(local) == a['local'][e].tolist() and float(reward) == a['reward'][e] and float(prob) == a['prob'][e], (seed, t, e)
                assert (int(done), int(collision), int(was_terminal)) == (a['done'][e], a['collision'][e], a['was_terminal'][e]), (seed, t, e)
                if done:
                    env.reset()
            ret = ret + a['reward']
            done_total += int(a['done'].sum())
        assert np.array_equal(own.state, fed.state) and done_total > 0
        total = whole.rollout(T, auto_reset=True)
        assert np.array_equal(bits(total['returns']), bits(ret)) and np.array_equal(whole.state, own.state), seed


def _windows(case, X):
    if case in wc.STEP_CASES:
        return [wc.step_window(X)]
    if case in wc.GRAPH_CASES:
        return [wc.graph_window(X)]
    return list(wc.rollout_windows(X, case.table))


ALL_CASES = wc.ROLLOUT_CASES + wc.STEP_CASES + wc.GRAPH_CASES


@pytest.mark.parametrize('case', ALL_CASES, ids=lambda c: ('rollout-' if c in wc.ROLLOUT_CASES else 'step-' if c in wc.STEP_CASES else '') + c.id)
def test_every_narrowing_shows_in_the_oracles_output_of_every_window(case):
    """No exemptions: a case whose inputs could not show a narrowing is repaired by its map seed (Case.map_seed).  A model that is
    the identity by the streams' definition does not apply (wide_counter_cases.narrowings says which and why); over a case's windows
    every model that can apply to its kind of launch does, and every case sees all three seeds."""
    crossings = wc.GRAPH_CROSSINGS if case in wc.GRAPH_CASES else wc.CROSSINGS
    seen, seeds, episodes = set(), set(), 0
    for X in crossings:
        seeds.add(case.seed(X))
        for window in _windows(case, X):
            run = wc.window_run(case, X, window.name)
            assert run.t0 == window.t0 and len(run.refs) == window.n_steps
            for name, (s, changed) in wc.narrowings(run).items():
                assert changed > 0, (case.id, X, window.name, name, s)
                assert s == (X - window.t0 if 'X' in name or 'quad' in name else 0), (name, s)
                seen.add(name)
            episodes += sum(int(ref['done'].sum()) for ref in run.refs)
            assert not any(ref['was_terminal'].any() for ref in run.refs)       # (auto-reset on, no terminal start rows)
    want = set(wc.NARROWINGS)
    if case not in wc.ROLLOUT_CASES or case.table:
        want -= {'policy at t - X from step X on', 'policy key (seed_lo + 1, seed_hi)'}
    if (1 << 49) not in crossings:
        want -= {'h hi unmasked in the quad field'}
    assert seen == want, (case.id, sorted(want - seen), sorted(seen - want))
    assert len(seeds) == (3 if len(crossings) >= 3 else len(crossings)) and episodes > 0, (case.id, seeds, episodes)


def test_every_fill_random_actions_window_shows_a_narrowed_policy_counter():
    """fill_random_actions(X - 3, 9): the rows from step X on differ from the rows a counter without its carry would give."""
    for X in wc.FILL_CROSSINGS:
        for k, (A, E) in enumerate(wc.FILL_SHAPES):
            seed, ids = wc.seed_of(k, X), wc.OFFSET + np.arange(E, dtype=np.uint64)
            for t in range(X, X + 6):
                right = philox.random_actions_np(seed, ids, t, A)
                assert not np.array_equal(right, philox.random_actions_np(seed, ids, t - X, A)), (X, A, t)
                assert not np.array_equal(right[37:], philox.random_actions_np(seed, ids & np.uint64(wc.M32), t, A)[37:]), (X, A, t)
                if (seed + 1) & wc.M32 == 0:
                    wrong_key = (seed & ~wc.M32 & wc.M64) | ((seed + 1) & wc.M32)
                    assert not np.array_equal(right, philox.random_actions_np((wrong_key - 1) & wc.M64, ids, t, A)), (X, A, t)


# ----------------------------------------------------------------------- the ledger
def test_the_case_tables_name_every_form_once_and_follow_the_goal_tests_list():
    for table in (wc.ROLLOUT_CASES, wc.STEP_CASES, wc.GRAPH_CASES):
        assert len({c.id for c in table}) == len(table) and len({c.layout for c in table}) == len(table)
        assert [c.index for c in table] == list(range(len(table)))
        assert all(c.E <= 16512 for c in table)
    rows = {(A, E, layout, tuple(sorted(tune.items()))) for A, E, layout, tune in wc.GOAL_ROWS}
    mine = {(c.A, c.E, c.layout, tuple(sorted(c.tune.items()))) for c in wc.ROLLOUT_CASES if not c.table}
    assert mine <= rows, sorted(mine - rows)
    assert {(A, E) for A, E, _, _ in rows - mine} == wc.GOAL_ROWS_LEFT_OUT
    names = ' '.join(c.layout for c in wc.ROLLOUT_CASES)
    for part in ('K=2', 'K=4', 'K=8', 'Q=16', ',COMPACT', ',BITMAP> block=512', ',BITMAP> block=1024', ',BITMAP5> block=512', ',BITMAP5> block=1024',
                 ',BITMAPD> block=512', ',BITMAPD> block=1024', 'MV_LDS', 'MV_GLOBAL', 'RAGGED', 'rollout_kernel<A=6>', 'lq_rollout_kernel_table'):
        assert part in names, part
    for A in (8, 32):
        assert {re.search(r'K=(\d)', c.layout).group(1) for c in wc.ROLLOUT_CASES if c.A == A and 'lq_rollout_kernel<' in c.layout} == {'2', '4', '8'}
    for case in wc.STEP_CASES:
        first, later = wc.step_name(case, 0), wc.step_name(case, 1)
        assert first == case.layout and ('NO_TERMINAL' in later) == case.layout.startswith('lq_step_kernel'), (first, later)
        assert later.replace(',NO_TERMINAL', '') == first
    assert wc.step_name(wc.STEP_CASES[0], 1) == 'lq_step_kernel<Q=2,K=4,SCEN,NO_TERMINAL> block='
    assert wc.step_name(wc.STEP_CASES[3], 1) == 'lq_step_kernel<Q=2,K=8,NO_TERMINAL,BIG> block=1024'


def _shape(case):
    m = re.search(r'<Q=(\d+),K=(\d+)', case.layout)
    return (int(m.group(2)), int(m.group(1))) if m else None


@pytest.mark.parametrize('case', wc.ROLLOUT_CASES, ids=lambda c: c.id)
def test_rollout_case_plans_the_form_it_names(case, shim):  # noqa: F811
    from gym_mapf_amd import _native
    lib = _native.load()
    grid, nbr, start, goal, policy = wc.tables_of(case)
    V, tune = nbr.shape[0], case.tune_text().encode() or None
    delta = int(move_tables(shim, nbr, wc.SLIP)[2] is not None)
    out = (ctypes.c_uint64 * 9)()
    launches = [(n, 0 if w.mode == 'policy' else 1) for w in wc.rollout_windows(wc.CROSSINGS[0], case.table) for n in w.lengths]
    assert launches == ([(5, 1), (7, 1)] if case.table else [(5, 1), (7, 1), (12, 0)])
    for T, streamed in launches:
        rc = lib.mapf_debug_rollout_plan(V, case.A, case.E, T, streamed, delta, N_CU, tune, out)       # (-1: a key the planner does not know)
        if case.table:
            assert shim.shim_plan_rollout_table(V, case.A, case.E, T, delta, policy[0].size, N_CU, tune, 0, out, None) == 1
            assert (out[0], out[1]) == _shape(case) and case.E % (out[3] // out[1]) == 0
        elif case.form is not None:
            assert rc == 1 and (out[0], out[1]) == _shape(case) and out[2] == wc.FORMS.index(case.form), (T, streamed, rc, tuple(out))
            assert case.E % (out[3] // out[1]) == 0 and out[5] <= 160 * 1024
            if '>' in case.layout:                                    # a whole name: its tags are the form's, its block the plan's
                compact, tag = wc.FORM_NAME[case.form]
                assert (',COMPACT' in case.layout) == bool(compact) and (tag + '> block=') in case.layout
                block = case.layout.split('block=')[1]
                assert not (block and streamed) or out[3] == int(block), (T, tuple(out))
        else:
            assert rc == 0, (T, streamed, rc)
            if case.kernel == 'auto':
                plan, name = (ctypes.c_uint64 * 7)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
                assert shim.shim_plan_rollout_lg(V, case.A, case.E, 1, 0 if streamed else 1, tune, plan, name) == 1
                assert name.value.decode().startswith(case.layout), (name.value, case.layout)
    assert case.kernel == 'auto' or (case.layout.startswith('rollout_kernel<A=%d>' % case.A) and case.A <= 16)


@pytest.mark.parametrize('case', wc.STEP_CASES + wc.GRAPH_CASES, ids=lambda c: c.id)
def test_step_case_plans_the_form_it_names(case, shim):  # noqa: F811
    grid, nbr, start, goal, _ = wc.tables_of(case)
    V, tune = nbr.shape[0], case.tune_text().encode() or None
    delta = int(move_tables(shim, nbr, wc.SLIP)[2] is not None)
    out = (ctypes.c_uint64 * 8)()
    rc = shim.shim_plan_step(V, case.A, case.E, delta, N_CU, tune, out)
    if case.kernel == 'thread_per_env':
        assert case.layout.startswith('step_kernel<A=%d,' % case.A) and case.A <= 16
    elif case.form is not None:
        assert rc == 1 and (out[0], out[1]) == _shape(case) and out[2] == case.form, (rc, tuple(out))
        assert (',BIG>' in case.layout) == (case.form == 1) and (',DELTA' in case.layout) == (case.form >= 2) and (',BITMAP>' in case.layout) == (case.form == 3)
        block = case.layout.split('block=')[1] if 'block=' in case.layout else ''
        assert not block or out[3] == int(block)
        scen, rows = np.zeros(case.E, np.uint8), np.zeros(256 * 2 * case.A, np.uint16)
        n = shim.shim_scen_table(start.ctypes.data, 0, goal.ctypes.data, 0, case.E, case.A, scen.ctypes.data, rows.ctypes.data)
        assert n == (0 if case.scen is None else 5), n
        assert (',SCEN' in case.layout) == (case.scen is True) and (case.scen is not False or case.tune.get('scen_table') == '0')
        # ... and step_name's prefixes are prefixes of the name the launcher notes for that plan (the graph cases name the first call only)
        name = ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
        for call in (0, 1) if case in wc.STEP_CASES else (0,):
            assert shim.shim_lq_step_name(V, case.A, case.E, delta, N_CU, tune, int(case.scen is True), int(call == 0), name) == 1
            assert name.value.decode().startswith(wc.step_name(case, call)), (call, name.value, wc.step_name(case, call))
    else:
        assert rc == 0, (rc, tuple(out))
        plan, name = (ctypes.c_uint64 * 4)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
        assert shim.shim_plan_step_lg(case.A, case.E, 0, plan, name) == 1
        assert name.value.decode().startswith(case.layout), (name.value, case.layout)
