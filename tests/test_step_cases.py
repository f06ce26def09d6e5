"""The single step's case table (tests/step_cases.py), checked without a GPU: every case takes the packed family and plans exactly the
instance it declares, the table names all 84 kernels of the launcher, the chunk-walk cases have the geometry they claim, and the C
oracle's output of every pass contains what makes a wrong kernel show -- tests/test_gpu_step_forms.py then compares the kernels with it."""
import ctypes

import numpy as np
import pytest

import step_cases as sc
from host_shim import move_tables, slip_rows
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import KERNEL_NAME_BYTES, LQ_STEP_LAUNCHES, PACKED, lq_step_fixture, routed_step

SHAPES = list({(c.key, c.E): c for c in sc.CASES}.values())               # (the three grids of a chunk walk share their runs)


def _variant(scen, term):
    return '%s %s' % ('SCEN' if scen else 'ROWS', 'TERMINAL' if term else 'NO_TERMINAL')


def _planned(shim, n_cu, case, scen, term, grid=True):  # noqa: F811
    """the step of a handle through route_step: ((Q, K, form), grid, n_chunks, name) -- the packed family or an AssertionError"""
    V = the_cells()
    tune = case.tune_text(scen, grid).encode() or None
    family, out, name = routed_step(shim, V, case.A, case.E, 0, 0, tune, delta=1, n_cu=n_cu, scen=int(scen), term=int(term))
    assert family == PACKED, (case.id, family)
    again = ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    assert shim.shim_lq_step_name(V, case.A, case.E, 1, n_cu, tune, int(scen), int(term), again) == 1 and again.value.decode() == name, case.id
    return (out[1], out[0], out[2]), out[4], out[5], name


def the_cells():
    return sc.the_map()[1].shape[0]


def test_the_instance_cases_are_the_recorded_launches(shim):  # noqa: F811
    """one instance case per entry of the fixture, in its order, at its tune and at its batch or twice that; delta rows apply on the map"""
    assert [c.key for c in sc.INSTANCE_CASES] == list(LQ_STEP_LAUNCHES) and len(sc.INSTANCE_CASES) == 21
    for c in sc.INSTANCE_CASES:
        form, K, Q, E, tune = LQ_STEP_LAUNCHES[c.key]
        assert (c.form, c.K, c.Q, c.tune) == (form, K, Q, tune) and c.E in (E, 2 * E) and 64 <= c.E <= 1024, c.id
    assert the_cells() == 341 == lq_step_fixture()['launches']['Plain-K4-Q1']['V']
    assert move_tables(shim, sc.the_map()[1], 0.2)[2] is not None
    assert len({c.id for c in sc.CASES}) == len(sc.CASES)
    for c in sc.CASES:
        assert all(s in sc.SEEDS_SEARCHED for s in c.seeds), c.id


def test_every_case_plans_its_instance_and_the_table_names_all_84_kernels(shim):  # noqa: F811
    """route_step, asked at the fixture's CU count as the dispatcher asks it: the packed family and exactly the case's (Q, K, form),
    with and without the scenario table, terminal test or not; the names are the fixture's in full (a name says nothing of the batch
    or the grid), and over the table they are all 84"""
    recorded = lq_step_fixture()
    names = set()
    for case in sc.CASES:
        for scen in (True, False):
            for term in (True, False):
                instance, grid, n_chunks, name = _planned(shim, recorded['n_cu'], case, scen, term)
                assert instance == (case.Q, case.K, case.form), (case.id, instance)
                assert name == recorded['launches'][case.key]['names'][_variant(scen, term)], (case.id, name)
                names.add(name)
    assert len(names) == 84 == sum(len(launch['names']) for launch in recorded['launches'].values())
    # ... and the schedule launches both kinds of every handle several times
    plan = sc.step_plan()
    assert len(plan) == sc.N_STEPS == 12 and sum(may for _, may, _ in plan) == 4 and sum(1 for _, _, set_before in plan if set_before) == 1
    assert [may for _, may, _ in plan] == [False, False, False, False, True, True, False, True, False, False, True, False]


@pytest.mark.parametrize('case', sc.WALK_CASES, ids=lambda c: c.id)
def test_chunk_walk_geometry(case, shim):  # noqa: F811
    """seven chunks; step_grid blocks under the key, seven without it (one chunk per block: what the suite ran before the key)"""
    n_cu = lq_step_fixture()['n_cu']
    for scen in (True, False):
        instance, grid, n_chunks, _ = _planned(shim, n_cu, case, scen, True)
        assert (n_chunks, grid) == (sc.WALK_CHUNKS, case.step_grid), (case.id, grid, n_chunks)
        walked = [len(range(b, n_chunks, grid)) for b in range(grid)]
        assert tuple(walked) == sc.WALK_PATTERNS[case.step_grid]
        instance_free, grid_free, n_chunks_free, _ = _planned(shim, n_cu, case, scen, True, grid=False)
        assert (instance_free, grid_free, n_chunks_free) == (instance, sc.WALK_CHUNKS, sc.WALK_CHUNKS), case.id


def test_step_grid_only_lowers_the_grid_of_the_resident_forms(shim):  # noqa: F811
    """the key never raises a grid, leaves the plain step alone and is refused when malformed"""
    out, V = (ctypes.c_uint64 * 8)(), the_cells()
    for case in sc.CASES:
        assert shim.shim_plan_step(V, case.A, case.E, 1, 256, case.tune_text(True, grid=False).encode() or None, out) == 1
        free = tuple(out)
        for n in (1, 5, 4096):
            tune = ','.join(filter(None, (case.tune_text(True, grid=False), 'step_grid=%d' % n))).encode()
            assert shim.shim_plan_step(V, case.A, case.E, 1, 256, tune, out) == 1
            want = min(n, free[4]) if case.form != 0 else free[4]
            assert tuple(out) == free[:4] + (want,) + free[5:], (case.id, n, tuple(out), free)
    assert shim.shim_plan_step(V, 8, 1024, 1, 256, b'step_grid=x', out) == -1
    assert shim.shim_plan_step(V, 8, 1024, 1, 256, b'step_grid=', out) == -1


@pytest.fixture(scope='module')
def slip_thresholds(shim):  # noqa: F811
    """per slip rate: (the top 16 bits of every threshold a list compares against, the thresholds as 53-bit integers)"""
    found = {}
    for p in sc.PASSES:
        rows = slip_rows(shim, p.fail_prob)[0]
        th16 = sorted({int(row['th'][k]) for row in rows for k in range(int(row['n']) - 1)})
        th53 = sc.exact_thresholds(row['cum'][k] for row in rows for k in range(int(row['n']) - 1))
        assert th53 == sorted({int(row['thr'][k]) for row in rows for k in range(int(row['n']) - 1)})   # (what the host built: ceil(cum * 2^53))
        assert len(th16) == 2 and sorted(t >> 37 for t in th53) == th16, (th16, th53)
        found[p.name] = (th16, th53)
    return found


_TIES = {}               # {(case's key, E, pass): (ties, not passed, passed)}: computed once, whichever test asks first


def ties_of(case, p, slip_thresholds):
    at = (case.key, case.E, p.name)
    if at not in _TIES:
        th16, th53 = slip_thresholds[p.name]
        run = case.run(p)
        _TIES[at] = (sc.slip_ties(run, th16),) + sc.tie_outcomes(run, th53)
    return _TIES[at]


@pytest.mark.parametrize('case', SHAPES, ids=lambda c: c.key + '-E%d' % c.E)
def test_the_oracles_output_can_show_an_error(case, slip_thresholds):
    """per pass (the two handles of a pass share the oracle's run): goal ends, collision ends, vertex collisions on the shared goal;
    terminal envs on at least two of the steps planned with the terminal test and on none planned NO_TERMINAL; three counts of
    A - stayed under SoC; MIN_TIES slip ties among the non-terminal envs"""
    plan = sc.step_plan()
    for p in sc.PASSES:
        run = case.run(p)
        tag = (case.id, p.name)
        found = sc.outcomes(run)
        assert found['goals'] > 0 and found['collisions'] > 0 and found['on_shared_goal'] > 0, (tag, found)
        with_terminal = [n > 0 for n in found['terminal']]
        assert sum(has and may for has, (_, may, _) in zip(with_terminal, plan)) >= 2, (tag, found['terminal'])
        assert not any(has and not may for has, (_, may, _) in zip(with_terminal, plan)), (tag, found['terminal'])
        assert not p.soc or len(sc.soc_counts(run)) >= 3, (tag, sorted(sc.soc_counts(run)))
        ties, below, passed = ties_of(case, p, slip_thresholds)
        assert ties >= sc.MIN_TIES and below + passed == ties, (tag, ties, below, passed)
        for (state, t), s in zip(run.after, range(sc.N_STEPS)):
            assert t == s + 1
        assert sorted(run.set_states) == [7] and np.array_equal(run.set_states[7][::4], run.goal[::4])


def test_both_refinement_outcomes_occur_in_every_form(slip_thresholds):
    """over a StepForm's cases the 53-bit compare resolves at least one tie as 'threshold not passed' and one as 'passed' (a kernel
    that drops the refinement, or settles it the other way, then moves an agent of a case of that form)"""
    totals = {}
    for case in SHAPES:
        for p in sc.PASSES:
            _, below, passed = ties_of(case, p, slip_thresholds)
            totals[case.form] = tuple(np.add(totals.get(case.form, (0, 0)), (below, passed)).tolist())
    assert sorted(totals) == [0, 1, 2, 3]
    for form, (below, passed) in totals.items():
        assert below > 0 and passed > 0, (sc.STEP_FORMS[form], below, passed)


def test_graph_run_is_fourteen_oracle_steps():
    run = sc.GraphRun()
    assert len(run.refs) == 14 and run.after[-1][1] == 14 and sum(int(ref['done'].sum()) for ref in run.refs) > 0
