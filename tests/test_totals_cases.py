"""The totals-only sweep's case table (tests/totals_cases.py), checked without a GPU: it covers every packed rollout instance the
launcher holds (the ledger), every case plans the instance it declares on both map families (reachability), and the C oracle's
output of every pass contains what makes a wrong kernel show -- tests/test_gpu_totals.py then compares the kernels with it."""
import ctypes

import numpy as np
import pytest

import totals_cases as tc
from host_shim import move_tables, slip_rows
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from parity_checks import bits
from plan_sweeps import KERNEL_NAME_BYTES

T_VALUES = sorted(set(tc.LENGTHS + tc.LENGTHS_CHAIN + (tc.OVERWRITE_STEPS, tc.RECORD_STEPS)))


def test_the_case_table_is_the_ledger_of_packed_totals_instances(shim):  # noqa: F811
    """the (K, Q, form) the launcher holds == the ones the table declares, each once: an instance added to mapf_layout.hpp
    without a totals case fails here.  The six passes of a case name six different kernels: 120 names for the 20 entries."""
    held = {(K, Q, form) for K in (2, 4, 8) for Q in (1, 2, 4, 8, 16) for form in range(len(tc.FORMS))
            if shim.shim_rollout_instance_exists(K, Q, form, 0) == 1}
    declared = [(c.K, c.Q, tc.FORMS.index(c.form)) for c in tc.PACKED_CASES]
    assert len(set(declared)) == len(declared), 'a (K, Q, form) is declared twice'
    assert set(declared) == held, (sorted(held - set(declared)), sorted(set(declared) - held))
    names = {c.kernel_name(p) for c in tc.PACKED_CASES for p in tc.passes_of(c)}
    assert len(names) == 6 * len(held) == 120, len(names)
    assert len({c.id for c in tc.CASES}) == len(tc.CASES)
    assert all(c.agent_steps >= 500000 for c in tc.PACKED_CASES)
    assert sorted(c.id for c in tc.CASES if c.tie_exempt) == ['lg-A3-E257', 'lg-A8-E300']


@pytest.fixture(scope='module')
def thresholds16(shim):  # noqa: F811
    """the top 16 bits of every threshold a slip rate's lists compare against (a list's last threshold is never compared)"""
    found = {}
    for fail_prob in set(tc.SLIP.values()):
        rows = slip_rows(shim, fail_prob)[0]
        found[fail_prob] = sorted({int(row['th'][k]) for row in rows for k in range(int(row['n']) - 1)})
        assert len(found[fail_prob]) == 2, found
    return found


@pytest.mark.parametrize('case', tc.CASES, ids=lambda c: c.id)
def test_case_reaches_its_kernel_and_its_inputs_can_show_an_error(case, shim, thresholds16):  # noqa: F811
    from gym_mapf_amd import _native
    lib = _native.load()
    tables = tc.Tables(case)
    tune = case.tune_text().encode() or None
    # ---- reachability: the planner, asked as the launcher asks it, plans the declared instance (or declines, for the other families)
    out = (ctypes.c_uint64 * 6)()
    for family in ('R', 'G') if case.packed else ('R',):
        nbr = getattr(tables, family)[1]
        V = nbr.shape[0]
        delta = int(move_tables(shim, nbr, 0.2)[2] is not None)
        assert family != 'R' or delta == 1                           # (delta rows apply on the random maps)
        for streamed in (1, 0):
            for T in T_VALUES:
                rc = lib.mapf_debug_rollout_plan(V, case.A, case.E, T, streamed, delta, 256, tune, out)
                if case.packed:
                    assert rc == 1 and tuple(out)[:3] == (case.K, case.Q, tc.FORMS.index(case.form)), (family, V, streamed, T, rc, tuple(out))
                    assert case.E % (out[3] // case.Q) == 0 and out[5] <= 160 * 1024
                else:
                    assert rc == 0, (family, V, streamed, T, rc, tuple(out))
            if case.lg:
                plan, name = (ctypes.c_uint64 * 7)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
                assert shim.shim_plan_rollout_lg(V, case.A, case.E, 0, 0 if streamed else 1, tune, plan, name) == 1
                want = 'lg_rollout_kernel<L=%d,%s,%s,TOTALS,%s,' % (case.lg + ('STREAM' if streamed else 'POLICY',))
                assert name.value.decode().startswith(want), (name.value, want)
    # ---- the inputs can show an error: on the oracle's output alone
    many_episodes = goal_episodes = clash_episodes = r_collisions = ties = 0
    for p in tc.passes_of(case):
        run = tc.PassRun(case, p, tables)
        tag = (case.id, p.tag)
        assert case.kernel_name(p).count('TOTALS') == (0 if case.kernel == 'thread_per_env' else 1)
        n = run.n_totals_steps
        total = run.totals(0, n)
        many_episodes += int((total['episodes'] >= 2).sum())
        for ref in run.refs:
            fresh = ref['was_terminal'] == 0
            goal_episodes += int((fresh & (ref['done'] == 1) & (ref['collision'] == 0)).sum())
            clash_episodes += int((fresh & (ref['collision'] == 1)).sum())
        if p.family == 'R':
            r_collisions += int(total['collisions'].sum())
        ties += tc.slip_ties(run, thresholds16[p.fail_prob], tc.MIN_TIES - ties)
        # the accumulated totals are not zero anywhere it matters: the overwriting launch must show if it added instead
        lo, hi = run.steps_of(len(p.lengths))
        over = run.totals(lo, hi)
        added = run.totals(lo, hi, base=total)
        assert not np.array_equal(bits(over['returns']), bits(added['returns'])), tag
        assert not np.array_equal(over['episodes'], added['episodes']), tag
        if p.rewards == tc.INEXACT and not p.auto_reset and case.ends_at_once_without_reset:
            assert not p.soc or len(tc.soc_counts(run, n)) >= 3, tag     # (what is left of the conditions below: see the property)
        elif p.rewards == tc.INEXACT:
            tc._assert_a_wrong_rounding_would_show(run.refs[:n], run.prevs[:n], run.acts[:n], run.goal, p.rewards,
                                                   p.soc and case.soc_counts_apply, p.fail_prob, tag)
            # a launch that restarted its chain at zero and added the old total at the end: (earlier launches) + (this launch),
            # at one of the two accumulating launches (the GPU test compares after each)
            shows = 0
            for k in range(1, len(p.lengths)):
                first, last = sum(p.lengths[:k]), sum(p.lengths[:k + 1])
                restarted = run.totals(0, first)['returns'] + run.totals(first, last)['returns']
                shows += int((bits(restarted) != bits(run.totals(0, last)['returns'])).sum())
            assert shows > 0, tag
    assert many_episodes > 0 and goal_episodes > 0 and clash_episodes > 0 and r_collisions > 0, \
        (case.id, many_episodes, goal_episodes, clash_episodes, r_collisions)
    assert case.tie_exempt or ties >= tc.MIN_TIES, (case.id, ties)
