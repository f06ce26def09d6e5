"""Every decision of the launch planners (csrc/mapf_plan.hip), pinned.

The packed planners -- plan_rollout_lq, plan_rollout_lq_table and plan_step_lq -- are swept over shapes and MAPF_TUNE overrides, and
the SHA-256 of each group's concatenated results ("no packed form" is one of the results) is compared with
tests/golden/plan_decisions.json -- recorded from the commit before the planner was rewritten as ordered candidate lists, so a
change of any decision names its group here.

The lane-group planners -- plan_rollout_lg and plan_step_lg -- take every launch the packed kernels decline.  Their recorded
decisions are those of the commit before they existed, when the launchers decided inline and only mapf_last_kernel showed what
they decided: every shape of the LG_* sweep (tests/plan_sweeps.py) was launched once on an MI355X (a one-step rollout, a step) and the kernel's name
parsed into the fields a plan holds.  The fixture keeps them per shape ('-' = a packed kernel took the launch), and the full name
of one shape per distinct name.  The comparison involves no GPU; one GPU test launches a shape of every kind.

    python tests/test_plan_decisions.py --record [OUT.json] [packed] [lane_group]

writes the fixture from the library MAPF_HIP_LIB names (default: the tree's) and the host shim MAPF_HOST_SHIM names (default:
built from the tree's sources); `packed` / `lane_group` alone re-records those groups only and keeps the others of OUT.json.
`lane_group` needs a GPU.

The limit instances of the lane-group family (mapf_lg_limit.hip) are named by the same two planners, asked for a limit plan.  Their
plans and full names over LIMIT_* (tests/plan_sweeps.py) are compared with tests/golden/plan_decisions_limit.json, recorded on the CPU from the
commit that still had a planner and name functions of their own for them (tests/golden/generation_info.json says how):

    python tests/test_plan_decisions.py --record-limit [OUT.json]

The packed rollout launches are named by lq_rollout_kernel_name.  tests/golden/lq_kernel_names.json holds what mapf_last_kernel said
after a one-step rollout of every launch of lq_launches() below -- every packed instance list entry, every policy, criteria /
terminal variant, recording or not, both table forms, with and without the limit -- on an MI355X, from the library of the commit
whose launchers still formatted these names themselves (MAPF_HIP_LIB; generation_info.json says how):

    python tests/test_plan_decisions.py --record-lq-names [OUT.json]

The packed single step is named by lq_step_kernel_name.  tests/golden/lq_step_kernel_names.json holds what mapf_last_kernel said after
a step of every launch of LQ_STEP_LAUNCHES (tests/plan_sweeps.py) -- every entry of the step's instance list, with and without the scenario table, a step
that may meet a terminal env and one that cannot -- on an MI355X, from the library of the commit whose launcher still formatted these
names itself:

    python tests/test_plan_decisions.py --record-lq-step-names [OUT.json]"""
import ctypes
import hashlib
import json
import os
import re
import sys
import tempfile

import pytest

from conftest import GOLDEN
from host_shim import build_shim, load_shim, step_instances
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import (FIXTURE, FIXTURE_LQ_NAMES, FIXTURE_LQ_STEP_NAMES, KERNEL_NAME_BYTES, LG_AGENTS, LG_ENVS, LG_MAPS, LG_PACKED, LG_ROLLOUTS, LG_STEPS, LIMIT_AGENTS,
                         LIMIT_CELLS, LIMIT_ENVS, LQ_STEP_LAUNCHES, LQ_TABLE_ROWS, PACKED, PREFER_LG, ROLLOUT_PLAN_AGENTS, ROLLOUT_PLAN_CELLS, ROLLOUT_PLAN_ENVS,
                         ROLLOUT_PLAN_TUNES, STEP_PLAN_AGENTS, STEP_PLAN_CELLS, STEP_PLAN_CUS, STEP_PLAN_ENVS, STEP_PLAN_TUNES, TABLE_AGENTS, TABLE_BYTES, TABLE_ENVS,
                         TABLE_TUNES, LaneGroupLauncher, launch_lq, lg_key, lg_shapes, lq_fixture, lq_step_fixture, parse_lg_key, plan_fixture, planned_rollout_lg,
                         planned_step_lg, routed_rollout, routed_step, tune_name, tuned_env)

NOT_PACKED = b'-'
LG_ROLLOUT_NAME = re.compile(r'^lg_rollout_kernel(_table)?<L=(\d+),(FULL|RAGGED),(MV_LDS|MV_GLOBAL),(RECORD|TOTALS),(STREAM|POLICY|TABLE),(DENSE|GUARDED)> block=(\d+) ')
LG_STEP_NAME = re.compile(r'^lg_step_kernel<L=(\d+),(FULL|RAGGED),(EXT_UNIFORMS|PHILOX)> block=(\d+) ')
LG_ROLLOUT_CODE, LG_STEP_CODE = re.compile(r'^(\d+)([FR])([LG])([DG])(\d+)$'), re.compile(r'^(\d+)([FR])(\d+)$')   # (lg_rollout_code, lg_step_code)
FIXTURE_LIMIT = os.path.join(GOLDEN, 'plan_decisions_limit.json')
# (criteria, auto-reset): no env of these launches starts terminal, so a launch may meet a terminal env exactly without auto-reset
LQ_VARIANTS = {'SOC': ('SoC', True), 'MAKESPAN': ('Makespan', False), 'NO_TERMINAL': ('Makespan', True)}
LQ_POLICIES = ('STREAM', 'POLICY', 'TABLE')
STEP_FORM_TAG, STEP_FORM_BLOCK = ('', ',BIG', ',DELTA', ',DELTA,BITMAP'), (64, 1024, 512, 512)   # what a name says of each StepForm: its tag, its block
# (scenario table, may be terminal): the handles' rows come from five scenarios, so MAPF_TUNE scen_table=0 is what leaves the table out;
# no env starts terminal, so a step may meet a terminal env exactly when the step before it ran without auto-reset
LQ_STEP_VARIANTS = {'%s %s' % ('SCEN' if scen else 'ROWS', 'TERMINAL' if term else 'NO_TERMINAL'): (scen, term) for scen in (True, False) for term in (True, False)}


def rollout_digests(lib):
    """plan_rollout_lq through mapf_debug_rollout_plan: the sweep of test_packed_rollout_dispatch_never_plans_past_the_lds_or_
    launch_bounds, on 256 and 64 CUs, for launches of 64 and of 65536 steps (one more than a packed launch counts)."""
    out = (ctypes.c_uint64 * 6)()
    plan = lib.mapf_debug_rollout_plan
    digests = {}
    for tune in ROLLOUT_PLAN_TUNES:
        for A in ROLLOUT_PLAN_AGENTS:
            for streamed in (1, 0):
                for delta in (0, 1):
                    for n_cu in (256, 64):
                        for T in (64, 65536):
                            h = hashlib.sha256()
                            for E in ROLLOUT_PLAN_ENVS:
                                for V in ROLLOUT_PLAN_CELLS:
                                    rc = plan(V, A, E, T, streamed, delta, n_cu, tune, out)
                                    assert rc in (0, 1), (rc, tune)
                                    h.update(bytes(out) if rc else NOT_PACKED)
                            digests['%s A=%d streamed=%d delta=%d n_cu=%d T=%d' % (tune_name(tune), A, streamed, delta, n_cu, T)] = h.hexdigest()
    return digests


def table_plans(shim_lib):
    """plan_rollout_lq_table over the same cells: yields (group, result or None)"""
    out = (ctypes.c_uint64 * 9)()
    for tune in TABLE_TUNES:
        for A in TABLE_AGENTS:
            for mult in TABLE_BYTES:
                for delta in (0, 1):
                    group = '%s A=%d table_bytes=%dV delta=%d' % (tune_name(tune), A, mult, delta)
                    for E in TABLE_ENVS:
                        for V in ROLLOUT_PLAN_CELLS:
                            rc = shim_lib.shim_plan_rollout_table(V, A, E, 64, delta, mult * V, 256, tune, 0, out, None)
                            assert rc in (0, 1) and (not rc or out[8] == 0), (rc, tune)
                            yield group, (V, E, tuple(out)[:8]) if rc else None   # (the recorded eight fields; the ninth marks a limit plan)


def table_digests(shim_lib):
    hashes = {}
    for group, result in table_plans(shim_lib):
        hashes.setdefault(group, hashlib.sha256()).update(repr(result[2]).encode() if result else NOT_PACKED)
    return {group: h.hexdigest() for group, h in hashes.items()}


def step_digests(shim_lib):
    """plan_step_lq: the sweep of test_packed_step_plan_stays_within_the_lds_and_its_residency"""
    out = (ctypes.c_uint64 * 8)()
    digests = {}
    for tune in STEP_PLAN_TUNES:
        for n_cu in STEP_PLAN_CUS:
            for A in STEP_PLAN_AGENTS:
                h = hashlib.sha256()
                for E in STEP_PLAN_ENVS:
                    for delta in (0, 1):
                        for V in STEP_PLAN_CELLS:
                            rc = shim_lib.shim_plan_step(V, A, E, delta, n_cu, tune, out)
                            assert rc in (0, 1), (rc, tune)
                            h.update(bytes(out) if rc else NOT_PACKED)
                digests['%s n_cu=%d A=%d' % (tune_name(tune), n_cu, A)] = h.hexdigest()
    return digests


def lg_rollout_code(name, record, policy):
    """a rollout kernel's name as the fields of a plan: '<L><F|R><L|G><D|G><block>' (full or ragged groups, move table in LDS or
    global memory, dense or guarded), '-' for a packed kernel; what the name says about recording and the policy must be what
    the launch asked for"""
    if name.startswith('lq_rollout_kernel'):
        return LG_PACKED
    m = LG_ROLLOUT_NAME.match(name)
    assert m, name
    table, L, full, mv, rec, pol, dense, block = m.groups()
    assert rec == ('RECORD' if record else 'TOTALS') and pol == ('STREAM', 'POLICY', 'TABLE')[policy] and (table is not None) == (policy == 2), name
    return '%s%s%s%s%s' % (L, full[0], 'L' if mv == 'MV_LDS' else 'G', dense[0], block)


def lg_step_code(name, uniforms):
    """... of a step kernel: '<L><F|R><block>'"""
    if name.startswith('lq_step_kernel'):
        return LG_PACKED
    m = LG_STEP_NAME.match(name)
    assert m, name
    L, full, ext, block = m.groups()
    assert ext == ('EXT_UNIFORMS' if uniforms else 'PHILOX'), name
    return '%s%s%s' % (L, full[0], block)


def limit_plans(shim_lib):
    """the limit plans and names of the LIMIT_* sweep: {'rollout': {shape: 'L full mv_lds dense block grid lds_bytes|name'}, 'step':
    {shape: 'L full block grid|name'}}"""
    out, name = (ctypes.c_uint64 * 7)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    rollouts, steps = {}, {}
    for A in LIMIT_AGENTS:
        for E in LIMIT_ENVS:
            for V in LIMIT_CELLS:
                for record, policy in LG_ROLLOUTS:
                    assert shim_lib.shim_plan_limit_rollout_lg(V, A, E, record, policy, None, out, name) == 1
                    rollouts['V=%d A=%d E=%d record=%d policy=%d' % (V, A, E, record, policy)] = '%s|%s' % (' '.join(str(x) for x in out), name.value.decode())
            for uniforms in LG_STEPS:
                assert shim_lib.shim_plan_limit_step_lg(A, E, uniforms, out, name) == 1
                steps['A=%d E=%d uniforms=%d' % (A, E, uniforms)] = '%s|%s' % (' '.join(str(x) for x in out[:4]), name.value.decode())
    return {'rollout': rollouts, 'step': steps}


def lq_launches():
    """the handles of the packed-name fixture: (key, family, A, E, tune text, policy, limited, the parts the case says the names hold)"""
    import limit_packed_cases as lp
    import totals_cases as tc
    for c in tc.PACKED_CASES:
        for policy in LQ_POLICIES[:2]:
            yield '%s %s' % (c.id, policy), 'plain', c.A, c.E, c.tune_text(), policy, False, ('<Q=%d,K=%d,' % (c.Q, c.K),) + tc.FORM_NAME[c.form]
    for c in lp.CASES:
        for table_lds in lp.TABLE_LDS:
            for limited in (False, True):
                tune = c.tune_bytes(table_lds, limit_packed=limited).decode()
                parts = c.name_parts(table_lds) if limited else ('lq_rollout_kernel_table<Q=%d,K=%d,' % (c.Q, c.K),) + c.name_parts(table_lds)[1:2] + c.name_parts(table_lds)[3:]
                yield '%s lds=%d limit=%d' % (c.id, table_lds, limited), 'table', c.A, c.E, tune, 'TABLE', limited, parts


def record_lq_names(n_cu):
    """{'n_cu', 'launches': {key: {'V', 'A', 'E', 'tune', 'delta', 'table_bytes', 'policy', 'limited', 'names': {'<variant> <RECORD|TOTALS>': full
    name}}}}: what the CPU side needs to plan the same launch, and what the GPU side said"""
    import episode_limit_cases as ec
    grid, found = ec.random_map(3), {}
    V = len(grid.tables()[0])
    for key, family, A, E, tune, policy, limited, parts in lq_launches():
        names = {}
        for criteria in ('SoC', 'Makespan'):                    # (one handle per criteria)
            runs = [(variant, auto_reset, record) for variant, (c, auto_reset) in LQ_VARIANTS.items() if c == criteria for record in (True, False)]
            for (variant, _, record), name in zip(runs, launch_lq(grid, A, E, tune, policy, limited, criteria, [run[1:] for run in runs])):
                says = (',RECORD,' if record else ',TOTALS,', ',%s,' % policy, ',SOC' if criteria == 'SoC' else ',MAKESPAN')
                assert all(part in name for part in parts + says) and ('NO_TERMINAL' in name) == (variant == 'NO_TERMINAL'), (key, variant, name, parts)
                names['%s %s' % (variant, 'RECORD' if record else 'TOTALS')] = name
        print('launched %s' % key, flush=True)
        found[key] = {'V': V, 'A': A, 'E': E, 'tune': tune, 'delta': 1, 'table_bytes': LQ_TABLE_ROWS * V if policy == 'TABLE' else 0, 'policy': policy,
                      'limited': int(limited), 'names': names}
    return {'n_cu': n_cu, 'launches': found}


def planned_lq_name(shim_lib, n_cu, launch, variant, record):
    """the same launch through the planner and lq_rollout_kernel_name (the shim): the name, or None where no packed form applies"""
    name = ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    criteria, auto_reset = LQ_VARIANTS[variant]
    rc = shim_lib.shim_lq_rollout_name(launch['V'], launch['A'], launch['E'], launch['delta'], launch['table_bytes'], n_cu, launch['tune'].encode() or None,
                                       LQ_POLICIES.index(launch['policy']), launch['limited'], int(record), int(criteria == 'SoC'), int(not auto_reset), name)
    assert rc in (0, 1), (rc, launch)
    return name.value.decode() if rc else None


def launch_lq_step(grid, A, E, tune, scen):
    """a handle of that shape under `tune` whose rows come from five scenarios (scen: through the scenario table; else scen_table=0),
    and the names of two of its steps: one that may meet a terminal env (the step before it ran without auto-reset) and, right after
    that auto-reset step, one that cannot"""
    import numpy as np
    rows = (np.arange(E) % 5)[:, None] + np.arange(A)[None, :]
    env = tuned_env(grid, A, E, ','.join(filter(None, (tune, '' if scen else 'scen_table=0'))), 'Makespan', rows, rows + 1)
    try:
        names, actions = [], np.zeros((E, A), np.uint8)
        for auto_reset in (False, True, True):
            env.step(actions, auto_reset=auto_reset)
            names.append(env.last_kernel('step'))
        return names[1:]
    finally:
        env.close()


def lq_step_head(form, K, Q, scen, term):
    """what the name of that instance begins with"""
    return 'lq_step_kernel<Q=%d,K=%d%s%s%s> block=%d ' % (Q, K, ',SCEN' if scen else '', '' if term else ',NO_TERMINAL', STEP_FORM_TAG[form], STEP_FORM_BLOCK[form])


def record_lq_step_names(n_cu):
    """{'n_cu', 'launches': {key: {'V', 'A', 'E', 'tune', 'delta', 'names': {'<SCEN|ROWS> <TERMINAL|NO_TERMINAL>': full name}}}}"""
    import episode_limit_cases as ec
    grid, found = ec.random_map(3), {}
    V = len(grid.tables()[0])
    for key, (form, K, Q, E, tune) in LQ_STEP_LAUNCHES.items():
        names = {}
        for scen in (True, False):
            for term, name in zip((True, False), launch_lq_step(grid, K * Q, E, tune, scen)):
                assert name.startswith(lq_step_head(form, K, Q, scen, term)), (key, scen, term, name)
                names['%s %s' % ('SCEN' if scen else 'ROWS', 'TERMINAL' if term else 'NO_TERMINAL')] = name
        print('launched %s' % key, flush=True)
        found[key] = {'V': V, 'A': K * Q, 'E': E, 'tune': tune, 'delta': 1, 'names': names}
    return {'n_cu': n_cu, 'launches': found}


def planned_lq_step(shim_lib, n_cu, launch, scen, term):
    """the same step through the planner and lq_step_kernel_name (the shim): ((Q, K, form), name), or None where no packed form applies"""
    out, name = (ctypes.c_uint64 * 8)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    tune = ','.join(filter(None, (launch['tune'], '' if scen else 'scen_table=0'))).encode() or None
    shape = (launch['V'], launch['A'], launch['E'], launch['delta'], n_cu, tune)
    rc = shim_lib.shim_lq_step_name(*shape, int(scen), int(term), name)
    assert rc in (0, 1) and shim_lib.shim_plan_step(*shape, out) == rc, (rc, launch)
    return ((out[1], out[0], out[2]), name.value.decode()) if rc else None


def record_lane_group():
    """the two lane-group groups and the kept names: of every distinct name, the smallest shape that printed it"""
    launcher = LaneGroupLauncher()
    rollouts, steps, kept = {}, {}, {}
    for tune, rows, cols, A, E in lg_shapes():
        key = lg_key(tune, rows * cols, A, E)
        rollout_names, step_names = launcher.names(tune, rows, cols, A, E)
        rollouts[key] = ' '.join(lg_rollout_code(name, *LG_ROLLOUTS[i]) for i, name in enumerate(rollout_names))
        steps[key] = ' '.join(lg_step_code(name, LG_STEPS[i]) for i, name in enumerate(step_names))
        for planner, names in (('rollout', rollout_names), ('step', step_names)):
            for i, name in enumerate(names):
                if name.startswith('lg_') and (name not in kept or E * A < kept[name][0]):
                    kept[name] = (E * A, '%s|%d|%s' % (planner, i, key))
        if E == LG_ENVS[-1] and A == LG_AGENTS[-1]:
            print('launched %s V=%d' % (tune_name(tune), rows * cols), flush=True)
    return rollouts, steps, {name: where for name, (_, where) in kept.items()}


def _compare(planner, found):
    with open(FIXTURE) as f:
        recorded = json.load(f)[planner]
    assert sorted(found) == sorted(recorded), 'the sweep of %s has other groups than the recorded one' % planner
    differing = [group for group in found if found[group] != recorded[group]]
    assert not differing, '%s decides differently in %d of %d groups: %s' % (planner, len(differing), len(found), differing[:12])


def test_rollout_plan_decisions_are_the_recorded_ones():
    from gym_mapf_amd import _native
    found = rollout_digests(_native.load())
    assert len(found) == 12 * 7 * 2 * 2 * 2 * 2
    _compare('plan_rollout_lq', found)


def test_table_rollout_plan_decisions_are_the_recorded_ones_and_instantiated(shim):  # noqa: F811
    """... and whatever plan_rollout_lq_table plans is an instance of lq_rollout_kernel_table the launcher holds, in a block of at
    most 512 threads, within the CU's LDS"""
    hashes, n_packed, n_lds, forms = {}, 0, 0, set()
    for group, result in table_plans(shim):
        hashes.setdefault(group, hashlib.sha256()).update(repr(result[2]).encode() if result else NOT_PACKED)
        if result:
            V, E, (K, Q, form, block, image, total, table_lds, table_at) = result
            ctx = (group, V, E) + result[2]
            n_packed += 1
            n_lds += table_lds
            forms.add(form)
            assert shim.shim_rollout_instance_exists(K, Q, form, 1) == 1, ctx
            assert block <= 512 and E % (block // Q) == 0 and 1024 < image <= total <= 160 * 1024, ctx
            assert table_lds in (0, 1) and (table_at % 16 == 0 and image <= table_at < total if table_lds else table_at == 0), ctx
    assert forms == {0, 5} and n_packed > 20000 and 0 < n_lds < n_packed, (forms, n_packed, n_lds)
    _compare('plan_rollout_lq_table', {group: h.hexdigest() for group, h in hashes.items()})


def test_step_plan_decisions_are_the_recorded_ones(shim):  # noqa: F811
    _compare('plan_step_lq', step_digests(shim))


def test_lane_group_plans_are_the_recorded_ones(shim):  # noqa: F811
    """plan_rollout_lg and plan_step_lg decide what the inline launchers decided on the GPU, shape by shape; the grid follows from
    block, L and E, the dynamic LDS segment is the move table or nothing; the kept names are formatted byte for byte.  Where a
    packed kernel took the launch there is no lane-group plan to compare: the route must say packed there (tests/test_route.py
    compares the route with every entry) -- none with the packed layout off, and no more than half of the sweep in all."""
    recorded = plan_fixture()
    rollouts, steps, names = recorded['plan_rollout_lg'], recorded['plan_step_lg'], recorded['lg_kernel_names']
    keys = [lg_key(tune, rows * cols, A, E) for tune, rows, cols, A, E in lg_shapes()]
    assert len(keys) == 4 * 4 * 11 * 9 and sorted(keys) == sorted(rollouts) == sorted(steps)
    sizes = (ctypes.c_uint64 * 6)()
    shim.shim_sizes(2, sizes)
    mv_cols = sizes[0]                                           # (16-byte entries per cell of the move table)
    n, skipped, skipped_unpacked, wrong = 0, 0, 0, []
    for key in keys:
        tune, V, A, E = parse_lg_key(key)
        unpacked = tune is not None and b'quad_lanes=0' in tune
        rollout_codes, step_codes = rollouts[key].split(' '), steps[key].split(' ')
        assert len(rollout_codes) == len(LG_ROLLOUTS) and len(step_codes) == len(LG_STEPS), key
        for (record, policy), want in zip(LG_ROLLOUTS, rollout_codes):
            n += 1
            if want == LG_PACKED:
                skipped += 1
                skipped_unpacked += unpacked
                if routed_rollout(shim, V, A, E, PREFER_LG, policy, tune, record=record)[0] != PACKED:
                    wrong.append((key, record, policy, want))
                continue
            code, grid, lds_bytes, _ = planned_rollout_lg(shim, tune, V, A, E, record, policy)
            L, _, mv, _, block = LG_ROLLOUT_CODE.match(want).groups()
            if (code, grid, lds_bytes) != (want, -(-E // (int(block) // int(L))), V * mv_cols * 16 if mv == 'L' else 0):
                wrong.append((key, record, policy, want, code, grid, lds_bytes))
        for uniforms, want in zip(LG_STEPS, step_codes):
            n += 1
            if want == LG_PACKED:
                skipped += 1
                skipped_unpacked += unpacked
                if routed_step(shim, V, A, E, PREFER_LG, uniforms, tune)[0] != PACKED:
                    wrong.append((key, 'step', uniforms, want))
                continue
            code, grid, _ = planned_step_lg(shim, A, E, uniforms)
            L, _, block = LG_STEP_CODE.match(want).groups()
            if (code, grid) != (want, -(-E // (int(block) // int(L)))):
                wrong.append((key, 'step', uniforms, want, code, grid))
    assert not wrong, '%d of %d lane-group launches are planned differently: %s' % (len(wrong), n, wrong[:12])
    assert n == len(keys) * 8 and skipped_unpacked == 0 and 2 * skipped <= n, (n, skipped, skipped_unpacked)
    assert len(names) > 100
    for name, where in names.items():
        planner, i, key = where.split('|')
        tune, V, A, E = parse_lg_key(key)
        found = planned_rollout_lg(shim, tune, V, A, E, *LG_ROLLOUTS[int(i)])[3] if planner == 'rollout' else planned_step_lg(shim, A, E, LG_STEPS[int(i)])[2]
        assert found == name and len(name) < KERNEL_NAME_BYTES, (where, found, name)


def test_limit_plans_and_names_are_the_recorded_ones(shim):  # noqa: F811
    """plan_rollout_lg and plan_step_lg asked for a limit plan, and the names of those plans, against what the limit family's own
    planner and name functions gave before the two were folded: every field and every byte of the name; never dense"""
    with open(FIXTURE_LIMIT) as f:
        recorded = json.load(f)
    found = limit_plans(shim)
    assert len(found['rollout']) == 11 * 5 * 3 * 6 and len(found['step']) == 11 * 5 * 2
    for kind in ('rollout', 'step'):
        assert sorted(found[kind]) == sorted(recorded[kind]), kind
        wrong = [(shape, found[kind][shape], recorded[kind][shape]) for shape in found[kind] if found[kind][shape] != recorded[kind][shape]]
        assert not wrong, '%d of %d limit %s plans or names differ: %s' % (len(wrong), len(found[kind]), kind, wrong[:6])
    for line in found['rollout'].values():
        fields, name = line.split('|')
        assert fields.split(' ')[3] == '0' and '_limit_guarded<' in name and ',LIMIT> ' in name and len(name) < KERNEL_NAME_BYTES, line


def test_packed_rollout_names_are_the_recorded_ones(shim):  # noqa: F811
    """the planner and lq_rollout_kernel_name, asked for every launch of the fixture, against what the launchers' own format strings
    printed on the GPU before the name had one function: byte for byte, and shorter than what mapf_last_kernel keeps"""
    recorded = lq_fixture()
    launches, n = recorded['launches'], 0
    wanted = list(lq_launches())
    assert sorted(launches) == sorted(w[0] for w in wanted) and len(wanted) == 20 * 2 + 9 * 2 * 2
    for key, family, A, E, tune, policy, limited, parts in wanted:
        launch = launches[key]
        assert (launch['A'], launch['E'], launch['tune'], launch['policy'], launch['limited']) == (A, E, tune, policy, int(limited)), key
        assert sorted(launch['names']) == sorted('%s %s' % (v, r) for v in LQ_VARIANTS for r in ('RECORD', 'TOTALS')), key
        for which, name in launch['names'].items():
            variant, recording = which.split(' ')
            found = planned_lq_name(shim, recorded['n_cu'], launch, variant, recording == 'RECORD')
            assert found == name and len(name) < KERNEL_NAME_BYTES and all(part in name for part in parts), (key, which, found, name)
            n += 1
    assert n == 20 * 2 * 6 + 9 * 2 * 2 * 6 and len({name for launch in launches.values() for name in launch['names'].values()}) == n


# one launch set per packed family: the smallest full-block batches of the case tables (plain streamed, plain in-kernel policy, the
# table policy over full rows and over delta rows, both without and under the limit)
LQ_GPU_LAUNCHES = ('K2-Q16-FullRows STREAM', 'K4-Q8-DeltaRowsBitmap POLICY', 'k2-4x512 lds=0 limit=0', 'mv_lds_max_bytes1024-32x128 lds=1 limit=0',
                   'k2-4x512 lds=0 limit=1', 'mv_lds_max_bytes1024-32x128 lds=1 limit=1')


@pytest.mark.gpu
def test_packed_launches_print_the_recorded_names():
    """the launcher that takes a plan notes the name the plan's name function gives: a launch of every packed family, without terminal
    handling and totals only, then with it and recording, each compared in full with the recorded name"""
    import episode_limit_cases as ec
    launches, grid = lq_fixture()['launches'], ec.random_map(3)
    for key in LQ_GPU_LAUNCHES:
        launch = launches[key]
        assert (launch['A'], launch['E']) in ((32, 1024), (32, 2048), (4, 512), (32, 128)) and launch['V'] == len(grid.tables()[0]), key
        found = launch_lq(grid, launch['A'], launch['E'], launch['tune'], launch['policy'], launch['limited'], 'Makespan', [(True, False), (False, True)])
        assert found == [launch['names']['NO_TERMINAL TOTALS'], launch['names']['MAKESPAN RECORD']], (key, found)


def test_packed_step_names_are_the_recorded_ones(shim):  # noqa: F811
    """plan_step_lq and lq_step_kernel_name, asked for every step of the fixture, against what the launcher's own format strings printed
    on the GPU before the name had a function: byte for byte, shorter than what mapf_last_kernel keeps, every instance of the list"""
    recorded = lq_step_fixture()
    launches, names, seen = recorded['launches'], set(), set()
    assert sorted(launches) == sorted(LQ_STEP_LAUNCHES) and len(launches) == 21
    for key, (form, K, Q, E, tune) in LQ_STEP_LAUNCHES.items():
        launch = launches[key]
        assert (launch['A'], launch['E'], launch['tune']) == (K * Q, E, tune) and sorted(launch['names']) == sorted(LQ_STEP_VARIANTS), key
        for which, (scen, term) in LQ_STEP_VARIANTS.items():
            name = launch['names'][which]
            instance, found = planned_lq_step(shim, recorded['n_cu'], launch, scen, term)
            assert instance == (Q, K, form) and found == name and len(name) < KERNEL_NAME_BYTES and name.startswith(lq_step_head(form, K, Q, scen, term)), \
                (key, which, instance, found, name)
            names.add(name)
            seen.add(instance)
    assert len(names) == 84 and seen == step_instances(shim), (len(names), sorted(seen))


# one step launch per form: the shapes of wide_counter_cases.STEP_CASES' rows A8-Q2K4-SCEN, A8-Q4K2, A16-Q2K8-BIG, A32-DELTA and
# A32-DELTA-BITMAP at the fixture's batches (scenario table or not, as those rows have it)
LQ_STEP_GPU_LAUNCHES = (('Plain-K4-Q2', True), ('Plain-K2-Q4', False), ('FullRows-K8-Q2', False), ('DeltaRows-K4-Q8', False), ('DeltaRowsBitmap-K4-Q8', False))


@pytest.mark.gpu
def test_packed_step_launches_print_the_recorded_names():
    """the step's launcher notes the name the plan's name function gives: a launch of every form, a step that may be terminal and then
    one after an auto-reset step, each compared in full with the recorded name"""
    import episode_limit_cases as ec
    launches, grid = lq_step_fixture()['launches'], ec.random_map(3)
    for key, scen in LQ_STEP_GPU_LAUNCHES:
        launch, rows = launches[key], 'SCEN' if scen else 'ROWS'
        assert launch['E'] <= 1024 and launch['V'] == len(grid.tables()[0]), key
        found = launch_lq_step(grid, launch['A'], launch['E'], launch['tune'], scen)
        assert found == [launch['names'][rows + ' TERMINAL'], launch['names'][rows + ' NO_TERMINAL']], (key, found)


def lg_kinds(recorded):
    """{kind: (shape's key, index into LG_ROLLOUTS, recorded name)}: the smallest shape of every combination that exists of full /
    ragged groups, move table in LDS / global memory, dense / guarded and table policy or not; plus the smallest one whose block
    the 16-lane cap cut to 512 threads (V = 1500 leaves one table copy per CU: 1024 threads for every other group size).  A name
    is a function of the recorded fields, recording and policy, and the fixture keeps every distinct name once."""
    kinds, size, name_of = {}, {}, {}
    for name, where in recorded['lg_kernel_names'].items():
        planner, i, key = where.split('|')
        if planner == 'rollout':
            name_of[lg_rollout_code(name, *LG_ROLLOUTS[int(i)]), int(i)] = name
    for key, codes in recorded['plan_rollout_lg'].items():
        _, V, A, E = parse_lg_key(key)
        for i, code in enumerate(codes.split(' ')):
            if code == LG_PACKED:
                continue
            L, full, mv, dense, block = LG_ROLLOUT_CODE.match(code).groups()
            capped = (L, mv, block) == ('16', 'L', '512') and V == 1500
            for kind in [(full, mv, dense, LG_ROLLOUTS[i][1] == 2)] + ([('the L = 16 cap',)] if capped else []):
                if kind not in kinds or E * A < size[kind]:
                    kinds[kind], size[kind] = (key, i, name_of[code, i]), E * A
    return kinds


@pytest.mark.gpu
def test_lane_group_launches_print_the_recorded_names():
    """the launcher that takes a plan launches the instance the plan names: a shape of every kind of the sweep, each compared with
    the name recorded for it"""
    kinds = lg_kinds(plan_fixture())
    assert len(kinds) == 13, sorted(kinds, key=str)              # FULL: 2 x 2 x 2, RAGGED (never dense): 2 x 2, the cap
    launcher = LaneGroupLauncher()
    for kind, (key, i, name) in sorted(kinds.items(), key=str):
        tune, V, A, E = parse_lg_key(key)
        rows, cols = [m for m in LG_MAPS if m[0] * m[1] == V][0]
        assert launcher.names(tune, rows, cols, A, E)[0][i] == name, (kind, key, i)


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == '--record-limit':
        shim_path = os.environ.get('MAPF_HOST_SHIM') or build_shim(tempfile.mkdtemp(prefix='host_tables_'))
        with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE_LIMIT, 'w') as f:
            json.dump(limit_plans(load_shim(shim_path)), f, indent=0, sort_keys=True)
            f.write('\n')
        sys.exit(0)
    if len(sys.argv) >= 2 and sys.argv[1] in ('--record-lq-names', '--record-lq-step-names'):   # (need a GPU: its CU count is what the handles' tuning starts from)
        import torch
        from gym_mapf_amd import _native
        record, default = (record_lq_names, FIXTURE_LQ_NAMES) if sys.argv[1] == '--record-lq-names' else (record_lq_step_names, FIXTURE_LQ_STEP_NAMES)
        with open(sys.argv[2] if len(sys.argv) > 2 else default, 'w') as f:
            json.dump(record(torch.cuda.get_device_properties(0).multi_processor_count), f, indent=0, sort_keys=True)
            f.write('\n')
        print('recorded the packed %s names from %s' % ('rollout' if record is record_lq_names else 'step', _native.LIB_PATH))
        sys.exit(0)
    if len(sys.argv) < 2 or sys.argv[1] != '--record':
        sys.exit(__doc__)
    from gym_mapf_amd import _native
    out_path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    groups = sys.argv[3:] or ['packed', 'lane_group']
    assert set(groups) <= {'packed', 'lane_group'}, __doc__
    record = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            record = json.load(f)
    if 'lane_group' in groups:
        record['plan_rollout_lg'], record['plan_step_lg'], record['lg_kernel_names'] = record_lane_group()
    if 'packed' in groups:
        shim_path = os.environ.get('MAPF_HOST_SHIM') or build_shim(tempfile.mkdtemp(prefix='host_tables_'))
        shim_lib = load_shim(shim_path)
        record.update({'plan_rollout_lq': rollout_digests(_native.load()), 'plan_rollout_lq_table': table_digests(shim_lib),
                       'plan_step_lq': step_digests(shim_lib)})
    with open(out_path, 'w') as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %s of %s from %s' % (groups, {k: len(v) for k, v in record.items()}, _native.LIB_PATH))
