"""Every decision of the three launch planners (csrc/mapf_plan.hip), pinned: plan_rollout_lq, plan_rollout_lq_table and
plan_step_lq are swept over shapes and MAPF_TUNE overrides, and the SHA-256 of each group's concatenated results ("no packed
form" is one of the results) is compared with tests/golden/plan_decisions.json -- recorded from the commit before the planner
was rewritten as ordered candidate lists, so a change of any decision names its group here.  No GPU involved.

    python tests/test_plan_decisions.py --record [OUT.json]

writes the fixture from the library MAPF_HIP_LIB names (default: the tree's) and the host shim MAPF_HOST_SHIM names (default:
built from the tree's sources)."""
import ctypes
import hashlib
import json
import os
import sys
import tempfile

import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN
from test_cabi_and_host import ROLLOUT_PLAN_AGENTS, ROLLOUT_PLAN_CELLS, ROLLOUT_PLAN_ENVS, ROLLOUT_PLAN_TUNES
from test_host_tables import STEP_PLAN_AGENTS, STEP_PLAN_CELLS, STEP_PLAN_CUS, STEP_PLAN_ENVS, STEP_PLAN_TUNES, build_shim, load_shim
from test_host_tables import shim  # noqa: F401  (the host shim, built once per run)

FIXTURE = os.path.join(GOLDEN, 'plan_decisions.json')
NOT_PACKED = b'-'
TABLE_AGENTS, TABLE_ENVS = (4, 8, 16, 32, 64), (1024, 16384, 65536, 262144)
TABLE_BYTES = (1, 8, 64)                                               # policy tables of V, 8 V and 64 V action bytes
TABLE_TUNES = (None, b'policy_table_lds=0', b'policy_table_lds=1')


def _name(tune):
    return tune.decode() if tune else 'default'


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
                            digests['%s A=%d streamed=%d delta=%d n_cu=%d T=%d' % (_name(tune), A, streamed, delta, n_cu, T)] = h.hexdigest()
    return digests


def table_plans(shim_lib):
    """plan_rollout_lq_table over the same cells: yields (group, result or None)"""
    out = (ctypes.c_uint64 * 8)()
    for tune in TABLE_TUNES:
        for A in TABLE_AGENTS:
            for mult in TABLE_BYTES:
                for delta in (0, 1):
                    group = '%s A=%d table_bytes=%dV delta=%d' % (_name(tune), A, mult, delta)
                    for E in TABLE_ENVS:
                        for V in ROLLOUT_PLAN_CELLS:
                            rc = shim_lib.shim_plan_rollout_table(V, A, E, 64, delta, mult * V, 256, tune, out)
                            assert rc in (0, 1), (rc, tune)
                            yield group, (V, E, tuple(out)) if rc else None


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
                digests['%s n_cu=%d A=%d' % (_name(tune), n_cu, A)] = h.hexdigest()
    return digests


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


if __name__ == '__main__':
    if len(sys.argv) < 2 or sys.argv[1] != '--record':
        sys.exit(__doc__)
    from gym_mapf_amd import _native
    shim_path = os.environ.get('MAPF_HOST_SHIM') or build_shim(tempfile.mkdtemp(prefix='host_tables_'))
    shim_lib = load_shim(shim_path)
    record = {'plan_rollout_lq': rollout_digests(_native.load()), 'plan_rollout_lq_table': table_digests(shim_lib),
              'plan_step_lq': step_digests(shim_lib)}
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, 'w') as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %s groups from %s and %s' % ({k: len(v) for k, v in record.items()}, _native.LIB_PATH, shim_path))
