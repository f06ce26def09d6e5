"""CPU-side checks of the packed table-policy rollout under the episode step limit (MAPF_TUNE limit_packed=1, csrc/mapf_lq_limit.hip):
the tuning key, the limited form of plan_rollout_lq_table over the case table of tests/limit_packed_cases.py, the device listings
of the limit unit, and the outcomes the reference shows for every case.  No compute is launched here."""
import ctypes

import pytest

import episode_limit_cases as ec
import limit_packed_cases as lp
from gym_mapf_amd import _native as nat
from host_shim import device_listings, kernel_meta
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import ROLLOUT_PLAN_CELLS, TABLE_AGENTS, TABLE_BYTES, TABLE_ENVS, TABLE_TUNES

LDS = 160 * 1024


def _plan(shim, V, A, E, tune, limited, n_steps=64, delta=1, table_bytes=None):
    """(rc, the nine plan fields, what the tune string says of limit_packed)"""
    out, key = (ctypes.c_uint64 * 9)(), ctypes.c_int(-1)
    rc = shim.shim_plan_rollout_table(V, A, E, n_steps, delta, V * V if table_bytes is None else table_bytes, lp.N_CU, tune, int(limited), out, ctypes.byref(key))
    return rc, tuple(out), key.value


def test_the_tuning_key_is_accepted_and_defaults_to_off(shim):
    for tune, want in ((None, 0), (b'limit_packed=0', 0), (b'limit_packed=1', 1), (b'k=2,limit_packed=1', 1), (b'limit_packed=1,policy_table_lds=0', 1)):
        rc, _, key = _plan(shim, lp.V, 8, 256, tune, True)
        assert rc in (0, 1) and key == want, (tune, rc, key)
    assert _plan(shim, lp.V, 8, 256, b'limit_packed', True)[0] == -1 and _plan(shim, lp.V, 8, 256, b'limit_packed=x', True)[0] == -1


def test_the_limited_debug_plan_accepts_the_key_and_stays_the_lane_group_plan():
    """mapf_debug_rollout_plan_limited describes launches without a table policy: the key changes nothing of its answer"""
    lib = nat.load()
    plain, keyed = (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 6)()
    for c in lp.CASES:
        for streamed in (0, 1):
            assert lib.mapf_debug_rollout_plan_limited(lp.V, c.A, c.E, 64, streamed, 1, lp.N_CU, c.tune_bytes(limit_packed=False), 4, plain) == 0
            assert lib.mapf_debug_rollout_plan_limited(lp.V, c.A, c.E, 64, streamed, 1, lp.N_CU, c.tune_bytes(), 4, keyed) == 0, lib.mapf_last_error()
            assert tuple(keyed) == tuple(plain) and keyed[0] == 2, (c.id, tuple(keyed), tuple(plain))


@pytest.mark.parametrize('case', lp.CASES, ids=lambda c: c.id)
def test_every_case_plans_the_instance_it_names(shim, case):
    """... with either table form; the limited plan is the unlimited one but for the limit mark; E + 1, half the batch and
    launches of more than 65535 steps are declined"""
    c = case
    for table_lds in lp.TABLE_LDS:
        tune = c.tune_bytes(table_lds)
        rc, limited, _ = _plan(shim, lp.V, c.A, c.E, tune, True)
        assert rc == 1, (c.id, table_lds)
        K, Q, form, block, image, total, lds, table_at, mark = limited
        assert (K, Q, form, block, lds, mark) == (c.K, c.Q, c.form, c.block, table_lds, 1), (c.id, limited)
        assert c.A == K * Q and c.E * Q == 1024 and total <= LDS and shim.shim_rollout_instance_exists(K, Q, form, 1) == 1
        rc, plain, _ = _plan(shim, lp.V, c.A, c.E, tune, False)
        assert rc == 1 and plain == limited[:8] + (0,), (c.id, plain, limited)
        # (without the key in the string the planner answers the same: the key is the dispatch's condition, not the planner's)
        assert _plan(shim, lp.V, c.A, c.E, c.tune_bytes(table_lds, limit_packed=False), True)[:2] == (1, limited)
        for E in (c.E + 1, c.E // 2):
            assert _plan(shim, lp.V, c.A, E, tune, True)[0] == 0, (c.id, E)
        assert _plan(shim, lp.V, c.A, c.E, tune, True, n_steps=65535)[0] == 1 and _plan(shim, lp.V, c.A, c.E, tune, True, n_steps=65536)[0] == 0
        assert _plan(shim, lp.V, c.A + 1, c.E, tune, True)[0] == 0                        # an odd team


def test_the_case_table_covers_every_table_instance_once(shim):
    assert shim.shim_table_instance_count(0) == 9 and shim.shim_table_instance_count(4) == 5 and shim.shim_table_instance_count(2) == 4
    assert len({(c.K, c.Q, c.form) for c in lp.CASES}) == len(lp.CASES) == 9
    assert all(shim.shim_rollout_instance_exists(c.K, c.Q, c.form, 1) for c in lp.CASES)


def test_whatever_is_planned_limited_is_a_table_instance_within_the_block_and_lds_bounds(shim):
    """the sweep of tests/test_plan_decisions.py's table group with the key set: a limited plan is the unlimited one, marked"""
    n_planned, forms = 0, set()
    for tune in TABLE_TUNES:
        keyed = (tune + b',' if tune else b'') + b'limit_packed=1'
        for A in TABLE_AGENTS:
            for mult in TABLE_BYTES:
                for delta in (0, 1):
                    for E in TABLE_ENVS:
                        for V in ROLLOUT_PLAN_CELLS:
                            rc, limited, key = _plan(shim, V, A, E, keyed, True, delta=delta, table_bytes=mult * V)
                            plain = _plan(shim, V, A, E, tune, False, delta=delta, table_bytes=mult * V)
                            ctx = (keyed, A, mult, delta, E, V, limited)
                            assert rc in (0, 1) and rc == plain[0] and key == 1, ctx
                            if not rc:
                                continue
                            n_planned += 1
                            K, Q, form, block, image, total, lds, table_at, mark = limited
                            forms.add(form)
                            assert mark == 1 and limited[:8] == plain[1][:8] and plain[1][8] == 0, ctx
                            assert shim.shim_rollout_instance_exists(K, Q, form, 1) == 1 and K in (2, 4), ctx
                            assert block <= 512 and E % (block // Q) == 0 and 1024 < image <= total <= LDS, ctx
    assert n_planned > 20000 and forms == {lp.FULL_ROWS, lp.DELTA_ROWS_BITMAP}, (n_planned, forms)


@pytest.fixture(scope='module')
def limit_listings():
    """the four gfx950 device listings of mapf_lq_limit.hip, as the Makefile compiles them (side by side): {(K, RECORD): text}"""
    names = {(K, record): 'mapf_lq_limit_k%d_r%d' % (K, record) for K in (4, 2) for record in (1, 0)}
    texts = device_listings.listings(*names.values())
    return {key: texts[name] for key, name in names.items()}


def test_the_limit_listings_hold_108_kernels_free_of_register_spills(limit_listings):
    total = 0
    for (K, record), text in limit_listings.items():
        kernels = kernel_meta.kernels(text)
        # per (K, Q, form) triple: {SOC, MAKESPAN, MAKESPAN NO_TERMINAL} x {TABLE_GLOBAL, TABLE_LDS}
        # (instances of the kernel template with the table policy's two arguments and the limit behind (args, A, bitmap_base), as the
        # mangled names spell the pack)
        limit_form = lambda name: 'lq_rollout_kernelI' in name and 'JNS_11TablePolicyEjNS_12EpisodeLimitEEE' in name
        assert len(kernels) == (30 if K == 4 else 24) and all(limit_form(k['name']) for k in kernels), (K, record, len(kernels))
        assert len({k['name'] for k in kernels}) == len(kernels)
        for k in kernels:
            assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0) and k['vgpr'] <= 256, k
        total += len(kernels)
    assert total == 108


@pytest.mark.parametrize('case', lp.CASES, ids=lambda c: c.id)
def test_the_reference_shows_every_outcome_for_every_case(case):
    """truncations and goal endings in the 36 reference steps of every (N, slip); collision endings too (32 agents under N = 1 need
    not show them); the variants of the terminal-handling test show what that test is about"""
    c = case
    for N, slip in ec.LIMITS:
        goals, colls, truncs, _ = lp.reference_counts(lp.workload(c.A, c.E, N), N, slip)
        assert truncs > 0 and goals > 0 and (colls > 0 or (c.A == 32 and N == 1)), (c.id, N, slip, goals, colls, truncs)
    if c in lp.TERMINAL_CASES:
        goals, colls, truncs, noops = lp.reference_counts(lp.workload(c.A, c.E, 4, True), 4, 0.2)
        assert noops >= ec.T_TOTAL * (c.E // 7) and truncs > 0 and goals > 0 and colls > 0, (c.id, goals, colls, truncs, noops)
        # without auto-reset: done envs stay terminal (no-ops), truncated envs live on
        goals, colls, truncs, noops = lp.reference_counts(lp.workload(c.A, c.E, 4), 4, 0.2, auto_reset=False)
        assert noops > 0 and truncs > 0 and goals > 0 and colls > 0, (c.id, goals, colls, truncs, noops)
