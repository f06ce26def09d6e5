"""The host-built tables (csrc/mapf_tables.hip) and the single step's launch plan (csrc/mapf_plan.hip), checked without a
GPU: the two host-only units are compiled with a small C shim (tests/host_tables_shim.hip) into the test's tmp dir and driven
through ctypes.  The move table is compared with the movement lists the reference wrote into tests/golden/*.npz, the slip and
outcome rows with the rules re-stated here in Python (exact integer / Fraction arithmetic for the thresholds)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from gym_mapf_amd.envs.grid import MapfGrid
import mapf_oracle as mo
from host_shim import OUTCOME, SLIP, move_tables, sizes, slip_rows, step_instances
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import STEP_PLAN_AGENTS, STEP_PLAN_CELLS, STEP_PLAN_CUS, STEP_PLAN_ENVS, STEP_PLAN_TUNES

LDS = 160 * 1024


def _decode16(mv, slip):
    """(n, cells, q) of every 16-byte row -- int64[V, cols], int64[V, cols, 3], float64[V, cols, 3] -- after checking the
    words a row repeats from its code's slip row."""
    x, y, z, w = (mv[..., i].astype(np.int64) for i in range(4))
    code = (y >> 16) & 7
    cells = np.stack([x & 0xFFFF, x >> 16, y & 0xFFFF], axis=-1)
    assert np.array_equal(w, code * SLIP.itemsize)
    assert np.array_equal(y >> 19, slip['members'][code])
    assert np.array_equal(z, slip['th'][code][..., 0].astype(np.int64) | (slip['th'][code][..., 1].astype(np.int64) << 16))
    return slip['n'][code].astype(np.int64), cells, slip['q'][code]


def _same_lists(n, cells, q, exp_n, exp_cells, exp_q):
    assert np.array_equal(n, np.asarray(exp_n, np.int64))
    valid = np.arange(3)[None, None, :] < n[..., None]
    assert np.array_equal(cells[valid], np.asarray(exp_cells, np.int64)[valid])
    assert np.array_equal(np.ascontiguousarray(q).view(np.uint64)[valid], np.ascontiguousarray(exp_q, np.float64).view(np.uint64)[valid])


def test_move_table_rows_are_the_reference_movement_lists(shim, trajectory_set):
    meta, g = trajectory_set
    nbr = MapfGrid(meta['lines']).tables()[2]                     # as the product builds it
    V = len(nbr)
    assert nbr.shape == (V, 5) and V == len(g['valid_locations'])
    for fail_prob in (meta['fail_prob'], 0.0, 1.0):
        slip, _, _ = slip_rows(shim, fail_prob)
        mv, mv8, mv4 = move_tables(shim, nbr, fail_prob)
        n, cells, q = _decode16(mv, slip)
        if fail_prob == meta['fail_prob']:                        # the lists the reference wrote
            _same_lists(n[:, :5], cells[:, :5], q[:, :5], g['mv_n'], g['mv_next'], g['mv_prob'])
        if fail_prob != meta['fail_prob'] or V <= 4096:           # (tests/test_oracle_golden.py pins slip_distribution to the same goldens)
            exp_n, exp_cells, exp_q = np.zeros((V, 5), np.int64), np.zeros((V, 5, 3), np.int64), np.zeros((V, 5, 3))
            for v, row in enumerate(nbr.tolist()):
                for a in range(5):
                    dist = mo.slip_distribution(row, a, fail_prob)
                    exp_n[v, a] = len(dist)
                    for k, (c, p) in enumerate(dist):
                        exp_cells[v, a, k], exp_q[v, a, k] = c, p
            assert exp_n.max() <= (1 if fail_prob == 0.0 else (2 if fail_prob == 1.0 else 3))   # empty / zero-probability candidates are dropped
            _same_lists(n[:, :5], cells[:, :5], q[:, :5], exp_n, exp_cells, exp_q)
        if mv.shape[1] == 6:                                      # (experiment builds: column 5 = STAY again)
            assert np.array_equal(mv[:, 5], mv[:, 0])
        # the 8-byte rows: the same cells, the slip row's byte offset in the upper half of y
        assert np.array_equal(mv8[..., 0], mv[..., 0])
        assert np.array_equal(mv8[..., 1] & 0xFFFF, mv[..., 1] & 0xFFFF) and np.array_equal(mv8[..., 1] >> 16, mv[..., 3])
        # the 4-byte delta rows exist exactly when every neighbour id is within +-127 of its cell's id
        near = bool((np.abs(nbr.astype(np.int64) - np.arange(V)[:, None]) <= 127).all())
        assert (mv4 is not None) == near
        if meta['name'].startswith('berlin256'):                    # (ids run down 256-row columns: a false case)
            assert not near
        if mv4 is not None:
            mv_cols, delta_cols, row_bias, delta_words = sizes(shim, V)
            assert delta_words % 4 == 0 and 0 <= delta_words - V * delta_cols < 4 and not mv4[V * delta_cols:].any()
            rows4 = mv4[:V * delta_cols].reshape(V, delta_cols)
            own = np.arange(V, dtype=np.int64)[:, None]
            for col in range(delta_cols):
                src = col if col < mv.shape[1] else 0             # column 5 = STAY again
                valid = np.arange(3)[None, :] < n[:, src, None]
                deltas = np.stack([(rows4[:, col] >> (8 * k)) & 0xFF for k in range(3)], axis=-1).astype(np.uint8).view(np.int8).astype(np.int64)
                assert np.array_equal((own + deltas)[valid], cells[:, src][valid])
                assert np.array_equal((rows4[:, col] >> 24).astype(np.int64) * 8 - row_bias, mv[:, src, 3].astype(np.int64))


def _expected_slip_row(code, p):
    """single_agent_movements for the equality pattern `code` of the candidates (m, r, l), in Python floats: drop p <= 0, merge
    equal cells in first-seen order with old + new; cumsum left to right."""
    m, r = 0, (0 if code & 1 else 1)
    cand_cells = (m, r, 0 if code & 2 else (r if code & 4 else 2))
    cells, q, members = [], [], []
    for k in range(3):
        if not p[k] > 0:
            continue
        if cand_cells[k] in cells:
            j = cells.index(cand_cells[k])
            q[j] = q[j] + p[k]
            members[j] |= 1 << k
        else:
            cells.append(cand_cells[k]); q.append(p[k]); members.append(1 << k)
    cum, run = [], 0.0
    for k, x in enumerate(q):
        run = x if k == 0 else run + x
        cum.append(run)
    return q, cum, members


@pytest.mark.parametrize('fail_prob', [0.0, 0.05, 0.1, 0.2, 0.3, 1.0 / 3.0, 0.5, 0.7, 0.999, 1.0])
def test_slip_rows_thresholds_and_members(shim, fail_prob):
    rows, p_cand, flags = slip_rows(shim, fail_prob)
    rf = lf = fail_prob / 2
    p = [1 - rf - lf, rf, lf]                                      # mapf_env.py:131-132, :167
    assert p_cand.tobytes() == np.asarray(p).tobytes()
    any_multi = top_tie = False
    for code in range(8):
        row = rows[code]
        q, cum, members = _expected_slip_row(code, p)
        n = len(q)
        assert int(row['n']) == n and 1 <= n <= 3
        assert row['q'][:n].tobytes() == np.asarray(q).tobytes() and not row['q'][n:].any()
        assert row['cum'][:n].tobytes() == np.asarray(cum).tobytes() and np.all(np.isneginf(row['cum'][n:]))
        thr = [min(math.ceil(Fraction(c) * 2 ** 53), 2 ** 53) for c in cum]                   # exact: cum > u  <=>  mant(u) < thr
        assert [int(t) for t in row['thr']] == thr + [0] * (3 - n)
        th = [min(t >> 37, 65535) for t in thr] + [65535] * (3 - n)
        assert int(row['th'][0]) == th[0] and int(row['th'][1]) == th[1]
        assert int(row['th'][2]) == th[0] | (th[1] << 16) and int(row['th_biased']) == (th[0] | (th[1] << 16)) ^ 0x80008000
        assert int(row['members']) == sum(mem << (3 * k) for k, mem in enumerate(members))
        any_multi |= n > 1
        top_tie |= n == 3 and thr[2] < 2 ** 53
    assert (int(flags[0]), int(flags[1])) == (int(any_multi), int(top_tie))


def _outcome_status(f):
    """done | collision << 8 | next_terminal << 16 from f = vertex | swap << 1 | off_goal_next << 2 (mapf_env.py:210-235)"""
    vertex, coll, goal_next = bool(f & 1), bool(f & 3), not f & 4
    return int(coll or goal_next) | (0x100 if coll else 0) | (0x10000 if vertex or goal_next else 0)


@pytest.mark.parametrize('rewards', [(-1000.0, 100.0, -1.0), (-0.1, 0.3, -0.7), (0.0, 0.0, 0.0)])
def test_outcome_rows(shim, rewards):
    r_clash, r_goal, r_living = rewards
    rows = np.zeros(16, OUTCOME)
    shim.shim_outcome_rows(r_clash, r_goal, r_living, rows.ctypes.data)
    for i in range(16):
        st = _outcome_status(i & 7)
        assert shim.shim_outcome_status(i & 7) == st
        reward = r_clash + r_living if st & 0x100 else (r_goal + r_living if st & 1 else r_living)
        status = st if i < 8 else 0x10001
        assert np.float64(rows[i]['reward']).tobytes() == np.float64(reward if i < 8 else 0.0).tobytes(), i
        assert int(rows[i]['status']) == status and int(rows[i]['pad']) == (status & 1) | ((status & 0x100) << 8), i


def _scen(lib, start, goal, E, A, sb=False, gb=False):
    scen, rows = np.full(E, 255, np.uint8), np.zeros(256 * 2 * A, np.uint16)
    n = lib.shim_scen_table(start.ctypes.data, int(sb), goal.ctypes.data, int(gb), E, A, scen.ctypes.data, rows.ctypes.data)
    assert n <= 256
    return n, scen, rows.reshape(256 * 2, A)


def test_scenario_table_round_trips(shim):
    rng = np.random.default_rng(3)
    E, A = 1000, 3
    for n_pairs in (1, 6, 256):
        pairs = rng.permutation(5000)[:n_pairs * 2 * A].astype(np.uint16).reshape(n_pairs, 2, A)     # distinct rows
        pick = np.concatenate([np.arange(n_pairs), rng.integers(0, n_pairs, E - n_pairs)]) if n_pairs <= E else None
        start, goal = np.ascontiguousarray(pairs[pick, 0]), np.ascontiguousarray(pairs[pick, 1])
        n, scen, rows = _scen(shim, start, goal, E, A)
        assert n == n_pairs and scen.max() == n_pairs - 1
        assert np.array_equal(rows[2 * scen.astype(np.int64)], start) and np.array_equal(rows[2 * scen.astype(np.int64) + 1], goal)
        # broadcast starts: every pair's start row is THE start row
        n, scen, rows = _scen(shim, start[:1].copy(), goal, E, A, sb=True)
        assert n == n_pairs and np.array_equal(rows[2 * scen.astype(np.int64)], np.repeat(start[:1], E, 0))
        assert np.array_equal(rows[2 * scen.astype(np.int64) + 1], goal)
    # more than 256 distinct pairs: no table
    start = np.arange(E * A, dtype=np.uint16).reshape(E, A)
    assert _scen(shim, start, start.copy(), E, A)[0] == 0
    start[257:] = start[0]
    assert _scen(shim, start, start.copy(), E, A)[0] == 0                                        # 257 pairs
    start[256:] = start[0]
    assert _scen(shim, start, start.copy(), E, A)[0] == 256


def test_greedy_policy_cells(shim):
    lines = ['..@...', '.@..@.', '......', '@..@..', '...@.@']
    valid, _, nbr = MapfGrid(lines).tables()
    V = len(valid)
    rc = np.asarray(valid, np.int64)
    cell_rc = (rc[:, 0] | (rc[:, 1] << 16)).astype(np.uint32)
    cells = np.zeros((V, 2), np.uint32)
    err = ctypes.create_string_buffer(256)
    assert shim.shim_greedy_cells(nbr.ctypes.data, V, cell_rc.ctypes.data, cells.ctypes.data, err, 256) == 1
    n_moves = 0
    for v in range(V):
        best = 0
        for sr in (-1, 0, 1):
            for sc in (-1, 0, 1):
                # the first action in ACTIONS order that is not blocked and lands one step closer in row or in column
                pick = 0
                for a in range(1, 5):
                    tgt = int(nbr[v, a])
                    dr, dc = rc[tgt, 0] - rc[v, 0], rc[tgt, 1] - rc[v, 1]
                    if tgt != v and ((dr != 0 and dr == sr) or (dc != 0 and dc == sc)):
                        pick = a
                        break
                n_moves += pick != 0
                best |= pick << (3 * (3 * (sr + 1) + (sc + 1)))
        assert (int(cells[v, 0]), int(cells[v, 1])) == (int(cell_rc[v]), best), v
    assert n_moves > V
    wrong = cell_rc.copy()
    wrong[[0, V - 1]] = wrong[[V - 1, 0]]
    assert shim.shim_greedy_cells(nbr.ctypes.data, V, wrong.ctypes.data, cells.ctypes.data, err, 256) == 0
    assert b'cell_rc does not match the neighbour table' in err.value


def test_packed_step_plan_stays_within_the_lds_and_its_residency(shim):
    """plan_step_lq swept like the rollout plan (tests/test_cabi_and_host.py): whatever instance is planned exists, fills whole
    blocks, keeps its LDS image within the CU's 160 KB (and within the limit the launcher raises the kernel to), and its
    resident grid within what the LDS image and 2048 threads per CU allow."""
    out = np.zeros(8, np.uint64)
    stride = lambda V: (((V + 31) // 32) * 4 + 15) & ~15                                   # noqa: E731  (bytes of one env's bitmap)
    cells, tunes = STEP_PLAN_CELLS, STEP_PLAN_TUNES
    instances = step_instances(shim)
    assert len(instances) == 21, sorted(instances)
    seen, n_planned = set(), 0
    for tune in tunes:
        for n_cu in STEP_PLAN_CUS:
            for A in STEP_PLAN_AGENTS:
                for E in STEP_PLAN_ENVS:
                    for delta in (0, 1):
                        for V in cells:
                            rc = shim.shim_plan_step(V, A, E, delta, n_cu, tune, out.ctypes.data)
                            assert rc in (0, 1), (rc, tune)
                            if not rc:
                                continue
                            K, Q, big, block, grid, n_chunks, lds, limit = (int(x) for x in out)
                            ctx = (tune, n_cu, A, E, delta, V, K, Q, big, block, grid, n_chunks, lds, limit)
                            n_planned += 1
                            seen.add((Q, K, big))
                            assert (Q, K, big) in instances and K * Q == A and tune != b'quad_lanes=0', ctx
                            assert block in (64, 128, 256, 512, 1024) and block % Q == 0 and E % (block // Q) == 0 and E > 0, ctx
                            assert n_chunks * block == E * Q and 1 <= grid <= n_chunks, ctx                 # whole blocks
                            if big == 0:
                                assert block <= 512 and grid == n_chunks and lds == 0, ctx                   # launch bounds 512, static image
                                continue
                            table = 1024 + (V * 6 * 16 if big == 1 else ((V * 6 + 3) & ~3) * 4)
                            assert lds == table + ((block // 8) * stride(V) if big == 3 else 0), ctx
                            assert 1024 < lds <= LDS and (lds <= 32 * 1024 or lds <= limit <= LDS), ctx
                            assert big == 1 or delta, ctx
                            assert grid <= min(LDS // lds, 2048 // block) * n_cu, ctx                        # the residency the plan states
                            if big == 1:
                                assert 2 * lds <= LDS and block == 1024 and grid <= (1 if K == 8 else 2) * n_cu, ctx
    assert seen == instances and n_planned > 50000, (sorted(instances - seen), n_planned)
    assert shim.shim_plan_step(683, 8, 65536, 0, 256, b'step_big=two', out.ctypes.data) == -1
