"""The reference of the episode log (tests/episode_log_cases.py) alone shows what the GPU tests rely on, over the table source: partial
episodes that cross a launch boundary, every outcome, zero-length records, logs that overflow and logs that do not fill, and record
returns whose sum is NOT the totals' return bit for bit.  No GPU, no library call."""
import numpy as np
import pytest

import episode_budget_cases as bc
import episode_limit_cases as ec
import episode_log_cases as lc

_RUNS = {}


def _run(A, E, N, slip, B, C):
    """the four launches of a pass under the table source, computed once: (reference, per-launch steps, partial lengths after launch 1)"""
    key = (A, E, N, slip, B, C)
    if key not in _RUNS:
        w = ec.Workload(A, E, N or 4)
        ref = lc.oracle(w, N, slip, B, C)
        launches, carried = [], None
        for n in ec.LAUNCHES:
            launches.append(ref.run(w, 'table', n))
            if carried is None:
                carried = ref.len.copy()
        _RUNS[key] = (ref, launches, carried)
    return _RUNS[key]


@pytest.mark.parametrize('A,E', bc.SHAPES)
def test_partial_episodes_cross_the_first_launch_boundary_and_every_outcome_appears(A, E):
    seen = {}
    for N, slip, B in bc.PASSES:
        ref, _, carried = _run(A, E, N, slip, B, B)
        assert int((carried > 0).sum()) >= 4, (A, E, N, slip, B, int((carried > 0).sum()))
        got = ref.records['outcome'][lc.stored(ref)]
        assert set(np.unique(got)) <= {lc.GOAL, lc.COLLISION, lc.TRUNCATED}
        seen[(N, slip, B)] = set(int(x) for x in np.unique(got))
        # a record's length is what its steps say: never beyond the limit, zero only for a terminal start's no-op (outcome 1)
        rec = ref.records[lc.stored(ref)]
        assert (rec['steps'] <= (N or ec.T_TOTAL)).all() and (rec['outcome'][rec['steps'] == 0] == lc.GOAL).all()
        assert (rec['steps'][rec['outcome'] == lc.TRUNCATED] == N).all()
    assert set().union(*seen.values()) == {lc.GOAL, lc.COLLISION, lc.TRUNCATED}, (A, E, seen)
    if A == 2:
        assert [p for p, s in seen.items() if lc.COLLISION in s] == [(4, 0.2, 10)], seen


def test_two_agents_log_zero_length_records():
    hits = 0
    for N, slip, B in bc.PASSES:
        ref, _, _ = _run(2, 37, N, slip, B, B)
        rec = ref.records[lc.stored(ref)]
        zero = rec[rec['steps'] == 0]
        hits += len(zero)
        assert (zero['outcome'] == lc.GOAL).all() and (zero['ret'].view(np.uint64) == 0).all()      # {+0.0, 0, 1}
    assert hits > 0


@pytest.mark.parametrize('A,E', bc.SHAPES)
def test_a_small_log_overflows_everywhere_and_a_large_one_does_not_fill(A, E):
    for N, slip, B in bc.PASSES:
        if B != 3:
            continue
        ref, _, _ = _run(A, E, N, slip, B, 2)
        assert (ref.count == 3).all() and (ref.left == 0).all(), (A, E, N, slip)
        whole, _, _ = _run(A, E, N, slip, B, B)
        assert np.array_equal(ref.records, whole.records[:, :2])                # the first C records, whatever follows
    ref, _, _ = _run(A, E, 4, 0.2, 10, 10)
    if A in (2, 3, 8, 16):
        assert (ref.count < 10).any(), (A, E, ref.count.min())
    assert (ref.count <= 10).all() and np.array_equal(ref.count, 10 - ref.left)
    assert (ref.records['outcome'][~lc.stored(ref)] == 0).all()                 # the slots from count on stay zero


def test_record_returns_do_not_sum_to_the_totals_bit_for_bit():
    """different association, INEXACT rewards: the log is compared with its own reference, never with the totals"""
    differing = 0
    for A, E in bc.SHAPES:
        ref, launches, _ = _run(A, E, 4, 0.2, 3, 3)
        totals = bc.totals_of([r for refs in launches for r in refs])
        assert (ref.left == 0).all() and (ref.acc.view(np.uint64) == 0).all() and not ref.len.any()
        summed = np.zeros(E)
        for k in range(3):
            summed = summed + ref.records['ret'][:, k]
        assert np.allclose(summed, totals['returns'], rtol=0, atol=1e-12)
        differing += int((summed.view(np.uint64) != totals['returns'].view(np.uint64)).sum())
        # the integers do agree: lengths with the live steps, outcomes with the three counts
        assert np.array_equal(ref.records['steps'].sum(axis=1), totals['live_steps'])
        assert np.array_equal((ref.records['outcome'] == lc.COLLISION).sum(axis=1), totals['collisions'])
        assert np.array_equal((ref.records['outcome'] == lc.TRUNCATED).sum(axis=1), totals['truncations'])
        assert np.array_equal((ref.records['outcome'] != lc.TRUNCATED).sum(axis=1), totals['episodes'])
    assert differing > 0
