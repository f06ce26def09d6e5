"""CPU checks of the episode-limit tests' own reference and workload (tests/episode_limit_cases.py): the composition of the C
oracle shows every outcome the GPU tests rely on -- goal ends, collision ends, truncations, terminal-start no-ops -- so a seed
that stops providing one fails here and not on the GPU.  No device."""
import numpy as np
import pytest

import episode_limit_cases as ec

# slip 0.2, N = 4, the table-driven sources: (A, E) -> (goal ends, collision ends, truncations) of the 36 steps
EXPECTED_N4 = {(3, 37): (528, 7, 82), (8, 64): (381, 162, 243), (16, 64): (144, 555, 233), (32, 64): (15, 1805, 36), (2, 37): (560, 2, 50)}


@pytest.mark.parametrize('A,E', sorted(EXPECTED_N4))
def test_reference_counts_at_limit_four_with_slip(A, E):
    w = ec.Workload(A, E, 4)
    assert w.nbr.shape[0] == 341
    for source in ('table', 'stream'):
        refs = w.oracle(4, 0.2).run(w, source, ec.T_TOTAL)
        counts = ec.outcome_counts(refs)
        assert counts[:3] == EXPECTED_N4[(A, E)], (source, counts)
        ec.check_outcomes(A, E, 4, 0.2, source, counts)
    if A == 2:                                                    # rule 1: steps from a terminal state (two starts on the goals)
        assert counts[3] == 108


def test_reference_counts_at_limit_one_and_without_slip():
    w = ec.Workload(8, 64, 1)
    assert ec.outcome_counts(w.oracle(1, 0.2).run(w, 'table', ec.T_TOTAL))[:3] == (176, 214, 1914)
    w = ec.Workload(8, 64, 4)
    assert ec.outcome_counts(w.oracle(4, 0.0).run(w, 'table', ec.T_TOTAL))[2] == 0     # every goal is at most three moves away
    w = ec.Workload(8, 64, 2)
    assert ec.outcome_counts(w.oracle(2, 0.0).run(w, 'table', ec.T_TOTAL))[2] > 0


@pytest.mark.parametrize('A,E', ec.SHAPES)
def test_every_pass_of_the_gpu_tests_shows_its_outcomes(A, E):
    seen = np.zeros(3, np.int64)
    for N, slip in ec.LIMITS:
        w = ec.Workload(A, E, N)
        for source in ec.SOURCES:
            counts = ec.outcome_counts(w.oracle(N, slip).run(w, source, ec.T_TOTAL))
            ec.check_outcomes(A, E, N, slip, source, counts)
            seen += counts[:3]
    assert seen[0] > 0 and seen[2] > 0 and (seen[1] > 0 or A == 2)     # (the passes ec.WITHOUT excuses: another pass of the shape shows it)


def test_the_composition_follows_the_definition():
    """a limit never reached is the plain oracle; without auto-reset a truncated env stays truncated on every later live step; the
    age saturates; reset(mask) zeroes the masked ages only"""
    w = ec.Workload(3, 37, 4)
    plain, far = w.oracle(0, 0.2), w.oracle(1 << 31, 0.2)
    for a, b in zip(plain.run(w, 'table', 20), far.run(w, 'table', 20)):
        assert all(np.array_equal(a[k], b[k]) for k in a) and not b['truncated'].any()
    assert np.array_equal(plain.co.state, far.co.state) and not plain.age.any()
    ref = w.oracle(3, 0.2)
    seen = np.zeros(w.E, bool)
    for r in ref.run(w, 'table', 8, auto_reset=False):
        live = r['was_terminal'] == 0
        assert (r['truncated'][seen & live & (r['done'] == 0)] == 1).all()
        seen |= r['truncated'] != 0
    assert seen.any() and (ref.age[seen] >= 3).all()
    mask = (np.arange(w.E) % 2).astype(np.uint8)
    before = ref.age.copy()
    ref.reset(mask)
    assert not ref.age[mask != 0].any() and np.array_equal(ref.age[mask == 0], before[mask == 0])
    ref.age[:] = ec.AGE_MAX
    ref.step(w.actions('table', ref), auto_reset=False)
    assert (ref.age == ec.AGE_MAX).all()
