"""CPU checks of the episode-budget tests' own reference and workload (tests/episode_budget_cases.py): the composition over the C
oracle shows every outcome the GPU tests rely on -- envs that park by goal end, by collision end, by truncation and by terminal-start
no-ops, parks in the first launch, in the one-step second launch and later, envs still running at the end -- so a seed that stops
providing one fails here and not on the GPU.  No device."""
import numpy as np
import pytest

import episode_budget_cases as bc
import episode_limit_cases as ec


def _pass(A, E, N, slip, B, source='table'):
    w = ec.Workload(A, E, N or 4)
    ref = bc.oracle(w, N, slip, B)
    launches = bc.run_launches(ref, w, source)
    return w, ref, launches


@pytest.mark.parametrize('A,E', bc.SHAPES)
def test_every_shape_shows_every_outcome_over_its_passes(A, E):
    kinds_seen, running_seen, differs = np.zeros(4, np.int64), 0, False
    for N, slip, B in bc.PASSES:
        w, ref, launches = _pass(A, E, N, slip, B)
        refs = [r for l in launches for r in l]
        per_launch, kinds = bc.park_counts(launches)
        tot = bc.totals_of(refs)
        # the invariant: B - left == episodes + truncations, and a parked env has spent exactly B
        assert np.array_equal(B - ref.left.astype(np.int64), tot['episodes'].astype(np.int64) + tot['truncations']), (A, E, N, slip, B)
        assert sum(per_launch) == int((ref.left == 0).sum()) == sum(kinds)
        assert (tot['live_steps'] <= ec.T_TOTAL).all() and tot['live_steps'].any()
        if N == 0:
            assert not tot['truncations'].any() and not ref.age.any() and (ref.left == 0).all()     # a budget without a limit parks every env
        if B == 3:
            assert (ref.left == 0).all(), (A, E, N, slip)                                           # every env parks under B = 3
        if (N, slip, B) == (4, 0.2, 3):
            assert all(n > 0 for n in per_launch[:3]), (A, E, per_launch)                           # the first, the one-step second, a later launch
        kinds_seen += kinds
        running_seen += int((ref.left != 0).sum())
        # the budget matters: some env's returns differ from those of the same 36 steps without a budget
        plain = w.oracle(N, slip)
        want = ec.totals_of(plain.run(w, 'table', ec.T_TOTAL))
        differs = differs or bool((want['returns'] != tot['returns']).any())
        # parked rows are recognisable, and they are the only ones
        for r in refs:
            assert np.array_equal((r['done'] == 0) & (r['prob'] == 0), r['parked']), (A, E, N, slip, B)
    goal, coll, trunc, noop = kinds_seen
    assert goal > 0 and trunc > 0 and (coll > 0 or A == 2), (A, E, kinds_seen)
    assert running_seen > 0 or A == 32, (A, E)          # (32 agents: every team collides early, all ten episodes fit into the 36 steps)
    assert differs
    if A == 2:
        assert noop > 0                                 # rule 1: two starts stand on their goals


def test_reference_counts_of_the_eight_agent_passes():
    """pinned so that a change of the workload shows here: parks per launch and by kind; envs running at the end"""
    _, ref, launches = _pass(8, 64, 4, 0.2, 3)
    per_launch, kinds = bc.park_counts(launches)
    assert (per_launch[0], per_launch[1], sum(per_launch[2:])) == (7, 9, 48) and kinds == (32, 11, 21, 0)
    _, ref, _ = _pass(8, 64, 4, 0.2, 10)
    assert int((ref.left != 0).sum()) == 17
    _, ref, _ = _pass(16, 37, 4, 0.2, 10)
    assert int((ref.left != 0).sum()) == 13
    _, ref, launches = _pass(2, 37, 4, 0.2, 3)
    assert bc.park_counts(launches)[1][3] == 3          # three envs park by terminal-start no-ops


def test_the_composition_follows_the_definition():
    """a parked env keeps cells, age and count and adds nothing (an accumulated -0.0 stays); a budget never reached is the limit
    oracle; re-arming starts a fresh batch of episodes from the start cells"""
    w = ec.Workload(3, 37, 4)
    far, lim = bc.oracle(w, 4, 0.2, 1 << 31), w.oracle(4, 0.2)
    for a, b in zip(far.run(w, 'table', 20), lim.run(w, 'table', 20)):
        assert all(np.array_equal(a[k], b[k]) for k in b) and not a['parked'].any()
    assert np.array_equal(far.co.state, lim.co.state) and np.array_equal(far.age, lim.age)
    ref = bc.oracle(w, 4, 0.2, 1)
    ref.run(w, 'table', 8)
    assert (ref.left == 0).all() and np.array_equal(ref.co.state, w.start) and not ref.age.any()
    t = ref.co.t
    refs = ref.run(w, 'table', 3)
    assert ref.co.t == t + 3 and np.array_equal(ref.co.state, w.start)
    base = {k: (np.full(w.E, -0.0) if k == 'returns' else np.zeros(w.E, np.uint32)) for k in bc.TOTALS}
    tot = bc.totals_of(refs, base)
    assert np.signbit(tot['returns']).all() and not any(tot[k].any() for k in bc.TOTALS[1:])
    ref.set_budget(2)
    assert (ref.left == 2).all()
    tot = bc.totals_of(ref.run(w, 'table', 12))
    assert (ref.left == 0).all() and np.array_equal(tot['episodes'] + tot['truncations'], np.full(w.E, 2, np.uint32))
