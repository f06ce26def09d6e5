"""CPU: the reference of the conflict-matrix tests (tests/conflict_pairs_cases.py) alone shows what the GPU tests rely on -- the
scripted family meets every agent pair exactly once as a vertex conflict and once as a swap, and the random budget workload shows
vertex conflicts, swaps, steps with several conflicting pairs and three agents on one cell.  Presence is asserted, not the counts: a
seed that stops providing one fails here and not on the GPU.  (At 8 agents the pass (4, 0.2, 10) under `table` shows 78 vertex and 22
swap counts and 3 multi-pair steps; at 32 agents 885, 151 and 295, and 16 steps with three agents on one cell.)"""
import numpy as np
import pytest

import conflict_pairs_cases as pc
import episode_budget_cases as bc
import episode_limit_cases as ec


@pytest.mark.parametrize('A', pc.EVERY_PAIR_AGENTS)
def test_every_pair_meets_every_pair_once_as_vertex_and_once_as_swap(A):
    w = pc.every_pair(A)
    assert w.E == A * (A - 1) and len(w.pairs) * 2 == w.E
    ref = w.oracle()
    r = ref.step(w.actions1, auto_reset=True)
    # every env is live, collides, and shows exactly one pair: its own, of its own kind
    assert not r['was_terminal'].any() and r['collision'].all() and r['done'].all()
    per_env = pc.pair_counts(r['prev'], r['local']) if A <= 40 else None
    if per_env is not None:
        assert (per_env.sum(axis=(1, 2)) == 1).all()
        for p, (i, j) in enumerate(w.pairs):
            assert per_env[2 * p, i, j] == 1 and per_env[2 * p + 1, j, i] == 1, (i, j)
    assert np.array_equal(ref.M, w.expected())
    # slots e % 2: the vertex envs fill slot 0's upper triangle, the swap envs slot 1's lower one
    ref = w.oracle(2, np.arange(w.E) % 2)
    ref.step(w.actions1, auto_reset=True)
    upper = np.triu(np.ones((A, A), np.uint64), 1)
    assert np.array_equal(ref.M[0], upper) and np.array_equal(ref.M[1], upper.T)


@pytest.mark.parametrize('A,E', pc.SHAPES)
def test_the_budget_workload_shows_vertex_conflicts_swaps_and_multi_pair_steps(A, E):
    for N, slip, B in bc.PASSES:
        w = ec.Workload(A, E, N or 4)
        triples = 0
        for source in ('table', 'policy'):
            ref = pc.PairsOracle(bc.oracle(w, N, slip, B))
            refs = [r for n in ec.LAUNCHES for r in ref.run(w, source, n)]
            vertex, swap, multi, triple = pc.pair_facts(refs)
            tag = (A, E, N, slip, B, source, vertex, swap, multi, triple)
            assert int(np.triu(ref.M[0], 1).sum()) == vertex and int(np.tril(ref.M[0], -1).sum()) == swap, tag
            assert not np.diagonal(ref.M[0]).any(), tag
            # a live step reports collision exactly when it adds at least one count
            for r in refs:
                rows = np.flatnonzero(r['counted'])
                hit = pc.pair_counts(r['prev'][rows], r['local'][rows]).any(axis=(1, 2))
                assert np.array_equal(hit, r['collision'][rows] != 0), tag
                assert not r['collision'][~r['counted']].any(), tag
            if A >= 5:
                assert vertex > 0 and swap > 0, tag
            if A >= 16:
                assert multi > 0, tag
            triples += triple
        # three agents on one cell: in every pass (N, slip, B), its two sources taken together -- 32 agents under the random
        # stream in the pass without slip show none on their own (with 64 envs: table 3, policy 0)
        if A >= 32:
            assert triples > 0, (A, E, N, slip, B, triples)
