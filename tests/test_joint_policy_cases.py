"""CPU checks of tests/joint_policy_cases.py: joint_actions against a plain double loop over envs and agents, the random workload's
plans are valid and carry the partner geometries, and the merge family shows by the oracle alone what tests/test_gpu_joint_policy.py
relies on -- under the solo plan every episode ends in a collision of the pair (0, 1) and of no other, under the merged plan every
episode ends on the goals and nothing collides."""
import numpy as np
import pytest

import joint_policy_cases as jc
from gym_mapf_amd.envs import policies
from gym_mapf_amd.envs.vec_env import VecMapfEnv


def _loop_actions(table, offsets, partners, state, V):
    E, A = state.shape
    offsets, partners = np.asarray(offsets).reshape(-1, A), np.asarray(partners).reshape(-1, A)
    out = np.zeros((E, A), np.uint8)
    for e in range(E):
        off, part = offsets[e % offsets.shape[0]], partners[e % partners.shape[0]]
        for i in range(A):
            j = int(part[i])
            c = int(state[e, i])
            out[e, i] = table[int(off[i]) + c] if j == i else table[int(off[i]) + c * V + int(state[e, j])]
    return out


@pytest.mark.parametrize('A,E,broadcast', [(s[0], s[1], False) for s in jc.SHAPES] + [jc.BROADCAST_SHAPE + (True,)])
def test_joint_actions_is_the_definition_and_the_plans_are_valid(A, E, broadcast):
    for round in range(2 if broadcast else 1):
        w = jc.RandomJoint(A, E, broadcast=broadcast, round=round)
        rs = np.random.RandomState(A + E)
        for state in (w.start, rs.randint(0, w.V, size=(E, A))):
            assert np.array_equal(jc.joint_actions(w.table, w.offsets, w.partners, state, w.V), _loop_actions(w.table, w.offsets, w.partners, state, w.V))
        # what the library checks, by the Python twin of its validation; solo and merged agents both occur
        VecMapfEnv._joint_arguments(w.V, E, A, **w.plan())
        part = np.asarray(w.partners, np.int64).reshape(-1, A)
        merged = part != np.arange(A)[None, :]
        assert merged.any() and (A == 2 or (~merged).any())
        assert w.offsets.dtype == np.uint32 and w.partners.dtype == np.uint16 and w.offsets.shape == ((A,) if broadcast else (E, A))
        # the geometries: every list of geometries(A) stands in some env's matching
        for k, forced in enumerate(jc.geometries(A)):
            if not broadcast or k == round:
                assert any(all(row[i] == j and row[j] == i for i, j in forced) for row in part), (A, forced)
    pairs = [p for forced in jc.geometries(A) for p in forced]
    if A >= 3:
        assert any(j == i + 1 and i % 2 == 0 for i, j in pairs) and any(j == i + 1 and i % 2 == 1 for i, j in pairs) and (0, A - 1) in pairs


@pytest.mark.parametrize('A', jc.MERGE_AGENTS)
@pytest.mark.parametrize('W', jc.MERGE_WIDTHS)
def test_merging_the_pair_ends_its_conflicts_by_the_oracle_alone(W, A):
    w = jc.merge(W, A)
    n = jc.MERGE_EPISODES
    solo, M = w.evaluated('table')
    assert (solo['collisions'] == n).all() and not solo['goal_ends'].any() and not solo['truncations'].any()
    assert (solo['live_steps'] == 2 * n).all()                             # the pair meets on step 2
    rows = policies.conflicting_pairs(M)
    assert len(rows) == 1 and rows[0][:2] == (0, 1) and rows[0][2] + rows[0][3] == n * w.E
    assert (rows[0][2] == 0) == (W == 4)                                   # W = 5: vertex conflicts, W = 4: swaps
    merged, M = w.evaluated('joint')
    assert (merged['goal_ends'] == n).all() and not merged['collisions'].any() and not merged['truncations'].any() and not M.any()
    # with slip the runs are only compared with the device: but they still end n episodes per env
    slipped, _ = w.evaluated('joint', slip=0.2)
    assert ((slipped['goal_ends'] + slipped['collisions'] + slipped['truncations']) == n).all()


def test_the_merged_plan_of_the_family_is_a_joint_plan():
    w = jc.merge(5, 3)
    table, offsets, partners = w.joint
    assert partners.tolist() == [1, 0, 2] and table.size == 2 * w.V * w.V + w.V and offsets.tolist() == [0, w.V * w.V, 2 * w.V * w.V]
    VecMapfEnv._joint_arguments(w.V, w.E, w.A, table, offsets, partners)
