"""CPU-side checks of the joint table policy (include/mapf_hip.h MAPF_POLICY_JOINT, mapf_set_policy_joint): the entry point validates
its arguments before a handle is touched, header / library / ctypes table agree on it, the ABI and mapf_rollout_io are what they
were, the six new compilations are in the Makefile's third table (the first two are what they were) and hold exactly the declared
instances without register spills or scratch, the units that count conflicting pairs without the mode compile to the listings the
commit before it gave them, the route and the names of launches without the mode are what they were, and the host helpers of
envs/policies.py and the argument checks of VecMapfEnv.set_policy('joint') do what they say.  No compute is launched here.  (What
needs a live handle -- an asymmetric partner map, a segment past the table, a byte 5, graph_begin -- is refused on the GPU in
tests/test_gpu_joint_policy.py.)"""
import ctypes
import hashlib
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import joint_policy_cases as jc
from conftest import ROOT
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import ACTIONS, policies
from gym_mapf_amd.envs.grid import MapfGrid
from gym_mapf_amd.envs.vec_env import VecMapfEnv
from host_shim import CSRC, device_listings, kernel_meta
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import AUTO, LG, PACKED, routed_rollout

HEADER = os.path.join(ROOT, 'include', 'mapf_hip.h')
SOURCE = '../csrc_joint/mapf_lg_joint'
LIMIT, BUDGET, PAIRS = 'NS_12EpisodeLimitE', 'NS_13EpisodeBudgetE', 'NS_13ConflictPairsE'
# the mangled argument packs behind (args, A) of each new compilation
PACKS = {'mapf_lg_joint_plain': '', 'mapf_lg_joint_limit': LIMIT, 'mapf_lg_joint_budget': LIMIT + BUDGET,
         'mapf_lg_joint_pairs_plain': PAIRS, 'mapf_lg_joint_pairs_limit': LIMIT + PAIRS, 'mapf_lg_joint_pairs_budget': LIMIT + BUDGET + PAIRS}
NEW_UNITS = tuple(PACKS)
ADDED_UNITS = ('mapf_lg_pairs_plain', 'mapf_lg_pairs_limit', 'mapf_lg_pairs_budget')
# sha256 of the device listings (hipcc -S --cuda-device-only, __hip_cuid_* masked) of the units that count conflicting pairs, as the
# commit before the joint table policy compiles them: the units keep their code
PARENT_LISTINGS = {
    'mapf_lg_pairs_plain': 'af52dc0777cde2f3f87581c299ce26db984767593677328ab176d3a19ed926a5',
    'mapf_lg_pairs_limit': '068df96603e3fff28dcffde535d76f63f3ce964c9324d120b5e882853e3e2264',
    'mapf_lg_pairs_budget': 'dffaa8e31a69335b91517b968194a9b8373348671401fba0dbe0bc979694542b',
}


def test_the_new_entry_point_validates_its_arguments_without_a_device():
    lib = nat.load()
    table, offset, partner = np.zeros(16, np.uint8), np.zeros(4, np.uint32), np.zeros(4, np.uint16)
    t, o, p = table.ctypes.data, offset.ctypes.data, partner.ctypes.data
    assert lib.mapf_set_policy_joint(None, t, 16, o, p, 0) == nat.MAPF_EINVAL and b'set_policy_joint: null handle' in lib.mapf_last_error()
    fake = ctypes.c_void_p(1)                   # (never dereferenced: the pointers are looked at first)
    assert lib.mapf_set_policy_joint(fake, None, 16, o, p, 0) == nat.MAPF_EINVAL and b'table is null' in lib.mapf_last_error()
    assert lib.mapf_set_policy_joint(fake, t, 16, None, p, 0) == nat.MAPF_EINVAL and b'offset is null' in lib.mapf_last_error()
    assert lib.mapf_set_policy_joint(fake, t, 16, o, None, 0) == nat.MAPF_EINVAL and b'partner is null' in lib.mapf_last_error()
    assert lib.mapf_set_policy_joint(fake, t, 0, o, p, 0) == nat.MAPF_EINVAL and b'table_bytes' in lib.mapf_last_error()
    assert lib.mapf_set_policy_joint(fake, t, 1 << 31, o, p, 0) == nat.MAPF_EINVAL and b'table_bytes' in lib.mapf_last_error()
    assert lib.mapf_set_policy_joint(fake, t, 16, o, p, 2) == nat.MAPF_EINVAL and b'unknown bits' in lib.mapf_last_error()


def test_header_library_and_ctypes_table_agree_on_the_new_name():
    lib = nat.load()
    raw = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    name = 'mapf_set_policy_joint'
    assert re.search(r'\bint %s\s*\(' % name, text) and hasattr(lib, name) and name in nat.SIGNATURES
    declared = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
    assert len(declared.split(',')) == len(nat.SIGNATURES[name][1]) == 6
    assert re.search(r'#define\s+MAPF_POLICY_JOINT\s+3\b', raw) and nat.MAPF_POLICY_JOINT == 3
    assert 'tables over joint states of agent groups' not in raw            # the table policy's "out of scope" points here now
    # a new symbol only: the ABI version and the rollout's argument block stay
    assert lib.mapf_abi_version() == nat.MAPF_ABI_VERSION == 6 and re.search(r'#define\s+MAPF_ABI_VERSION\s+6\b', raw)
    fields = [f for f, _ in nat.MapfRolloutIO._fields_]
    body = re.search(r'typedef struct mapf_rollout_io \{(.*?)\} mapf_rollout_io;', text, flags=re.S).group(1)
    assert re.findall(r'(\w+);', body) == fields and fields[-1] == 'rec_prob' and ctypes.sizeof(nat.MapfRolloutIO) == 88


def _table(target):
    text = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, target], universal_newlines=True)
    return dict(line.split() for line in text.splitlines())


def test_the_new_units_are_the_makefiles_third_table():
    first, added, joint = _table('print-kernel-units'), _table('print-added-kernel-units'), _table('print-joint-kernel-units')
    assert joint == {unit: SOURCE for unit in NEW_UNITS} and list(joint) == list(NEW_UNITS) == list(device_listings.joint_units())
    assert os.path.exists(os.path.join(CSRC, SOURCE + '.hip'))
    assert len(first) == 20 and list(added) == list(ADDED_UNITS) and not (set(first) | set(added)) & set(joint)
    dry = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, '-n', '-B', 'all', 'listings'], universal_newlines=True)
    for unit in list(first) + list(added) + list(joint):
        assert '/%s.o' % unit in dry and '/%s.s' % unit in dry, unit


@pytest.mark.parametrize('unit', NEW_UNITS)
def test_a_new_unit_holds_its_declared_instances_free_of_spills_and_scratch(unit):
    kernels = kernel_meta.kernels(device_listings.listings(unit)[unit])
    rollout = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'JNS_11JointPolicyE' + PACKS[unit] + 'EE' in k['name']]
    # 7 group sizes x FULL x MV_LDS x RECORD, as the unit's family comment declares; nothing else, and never beside the table policy
    assert re.search(r'each form: 7 group sizes x FULL x MV_LDS x RECORD = 56 instances', open(os.path.join(CSRC, SOURCE + '.hip')).read())
    assert (len(rollout), len(kernels)) == (56, 56) and not any('TablePolicy' in k['name'] for k in kernels)
    for k in kernels:
        assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0), k


def test_the_units_that_count_pairs_keep_their_code():
    for unit, want in PARENT_LISTINGS.items():
        text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', device_listings.listings(unit)[unit])
        assert 'JointPolicy' not in text, unit
        assert hashlib.sha256(text.encode()).hexdigest() == want, unit


def test_the_route_without_the_mode_is_what_it_was(shim):
    """tests/host_tables_shim.hip routes without the mode (the `joint` fact defaults to off): the 8-agent bench shape under the table
    policy still takes a packed kernel, and the limit / budget instances their names"""
    for limited, budgeted, want_family, want in ((0, 0, PACKED, 'lq_rollout_kernel_table<'), (1, 0, LG, 'lg_rollout_kernel_table_limit_guarded<'),
                                                 (1, 1, LG, 'lg_rollout_kernel_table_budget_guarded<')):
        family, _, name = routed_rollout(shim, 683, 8, 65536, AUTO, 2, limited=limited, budgeted=budgeted, table_bytes=8 * 683)
        assert family == want_family and name.startswith(want) and 'JOINT' not in name and 'joint' not in name, name


# ------------------------------------------------------------------- envs/policies.py
def _small_grid():
    return MapfGrid(['...', '.@.', '...'])      # 8 free cells


def test_pair_rows_from_policy_round_trips_a_random_two_agent_policy():
    from gym_mapf_amd.envs.mapf_env import integer_action_to_vector

    class Local:                                 # what pair_rows_from_policy reads of a two-agent MapfEnv
        def __init__(self, grid, n_agents=2):
            self.n_agents = n_agents
            self.valid_locations, self.loc_to_int, _ = grid.tables()

        def state_to_locations(self, s):
            V = len(self.valid_locations)
            return tuple(self.valid_locations[(s // V ** k) % V] for k in range(self.n_agents))

    env = Local(_small_grid())
    V = len(env.valid_locations)
    assert V == 8
    codes = np.random.RandomState(5).randint(0, 25, size=V * V)
    rows_0, rows_1 = policies.pair_rows_from_policy(env, lambda s: codes[s])
    assert rows_0.shape == rows_1.shape == (V, V) and rows_0.dtype == rows_1.dtype == np.uint8
    for s in range(V * V):
        c0, c1 = s % V, s // V                   # agent 0 is the least significant digit, of states and of actions
        names = integer_action_to_vector(int(codes[s]), 2)
        assert (ACTIONS[rows_0[c0, c1]], ACTIONS[rows_1[c1, c0]]) == tuple(names)
        assert (rows_0[c0, c1], rows_1[c1, c0]) == (codes[s] % 5, codes[s] // 5)
    with pytest.raises(ValueError):
        policies.pair_rows_from_policy(Local(_small_grid(), 1), lambda s: 0)
    with pytest.raises(ValueError):
        policies.pair_rows_from_policy(Local(_small_grid(), 3), lambda s: 0)
    with pytest.raises(ValueError):
        policies.pair_rows_from_policy(env, lambda s: 25)


@pytest.mark.parametrize('W', jc.MERGE_WIDTHS)
def test_pair_shortest_path_rows_never_conflicts_and_reaches_the_joint_goal(W):
    w = jc.merge(W, 3)
    V, nbr = w.V, w.nbr.astype(np.int64)
    goal_i, goal_j = int(w.goal[0, 0]), int(w.goal[0, 1])
    rows_i, rows_j = policies.pair_shortest_path_rows(w.grid, goal_i, goal_j)
    assert rows_i.shape == rows_j.shape == (V, V) and rows_i.dtype == rows_j.dtype == np.uint8 and rows_i.max() <= 4 and rows_j.max() <= 4
    # the joint cells that can reach the joint goal, by a search of this test's own over the allowed joint moves
    allowed = lambda ci, cj, ni, nj: ni != nj and not (ni == cj and nj == ci)
    reach, frontier = {(goal_i, goal_j)}, [(goal_i, goal_j)]
    while frontier:
        ci, cj = frontier.pop()
        for a_i, a_j in itertools.product(range(5), repeat=2):
            nxt = (int(nbr[ci, a_i]), int(nbr[cj, a_j]))
            if allowed(ci, cj, *nxt) and nxt not in reach:                  # (moves have reverses: forward from the goal)
                reach.add(nxt)
                frontier.append(nxt)
    assert (int(w.start[0, 0]), int(w.start[0, 1])) in reach
    for ci in range(V):
        for cj in range(V):
            a_i, a_j = int(rows_i[ci, cj]), int(rows_j[cj, ci])
            if (ci, cj) not in reach or (ci, cj) == (goal_i, goal_j):
                assert (a_i, a_j) == (0, 0), (ci, cj)
                continue
            at, steps = (ci, cj), 0
            while at != (goal_i, goal_j):                                   # follows the plan: never a conflict, always arrives
                nxt = (int(nbr[at[0], rows_i[at]]), int(nbr[at[1], rows_j[at[1], at[0]]]))
                assert allowed(at[0], at[1], *nxt) and nxt != at, (ci, cj, at)
                at, steps = nxt, steps + 1
                assert steps <= V * V
    # the tie-break: the first joint action in product order that is one step closer -- STAY first, so an agent waits when it may
    with pytest.raises(ValueError):
        policies.pair_shortest_path_rows(w.grid, goal_i, goal_i)
    with pytest.raises(ValueError):
        policies.pair_shortest_path_rows(w.grid, goal_i, V)


def test_join_plan_lays_the_segments_out_and_rejects_a_bad_cover():
    V = 8
    rs = np.random.RandomState(3)
    row = lambda: rs.randint(0, 5, size=V).astype(np.uint8)
    square = lambda: rs.randint(0, 5, size=(V, V)).astype(np.uint8)
    solo, pairs = {0: row(), 3: row()}, {(1, 4): (square(), square()), (5, 2): (square(), square())}
    table, offsets, partners = policies.join_plan(V, 6, solo, pairs)
    assert table.dtype == np.uint8 and offsets.dtype == np.uint32 and partners.dtype == np.uint16
    assert partners.tolist() == [0, 4, 5, 3, 1, 2] and table.size == 2 * V + 4 * V * V
    VecMapfEnv._joint_arguments(V, 7, 6, table, offsets, partners)
    state = rs.randint(0, V, size=(7, 6))
    acts = jc.joint_actions(table, offsets, partners, state, V)
    for e in range(7):
        assert acts[e, 0] == solo[0][state[e, 0]] and acts[e, 3] == solo[3][state[e, 3]]
        assert acts[e, 1] == pairs[1, 4][0][state[e, 1], state[e, 4]] and acts[e, 4] == pairs[1, 4][1][state[e, 4], state[e, 1]]
        assert acts[e, 5] == pairs[5, 2][0][state[e, 5], state[e, 2]] and acts[e, 2] == pairs[5, 2][1][state[e, 2], state[e, 5]]
    for bad_solo, bad_pairs in (({0: row(), 3: row(), 1: row()}, pairs),                     # agent 1 twice
                                ({0: row()}, pairs),                                         # agent 3 never
                                (solo, {(1, 4): pairs[1, 4], (5, 5): pairs[5, 2]}),          # agent 5 twice, agent 2 never
                                ({0: row(), 6: row()}, pairs),                               # no such agent
                                ({0: row(), 3: np.zeros(V + 1, np.uint8)}, pairs),
                                ({0: row(), 3: np.full(V, 5, np.uint8)}, pairs)):
        with pytest.raises(ValueError):
            policies.join_plan(V, 6, bad_solo, bad_pairs)


# ------------------------------------------------------------------- VecMapfEnv.set_policy('joint'): the errors that need no handle
def test_set_policy_joint_argument_errors():
    V, E, A = 8, 3, 4
    table = np.zeros(2 * V * V + 2 * V, np.uint8)
    offsets, partners = np.asarray([0, V * V, 2 * V * V, 2 * V * V + V]), np.asarray([1, 0, 2, 3])
    check = lambda **kw: VecMapfEnv._joint_arguments(V, E, A, **dict(dict(table=table, offsets=offsets, partners=partners), **kw))
    t8, o32, p16 = check()
    assert (t8.dtype, o32.dtype, p16.dtype) == (np.uint8, np.uint32, np.uint16) and o32.shape == (A,)
    assert check(offsets=np.tile(offsets, (E, 1)), partners=np.tile(partners, (E, 1)))[1].shape == (E, A)
    bad_byte = table.copy()
    bad_byte[77] = 5
    for kw, says in ((dict(table=None), 'needs'), (dict(table=bad_byte), r'table\[77\] = 5'), (dict(table=table.reshape(2, -1)), r'\[N\]'),
                     (dict(table=table.astype(np.float32)), 'integer'), (dict(offsets=offsets[:3]), r'\[E, A\]'),
                     (dict(partners=np.tile(partners, (E, 1))), 'both'), (dict(partners=np.asarray([1, 0, 2, 4])), r'partners\[3\] = 4'),
                     (dict(partners=np.asarray([1, 2, 0, 3])), 'not mutual'), (dict(partners=np.asarray([1, 1, 2, 3])), 'not mutual'),
                     (dict(offsets=np.asarray([0, V * V, 2 * V * V, 2 * V * V + V + 1])), 'ends past'),
                     (dict(offsets=np.asarray([1, V * V, 2 * V * V, 2 * V * V + V])), None),        # overlapping segments are fine
                     (dict(offsets=np.asarray([V * V + 2 * V + 1, V * V, 0, 0])), r'offsets\[0\] = 81: the segment of 64 bytes ends past'), (dict(offsets=np.asarray([-1, 0, 0, 0])), 'offsets')):
        if says is None:
            check(**kw)
            continue
        with pytest.raises(ValueError, match=says):
            check(**kw)
    with pytest.raises(ValueError, match=r'offsets\[2, 3\]'):               # [E, A] arrays: the entry is named by (env, agent)
        per_env = np.tile(offsets, (E, 1))
        per_env[2, 3] += 1
        check(offsets=per_env, partners=np.tile(partners, (E, 1)))
