"""CPU-side checks of the group policy (include/mapf_hip.h MAPF_POLICY_GROUP, mapf_set_policy_group): every validation rule fires with
its index named (through mapf_debug_policy_group, which runs the entry point's own checks without a handle), the host builder of the
device table agrees with a Python dict through the shared probe function, header / library / ctypes table agree, the ABI is what it
was, the eight new compilations are the Makefile's fifth table and hold exactly the declared instances without register spills or
scratch, the log units compile to the listings the commit before gave them, the route sends a group launch to the lane-group plan
whatever the handle prefers, and the argument checks of VecMapfEnv.set_policy('group') do what they say.  No compute is launched
here.  (That a refused call keeps the previous policy needs a live handle: tests/test_gpu_group_policy.py.)"""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import group_policy_cases as gc
from conftest import ROOT
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs.vec_env import VecMapfEnv
from host_shim import CSRC, device_listings, kernel_meta
from plan_sweeps import AUTO, KERNEL_NAME_BYTES, LG, PREFER_LG, PREFER_TPE

HEADER = os.path.join(ROOT, 'include', 'mapf_hip.h')
SOURCE = '../csrc_group/mapf_lg_group'
GROUP, LIMIT, BUDGET, LOG, PAIRS = 'NS_11GroupPolicyE', 'NS_12EpisodeLimitE', 'NS_13EpisodeBudgetE', 'NS_10EpisodeLogE', 'NS_13ConflictPairsE'
# the mangled argument packs behind (args, A, GroupPolicy) of each new compilation
PACKS = {'mapf_lg_group_plain': '', 'mapf_lg_group_limit': LIMIT, 'mapf_lg_group_budget': LIMIT + BUDGET,
         'mapf_lg_group_pairs_plain': PAIRS, 'mapf_lg_group_pairs_limit': LIMIT + PAIRS, 'mapf_lg_group_pairs_budget': LIMIT + BUDGET + PAIRS,
         'mapf_lg_group_log_budget': LIMIT + BUDGET + LOG, 'mapf_lg_group_log_pairs_budget': LIMIT + BUDGET + LOG + PAIRS}
NEW_UNITS = tuple(PACKS)
LOG_UNITS = ('mapf_lg_log_budget', 'mapf_lg_log_pairs_budget', 'mapf_lg_log_joint_budget', 'mapf_lg_log_joint_pairs_budget')
# sha256 of the device listings (hipcc -S --cuda-device-only, __hip_cuid_* masked) of the units that keep an episode log, as the
# commit before the group policy compiles them: the units keep their code
PARENT_LISTINGS = {
    'mapf_lg_log_budget': '42b8a48047e9c8f9568bfa09d17abbc12fd0353f4ab6fa8a44fd16c897cde4be',
    'mapf_lg_log_pairs_budget': '2973d036f6ace5ed2dd7849cdd509b80a44b3d3f0fec4284cdae22cd9d37fd5b',
    'mapf_lg_log_joint_budget': 'cb93077a9a455a5e9f563ada506c9cafdba769f059e60bc8c019e96e0333af0b',
    'mapf_lg_log_joint_pairs_budget': '4aade89b974fbfae8ed5461fc296cd28fd0e5b43b63708d6ee14993123fe8a1b',
}
PAD, MISS = nat.MAPF_GROUP_PAD, nat.MAPF_GROUP_MISS


# ------------------------------------------------------------------- the validation, through the debug entry
def _debug(V, A, E, plan, keys=None, key_book=None, flags=None, raw=None):
    """mapf_debug_policy_group over a plan dict (arrays as the library takes them): (rc, error, actions, probes, slots, max_probe)"""
    lib = nat.load()
    table = np.ascontiguousarray(plan['table'], np.uint8)
    rows, members, book = (np.ascontiguousarray(plan[k], t) for k, t in (('rows', np.uint16), ('members', np.uint16), ('book', np.uint32)))
    entries = np.zeros(len(plan['entry_cells']), nat.GROUP_ENTRY_DTYPE)
    entries['cell'], entries['action'] = plan['entry_cells'], plan['entry_actions']
    begin = np.ascontiguousarray(plan['book_begin'], np.uint32)
    keys = np.zeros((0, 4), np.uint16) if keys is None else np.ascontiguousarray(keys, np.uint16)
    key_book = np.zeros(0, np.uint32) if key_book is None else np.ascontiguousarray(key_book, np.uint32)
    actions, probes = np.zeros(len(keys), np.uint32), np.zeros(len(keys), np.uint32)
    slots, chain = ctypes.c_uint64(0), ctypes.c_uint32(0)
    flags = (nat.MAPF_POLICY_ROWS_BROADCAST if rows.ndim == 1 else 0) if flags is None else flags
    ptr = dict(table=table.ctypes.data, rows=rows.ctypes.data, members=members.ctypes.data, book=book.ctypes.data, entries=entries.ctypes.data, begin=begin.ctypes.data)
    ptr.update(raw or {})
    rc = lib.mapf_debug_policy_group(V, A, E, ptr['table'], table.shape[0], ptr['rows'], ptr['members'], ptr['book'], ptr['entries'], entries.size, ptr['begin'],
                                     begin.size - 1, flags, len(keys), keys.ctypes.data, key_book.ctypes.data, actions.ctypes.data, probes.ctypes.data,
                                     ctypes.byref(slots), ctypes.byref(chain))
    return rc, lib.mapf_last_error().decode(), actions, probes, slots.value, chain.value


def _small_plan():
    """V = 10, A = 6, E = 3: per env the groups (0, 2, 5) on book 1 and (1, 3) on book 0, agent 4 solo; two entries per book"""
    V, A, E = 10, 6, 3
    members = np.full((E, A, 4), PAD, np.uint16)
    book = np.zeros((E, A), np.uint32)
    for group, b in (((0, 2, 5), 1), ((1, 3), 0), ((4,), 77)):
        for i in group:
            members[:, i, :len(group)], book[:, i] = group, b
    cells = np.asarray([[1, 2, PAD, PAD], [2, 1, PAD, PAD], [3, 4, 5, PAD], [9, 0, 1, PAD]], np.uint16)
    actions = np.asarray([[1, 2, 0, 0], [3, 4, 0, 0], [1, 1, 1, 0], [4, 0, 2, 0]], np.uint8)
    return V, A, E, dict(table=np.zeros((2, V), np.uint8), rows=np.ones((E, A), np.uint16), members=members, book=book, entry_cells=cells, entry_actions=actions,
                         book_begin=np.asarray([0, 2, 4], np.uint32))


def _changed(plan, key, index, value):
    out = dict(plan)
    out[key] = np.array(plan[key])
    out[key][index] = value
    return out


def test_every_validation_rule_fires_with_its_index_named():
    V, A, E, plan = _small_plan()
    rc, err, *_ = _debug(V, A, E, plan)
    assert rc == nat.MAPF_OK, err
    flat = lambda e, i, k=None: (e * A + i) if k is None else (e * A + i) * 4 + k
    cases = [
        # null pointers; entries / book_begin only with no entries and no books
        (plan, dict(raw={'table': None}), 'table is null'), (plan, dict(raw={'rows': None}), 'row_index is null'),
        (plan, dict(raw={'members': None}), 'members is null'), (plan, dict(raw={'book': None}), 'book is null'),
        (plan, dict(raw={'entries': None}), 'entries is null'), (plan, dict(raw={'begin': None}), 'book_begin is null'),
        (plan, dict(flags=2), 'unknown bits'),
        # the table policy's own checks
        (_changed(plan, 'table', (1, 7), 5), {}, 'table[17] = 5 is not an action'),
        (_changed(plan, 'rows', (2, 3), 2), {}, 'row_index[%d] = 2 is not below n_rows' % flat(2, 3)),
        # the groups
        (_changed(plan, 'members', (1, 0, 2), A), {}, 'members[%d] = %d is not below n_agents' % (flat(1, 0, 2), A)),
        (_changed(_changed(plan, 'members', (1, 1, 1), PAD), 'members', (1, 1, 2), 3), {}, 'members[%d] = 3 follows padding' % flat(1, 1, 2)),
        (_changed(_changed(plan, 'members', (1, 0, 1), 5), 'members', (1, 0, 2), 2), {}, 'members[%d] = 2 is not above members[%d]' % (flat(1, 0, 2), flat(1, 0, 1))),
        (_changed(plan, 'members', (2, 4, 0), 3), {}, 'members[%d..]: the list of agent 4 does not contain it' % flat(2, 4, 0)),
        (_changed(plan, 'members', (0, 3, 0), 0), {}, 'members[%d..]: agent 3 is a member of agent 1' % flat(0, 3, 0)),      # (0, 3) against (1, 3)
        (_changed(plan, 'book', (1, 5), 0), {}, 'book[%d] = 0 differs from book[%d] = 1' % (flat(1, 5), flat(1, 0))),
        (_changed(_changed(plan, 'book', (2, 1), 2), 'book', (2, 3), 2), {}, 'book[%d] = 2 is not below n_books' % flat(2, 1)),
        # the books
        (_changed(plan, 'book_begin', 0, 1), {}, 'book_begin[0] = 1 is not 0'),
        (_changed(plan, 'book_begin', 1, 5), {}, 'book_begin[2] = 4 is below book_begin[1]'),
        (_changed(plan, 'book_begin', 2, 3), {}, 'book_begin[2] = 3 is not n_entries'),
        # the entries
        (_changed(plan, 'entry_cells', (2, 1), V), {}, 'entries[2].cell[1] = %d is not a cell' % V),
        (_changed(_changed(_changed(plan, 'entry_cells', (0, 2), 4), 'entry_cells', (0, 1), PAD), 'entry_actions', (0, 1), 0), {},
         'entries[0].cell[2] = 4 follows padding: padding must be trailing'),
        (_changed(plan, 'entry_actions', (3, 2), 5), {}, 'entries[3].action[2] = 5 is not an action'),
        (_changed(plan, 'entry_actions', (1, 3), 1), {}, 'entries[1].action[3] = 1 at a padded position'),
        (_changed(plan, 'entry_cells', 1, [1, 2, PAD, PAD]), {}, 'entries[1] has the same four cells as an earlier entry of book 0'),
    ]
    for bad, kw, says in cases:
        rc, err, *_ = _debug(V, A, E, bad, **kw)
        assert rc == nat.MAPF_EINVAL and says in err and err.startswith('set_policy_group: '), (says, rc, err)
    # the same cells in ANOTHER book are no duplicate; an entry of another arity with the same leading cells neither
    rc, err, *_ = _debug(V, A, E, _changed(_changed(plan, 'entry_cells', 2, [1, 2, PAD, PAD]), 'entry_actions', 2, [1, 1, 0, 0]))
    assert rc == nat.MAPF_OK, err
    rc, err, *_ = _debug(V, A, E, _changed(plan, 'entry_cells', 1, [1, 2, 7, PAD]))
    assert rc == nat.MAPF_OK, err
    # n_books == 0 with n_entries == 0: null entries and book_begin are fine, and book is not read
    none = dict(plan, entry_cells=np.zeros((0, 4), np.uint16), entry_actions=np.zeros((0, 4), np.uint8), book_begin=np.zeros(1, np.uint32))
    rc, err, _, _, slots, chain = _debug(V, A, E, none, raw={'entries': None, 'begin': None})
    assert (rc, slots, chain) == (nat.MAPF_OK, 1, 0), err
    # V = 65536 would make cell 0xFFFF ambiguous
    rc, err, *_ = _debug(65536, A, E, dict(plan, table=np.zeros((1, 65536), np.uint8), rows=np.zeros((E, A), np.uint16)))
    assert rc == nat.MAPF_EUNSUPPORTED and 'V <= 65535' in err
    # more than 2^24 entries: refused before an entry is read (the pointer is never followed that far)
    lib = nat.load()
    one = np.zeros(1, nat.GROUP_ENTRY_DTYPE)
    t, r, m, b = (np.ascontiguousarray(plan[k], ty) for k, ty in (('table', np.uint8), ('rows', np.uint16), ('members', np.uint16), ('book', np.uint32)))
    begin = np.asarray([0, (1 << 24) + 1], np.uint32)
    rc = lib.mapf_debug_policy_group(V, A, E, t.ctypes.data, 2, r.ctypes.data, m.ctypes.data, b.ctypes.data, one.ctypes.data, (1 << 24) + 1, begin.ctypes.data, 1, 0,
                                     0, None, None, None, None, None, None)
    assert rc == nat.MAPF_EINVAL and b'exceeds 2^24' in lib.mapf_last_error()


def test_the_entry_point_looks_at_its_pointers_before_the_handle():
    lib = nat.load()
    V, A, E, plan = _small_plan()
    arrays = [np.ascontiguousarray(plan[k], ty) for k, ty in (('table', np.uint8), ('rows', np.uint16), ('members', np.uint16), ('book', np.uint32))]
    t, r, m, b = (a.ctypes.data for a in arrays)
    call = lambda h, t, r, m, b, flags=0: lib.mapf_set_policy_group(h, t, 2, r, m, b, None, 0, None, 0, flags)
    assert call(None, t, r, m, b) == nat.MAPF_EINVAL and b'set_policy_group: null handle' in lib.mapf_last_error()
    fake = ctypes.c_void_p(1)                   # (never dereferenced: the pointers and the flags are looked at first)
    for args, says in (((None, r, m, b), b'table is null'), ((t, None, m, b), b'row_index is null'), ((t, r, None, b), b'members is null'),
                       ((t, r, m, None), b'book is null'), ((t, r, m, b, 2), b'unknown bits')):
        assert call(fake, *args) == nat.MAPF_EINVAL and says in lib.mapf_last_error(), says
    assert lib.mapf_policy_group_stats(None, None, None) == nat.MAPF_EINVAL


# ------------------------------------------------------------------- the builder, against a dict
def _random_books(n_entries, n_books, V, seed):
    """random books over cells that include 0, V - 1 and ids above 32767: ({book: {key: actions}}, the plan's three entry arrays)"""
    rs = np.random.RandomState(seed)
    books = [dict() for _ in range(n_books)]
    pool = np.concatenate([[0, V - 1], rs.randint(32768, V, size=20), rs.randint(0, V, size=40)])
    while sum(len(b) for b in books) < n_entries:
        G = int(rs.randint(1, 5))
        key = tuple(int(c) for c in rs.choice(pool, size=G)) + (PAD,) * (4 - G)
        books[int(rs.randint(0, n_books))].setdefault(key, tuple(int(a) for a in rs.randint(0, 5, size=G)) + (0,) * (4 - G))
    cells = np.asarray([k for b in books for k in b], np.uint16).reshape(-1, 4)
    actions = np.asarray([a for b in books for a in b.values()], np.uint8).reshape(-1, 4)
    begin = np.cumsum([0] + [len(b) for b in books]).astype(np.uint32)
    return books, pool, cells, actions, begin


@pytest.mark.parametrize('n_entries', (0, 1, 300, 4000))
def test_the_builder_agrees_with_a_dict_through_the_shared_probe(n_entries):
    V, A, E, n_books = 65535, 2, 1, 5
    books, pool, cells, actions, begin = _random_books(n_entries, n_books, V, 100 + n_entries)
    plan = dict(table=np.zeros((1, V), np.uint8), rows=np.zeros(A, np.uint16), members=np.asarray([[0, 1, PAD, PAD]] * 2, np.uint16), book=np.zeros(A, np.uint32),
                entry_cells=cells, entry_actions=actions, book_begin=begin)
    rs = np.random.RandomState(n_entries)
    # 10^5 keys: every present key under its own book and under another, random ones over the same cells (absent, mostly)
    present = [(k, b) for b, book in enumerate(books) for k in book]
    keys = [k for k, _ in present] + [k for k, _ in present]
    key_book = [b for _, b in present] + [(b + 1) % n_books for _, b in present]
    n_random = 100000 - len(keys)
    sizes = rs.randint(1, 5, size=n_random)
    random_keys = np.where(np.arange(4)[None, :] < sizes[:, None], rs.choice(pool, size=(n_random, 4)), PAD)
    keys = np.concatenate([np.asarray(keys, np.int64).reshape(-1, 4), random_keys])
    key_book = np.concatenate([np.asarray(key_book, np.int64), rs.randint(0, n_books + 1, size=n_random)])       # (n_books: no such book)
    rc, err, got, probes, slots, chain = _debug(V, A, E, plan, keys, key_book)
    assert rc == nat.MAPF_OK, err
    assert slots & (slots - 1) == 0 and slots >= max(1, 2 * n_entries) and (slots == 1 or slots < 4 * n_entries)
    want = np.full(len(keys), MISS, np.uint64)
    for n, (key, b) in enumerate(zip(keys.tolist(), key_book.tolist())):
        entry = books[b].get(tuple(key)) if b < n_books else None
        if entry is not None:
            want[n] = entry[0] | entry[1] << 8 | entry[2] << 16 | entry[3] << 24
    assert np.array_equal(got.astype(np.uint64), want)
    assert len(present) == n_entries and (want[:n_entries] != MISS).all() and (want[2 * n_entries:] == MISS).any()
    # the reported longest chain: no lookup reads more slots, some present key needs all of them, and 4000 entries make chains
    assert probes.max(initial=0) <= chain and (n_entries == 0 or probes[:n_entries].max() == chain)
    assert chain >= (2 if n_entries >= 4000 else min(n_entries, 1))
    assert (keys[:, 0] == 0).any() and (keys == V - 1).any() and ((keys > 32767) & (keys != PAD)).any()


def test_the_random_cases_big_table_has_probe_chains():
    A, E = gc.BIG_SHAPE
    w = gc.random_groups(A, E, big=True)
    rc, err, _, _, slots, chain = _debug(w.V, A, E, w.plan())
    assert rc == nat.MAPF_OK, err
    assert w.entry_cells.shape[0] >= gc.BIG_ENTRIES and slots == 8192 * (2 if w.entry_cells.shape[0] > 4096 else 1) and chain >= 2


# ------------------------------------------------------------------- header, library, ctypes table
def test_header_library_and_ctypes_table_agree_on_the_new_names():
    lib = nat.load()
    raw = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name, n_args in (('mapf_set_policy_group', 11), ('mapf_policy_group_stats', 3), ('mapf_debug_policy_group', 20)):
        assert re.search(r'\bint %s\s*\(' % name, text) and hasattr(lib, name) and name in nat.SIGNATURES, name
        declared = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
        assert len(declared.split(',')) == len(nat.SIGNATURES[name][1]) == n_args, name
    assert re.search(r'#define\s+MAPF_POLICY_GROUP\s+4\b', raw) and nat.MAPF_POLICY_GROUP == 4
    assert re.search(r'typedef struct mapf_group_entry \{ uint16_t cell\[4\]; uint8_t action\[4\]; \} mapf_group_entry;', raw)
    assert ctypes.sizeof(nat.MapfGroupEntry) == np.dtype(nat.GROUP_ENTRY_DTYPE).itemsize == 12
    assert 'groups of three or more (V^3 bytes)' not in raw and 'MAPF_POLICY_GROUP, below' in raw       # the joint policy's "out of scope" points here now
    for words in ('groups of five or more', 'packed and thread-per-env forms', 'the single step', 'recorded graphs', 'computes or repairs a plan on the device'):
        assert words in raw, words
    # new symbols only: the ABI version and the rollout's argument block stay
    assert lib.mapf_abi_version() == nat.MAPF_ABI_VERSION == 6 and re.search(r'#define\s+MAPF_ABI_VERSION\s+6\b', raw)
    assert ctypes.sizeof(nat.MapfRolloutIO) == 88


# ------------------------------------------------------------------- the fifth table of the Makefile
def _table(target):
    text = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, target], universal_newlines=True)
    return dict(line.split() for line in text.splitlines())


def test_the_new_units_are_the_makefiles_fifth_table():
    tables = [_table('print-%skernel-units' % t) for t in ('', 'added-', 'joint-', 'log-')]
    group = _table('print-group-kernel-units')
    assert group == {unit: SOURCE for unit in NEW_UNITS} and list(group) == list(NEW_UNITS) == list(device_listings.group_units())
    assert os.path.exists(os.path.join(CSRC, SOURCE + '.hip')) and os.listdir(os.path.join(CSRC, '..', 'csrc_group')) == ['mapf_lg_group.hip']
    assert [len(t) for t in tables] == [20, 3, 6, 4] and list(tables[3]) == list(LOG_UNITS) and not set().union(*tables) & set(group)
    dry = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, '-n', '-B', 'all', 'listings'], universal_newlines=True)
    for unit in [u for t in tables for u in t] + list(group):
        assert '/%s.o' % unit in dry and '/%s.s' % unit in dry, unit


@pytest.mark.parametrize('unit', NEW_UNITS)
def test_a_new_unit_holds_its_declared_instances_free_of_spills_and_scratch(unit):
    kernels = kernel_meta.kernels(device_listings.listings(unit)[unit])
    # 7 group sizes x FULL x MV_LDS x RECORD, as the unit's family comment declares: never streamed, never DENSE, nothing else, and
    # never beside the other table policies
    assert re.search(r'each form: 7 group sizes x FULL x MV_LDS x RECORD = 56 instances', open(os.path.join(CSRC, SOURCE + '.hip')).read())
    rollout = [k for k in kernels if re.search(r'lg_rollout_kernelILi\d+ELb[01]ELb[01]ELb[01]ELb0ELb0EJ' + GROUP + PACKS[unit] + 'EE', k['name'])]
    assert (len(rollout), len(kernels)) == (56, 56) and len({k['name'] for k in kernels}) == 56
    assert not any('TablePolicy' in k['name'] or 'JointPolicy' in k['name'] for k in kernels)
    for k in kernels:
        assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0), k['name']


def test_the_units_that_keep_a_log_keep_their_code():
    for unit, want in PARENT_LISTINGS.items():
        text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', device_listings.listings(unit)[unit])
        assert 'GroupPolicy' not in text, unit
        assert hashlib.sha256(text.encode()).hexdigest() == want, unit


# ------------------------------------------------------------------- the route
@pytest.fixture(scope='module')
def group_shim(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp('group_shim')), 'libgroup_policy_shim.so')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O1', '-std=c++17', '-fPIC', '-ffp-contract=off', '-shared', '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC,
           os.path.join(ROOT, 'tests', 'group_policy_shim.hip'), os.path.join(CSRC, 'mapf_tables.hip'), os.path.join(CSRC, 'mapf_plan.hip'), '-o', out]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert proc.returncode == 0, proc.stdout.decode('utf-8', 'replace')[-3000:]
    lib = ctypes.CDLL(out)
    lib.gshim_route_group.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_char_p]
    lib.gshim_group_lds_bytes.restype = ctypes.c_uint64
    return lib


def test_the_route_sends_a_group_launch_to_the_lane_group_plan(group_shim):
    """under every family flag and limit_packed, at the 8-agent bench shape (which a table launch routes to a packed kernel) and at
    two agents (which a plain launch routes to thread-per-env): the lane-group plan of the form, marked `group`, never dense"""
    out, name = (ctypes.c_uint64 * 13)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    assert group_shim.gshim_group_lds_bytes() == 96
    for V, A, E in ((683, 8, 65536), (683, 2, 4096), (3300, 5, 37)):
        for prefer in (AUTO, PREFER_TPE, PREFER_LG):
            for tune in (None, b'limit_packed=1', b'mv_lds_max_bytes=163840'):
                for limited, budgeted, logged in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)):
                    for pairs in (0, 1):
                        for record in (0, 1):
                            family = group_shim.gshim_route_group(V, A, E, 256, tune, prefer, limited, budgeted, pairs, logged, record, out, name)
                            L, full, mv_lds, dense, limit, budget, has_pairs, log, group, joint, block, grid, lds_bytes = out
                            tag = (V, A, E, prefer, tune, limited, budgeted, logged, pairs, record, name.value)
                            assert family == LG and group == 1 and joint == 0 and dense == 0, tag
                            assert (limit, budget, has_pairs, log) == (limited, budgeted, pairs, logged), tag
                            assert L == max(1, 1 << ((A + 1) // 2 - 1).bit_length()) and full == (A == 2 * L) and block * grid >= E * L, tag
                            # the image, the matrix's block, the log's and the policy's fit the CU's LDS beside the staged table
                            assert lds_bytes == (V * 5 * 16 if mv_lds else 0) and lds_bytes + 1024 + 32 + 64 + 96 <= 160 * 1024, tag
                            got = name.value.decode()
                            form = ('_budget_guarded_log' if logged else '_budget_guarded') if budgeted else ('_limit_guarded' if limited else '')
                            assert got.startswith('lg_rollout_kernel_group%s%s<L=%d,' % (form, '_pairs' if pairs else '', L)), tag
                            assert ',%s,GROUP,' % ('RECORD' if record else 'TOTALS') in got and len(got) < KERNEL_NAME_BYTES, tag


# ------------------------------------------------------------------- VecMapfEnv.set_policy('group'): the errors that need no handle
def test_set_policy_group_argument_errors():
    V, A, E, plan = _small_plan()
    check = lambda **kw: VecMapfEnv._group_arguments(V, E, A, **dict(plan, **kw))
    t8, r16, m16, b32, entries, begin = check()
    assert (t8.dtype, r16.dtype, m16.dtype, b32.dtype, begin.dtype) == (np.uint8, np.uint16, np.uint16, np.uint32, np.uint32)
    assert entries.dtype.itemsize == 12 and entries['cell'].tolist() == plan['entry_cells'].tolist() and m16.shape == (E, A, 4)
    shared = check(rows=plan['rows'][0], members=plan['members'][0], book=plan['book'][0])
    assert shared[1].shape == (A,) and shared[2].shape == (A, 4)
    none = check(entry_cells=None, entry_actions=None, book_begin=None)
    assert none[4].size == 0 and none[5].tolist() == [0]
    edit = lambda key, index, value: {key: _changed(plan, key, index, value)[key]}
    for kw, says in ((dict(table=None), 'needs'), (dict(entry_cells=None), 'come together'), (edit('table', (1, 7), 5), r'table\[1, 7\] = 5'),
                     (dict(table=plan['table'].reshape(-1)), r'\[R, V\]'), (dict(rows=plan['rows'][:, :3]), r'\[E, A\]'), (dict(members=plan['members'][0]), r'\[4\]'),
                     (edit('rows', (2, 3), 2), 'rows must name'), (edit('members', (1, 0, 2), A), r'members\[1, 0\]\[2\] = 6 is not an agent'),
                     (edit('members', (1, 1, 0), PAD), r'members\[1, 1\]\[1\] follows padding'), (edit('members', (1, 0, 1), 5), r'members\[1, 0\] is not ascending'),
                     (edit('members', (2, 4, 0), 3), r'members\[2, 4\] does not contain agent 4'), (edit('members', (0, 3, 0), 0), r'members\[0, 1\] names agent 3'),
                     (edit('book', (1, 5), 0), r'book\[1, 0\] = 1, but agent 5'), (edit('book', (2, 0), 2), r'book\[2, 0\] = 2 is not a book'),
                     (edit('book_begin', 1, 5), 'non-decreasing'), (edit('entry_cells', (2, 1), V), r'entry_cells\[2, 1\] = 10 is not a cell'),
                     (edit('entry_cells', (0, 0), PAD), r'entry_cells\[0, 1\] follows padding'), (edit('entry_actions', (3, 2), 5), r'entry_actions\[3, 2\] = 5'),
                     (edit('entry_actions', (1, 3), 1), r'entry_actions\[1, 3\] = 1 at a padded position'),
                     (edit('entry_cells', 1, [1, 2, PAD, PAD]), r'entry_cells\[1\] has the same four cells as entry_cells\[0\]'),
                     (dict(entry_cells=plan['entry_cells'].astype(np.float32)), 'integer')):
        with pytest.raises(ValueError, match=says):
            check(**kw)
    with pytest.raises(ValueError, match='65535'):
        VecMapfEnv._group_arguments(65536, E, A, **plan)
    # shared arrays: the entry is named by the agent alone
    with pytest.raises(ValueError, match=r'members\[4\] does not contain agent 4'):
        check(rows=plan['rows'][0], members=_changed(plan, 'members', (0, 4, 0), 3)['members'][0], book=plan['book'][0])
