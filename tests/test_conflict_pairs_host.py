"""CPU-side checks of the conflict matrix (include/mapf_hip.h mapf_set_conflict_pairs): the two entry points validate their arguments
before a handle is touched, header / library / ctypes table agree on them, the ABI, mapf_rollout_io and the debug plans are what
they were, the route of a launch without the matrix is what it was, the three new compilations are in the Makefile's
second table (the first one, which tests/test_cabi_and_host.py pins, is what it was) and hold exactly the declared instances without
register spills or scratch -- the gate that test applies to the first table --, and the lane-group rollout units that exist
without the matrix compile to the listings they had.  No compute is launched here.  (What needs a live handle -- a slot beyond
n_slots, an oversize matrix, reading with the mode off, graph_begin -- is refused on the GPU in tests/test_gpu_conflict_pairs.py.)"""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gym_mapf_amd import _native as nat
from host_shim import CSRC, device_listings, kernel_meta
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import AUTO, LG, PACKED, routed_rollout

HEADER = os.path.join(ROOT, 'include', 'mapf_hip.h')
NEW_SYMBOLS = ('mapf_set_conflict_pairs', 'mapf_conflict_pairs')
NEW_UNITS = ('mapf_lg_pairs_plain', 'mapf_lg_pairs_limit', 'mapf_lg_pairs_budget')
# the mangled argument packs behind (args, A) of each new compilation: without and with the table policy
PACKS = {'mapf_lg_pairs_plain': 'NS_13ConflictPairsEEE', 'mapf_lg_pairs_limit': 'NS_12EpisodeLimitENS_13ConflictPairsEEE',
         'mapf_lg_pairs_budget': 'NS_12EpisodeLimitENS_13EpisodeBudgetENS_13ConflictPairsEEE'}
# sha256 of the device listings (hipcc -S --cuda-device-only, __hip_cuid_* masked) of the lane-group rollout units that exist without
# the matrix, as the commit before the conflict matrix compiles them: the units keep their code
PARENT_LISTINGS = {
    'mapf_lg_rollout': 'cf814f5e15462bda86bb1e683f830326f8d6e6e3e1ea1e8cfa7806751704136a',
    'mapf_lg_limit': '6dab14bdfeeae266939ed8e2a9f55fff679f1535184ed7ebaee74d9567246e7b',
    'mapf_lg_budget': '2000985c67752641521423b10c58a1102aa132d97d1ebc0e6c98f8a763d51dfb',
}


def test_new_entry_points_validate_their_arguments_without_a_device():
    lib = nat.load()
    slots = np.zeros(4, np.uint32)
    out = np.zeros(4, np.uint64)
    assert lib.mapf_set_conflict_pairs(None, 1, slots.ctypes.data) == nat.MAPF_EINVAL and b'set_conflict_pairs: null handle' in lib.mapf_last_error()
    assert lib.mapf_set_conflict_pairs(None, 0, None) == nat.MAPF_EINVAL
    assert lib.mapf_conflict_pairs(None, out.ctypes.data, 0) == nat.MAPF_EINVAL and b'conflict_pairs: null handle' in lib.mapf_last_error()
    assert lib.mapf_conflict_pairs(None, None, 1) == nat.MAPF_EINVAL


def test_header_library_and_ctypes_table_agree_on_the_new_names():
    lib = nat.load()
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, text), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
        declared = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
        assert len(declared.split(',')) == len(nat.SIGNATURES[name][1]), name      # one ctypes argument per declared one
    # new symbols only: the ABI version and the rollout's argument block stay
    assert lib.mapf_abi_version() == nat.MAPF_ABI_VERSION == 6 and re.search(r'#define\s+MAPF_ABI_VERSION\s+6\b', open(HEADER).read())
    fields = [f for f, _ in nat.MapfRolloutIO._fields_]
    body = re.search(r'typedef struct mapf_rollout_io \{(.*?)\} mapf_rollout_io;', text, flags=re.S).group(1)
    assert re.findall(r'(\w+);', body) == fields and fields[-1] == 'rec_prob' and ctypes.sizeof(nat.MapfRolloutIO) == 88


def test_the_debug_plans_are_what_they_were():
    """mapf_debug_rollout_plan* answer for launches without the matrix: the packed plans and the lane-group limit plans they gave"""
    lib = nat.load()
    out = (ctypes.c_uint64 * 6)()
    limited = {(341, 2, 37): (2, 1, 0, 64, 0, 1), (341, 3, 64): (2, 2, 0, 64, 0, 2), (341, 8, 64): (2, 4, 0, 64, 0, 4),
               (341, 16, 37): (2, 8, 0, 64, 0, 5), (341, 32, 64): (2, 16, 0, 64, 0, 16),
               (341, 8, 65536): (2, 4, 1, 256, 341 * 5 * 16, 1024), (683, 8, 65536): (2, 4, 1, 512, 683 * 5 * 16, 512)}
    for (V, A, E), plan in limited.items():
        assert lib.mapf_debug_rollout_plan_limited(V, A, E, 64, 0, 1, 256, None, 4, out) == 0
        assert tuple(out) == plan, ((V, A, E), tuple(out))
    # an 8-agent batch of the bench's size still gets a packed plan, an odd team none
    assert lib.mapf_debug_rollout_plan(683, 8, 65536, 64, 0, 1, 256, None, out) == 1 and out[0] in (2, 4, 8)
    assert lib.mapf_debug_rollout_plan(683, 7, 65536, 64, 0, 1, 256, None, out) == 0 and tuple(out) == (0,) * 6


def test_the_route_without_the_matrix_is_what_it_was(shim):
    """tests/host_tables_shim.hip routes without the matrix (the `pairs` fact defaults to off): the 8-agent bench shape under the
    policy stream still takes a packed kernel without a limit and the lane-group limit / budget instances with one, under their names"""
    for limited, budgeted, want_family, want in ((0, 0, PACKED, 'lq_rollout_kernel'), (1, 0, LG, 'lg_rollout_kernel_limit_guarded<'),
                                                 (1, 1, LG, 'lg_rollout_kernel_budget_guarded<')):
        family, _, name = routed_rollout(shim, 683, 8, 65536, AUTO, 1, limited=limited, budgeted=budgeted)
        assert family == want_family and name.startswith(want) and 'PAIRS' not in name and 'pairs' not in name, name


def _table(target):
    text = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, target], universal_newlines=True)
    return dict(line.split() for line in text.splitlines())


def test_the_new_units_are_in_the_makefiles_second_table_and_no_other_file_holds_a_kernel():
    """`make print-added-kernel-units` lists the three compilations of pairs/mapf_lg_pairs.hip and nothing else; the first table is the
    twenty units it was; and every .hip file below csrc is the source of an entry of one of the two tables or a host unit without
    a kernel -- as tests/test_cabi_and_host.py has it for the first table and the directory itself"""
    first, added = _table('print-kernel-units'), _table('print-added-kernel-units')
    assert added == {unit: 'pairs/mapf_lg_pairs' for unit in NEW_UNITS} and list(added) == list(NEW_UNITS)
    assert len(first) == 20 and not set(first) & set(added) and list(device_listings.units()) == list(first)
    sources = set(first.values()) | set(added.values())
    found = sorted(os.path.relpath(os.path.join(d, f), CSRC)[:-4] for d, _, files in os.walk(CSRC) if os.path.relpath(d, CSRC).split(os.sep)[0] != 'build'
                   for f in files if f.endswith('.hip'))
    assert sorted(u for u in found if u not in sources) == ['mapf_capi', 'mapf_dispatch', 'mapf_plan', 'mapf_tables']
    # both tables go into the library and into `make listings`
    dry = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, '-n', '-B', 'all', 'listings'], universal_newlines=True)
    for unit in list(first) + list(added):
        assert '/%s.o' % unit in dry and '/%s.s' % unit in dry, unit


@pytest.mark.parametrize('unit', NEW_UNITS)
def test_a_new_unit_holds_its_declared_instances_free_of_spills_and_scratch(unit):
    kernels = kernel_meta.kernels(device_listings.listings(unit)[unit])
    rollout = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'J' + PACKS[unit] in k['name']]
    table = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'JNS_11TablePolicyE' + PACKS[unit] in k['name']]
    # 7 group sizes x FULL x MV_LDS x RECORD x (STREAM | table), as the unit's family comment declares; nothing else
    assert re.search(r'each form: 7 group sizes x FULL x MV_LDS x RECORD x \(STREAM \| table\)', open(os.path.join(CSRC, 'pairs', 'mapf_lg_pairs.hip')).read())
    assert (len(rollout), len(table), len(kernels)) == (112, 56, 168)
    for k in kernels:
        assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0), k


def test_the_existing_lane_group_rollout_units_keep_their_code():
    for unit, want in PARENT_LISTINGS.items():
        text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', device_listings.listings(unit)[unit])
        assert 'ConflictPairs' not in text, unit
        assert hashlib.sha256(text.encode()).hexdigest() == want, unit
