"""CPU-side checks of the episode budget (include/mapf_hip.h mapf_set_episode_budget): the new entry points validate their arguments
before a handle is touched, header / library / ctypes table agree on them, the ABI and mapf_rollout_io are what they were, the limit
plans are unchanged, and the budget instances of the lane-group kernels compile to exactly the declared count without register
spills or scratch.  No compute is launched here.  (What needs a live handle -- out_live_steps without a budget, a rollout without
auto-reset, step and graph_begin under a budget -- is refused on the GPU in tests/test_gpu_episode_budget.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gym_mapf_amd import _native as nat
from host_shim import CSRC, device_listings, kernel_meta

HEADER = os.path.join(ROOT, 'include', 'mapf_hip.h')
NEW_SYMBOLS = ('mapf_set_episode_budget', 'mapf_episodes_left', 'mapf_rollout_budgeted')


def test_new_entry_points_validate_their_arguments_without_a_device():
    lib = nat.load()
    buf = np.zeros(4, np.uint32)
    assert lib.mapf_set_episode_budget(None, 5) == nat.MAPF_EINVAL and b'set_episode_budget: null handle' in lib.mapf_last_error()
    assert lib.mapf_episodes_left(None, buf.ctypes.data, None) == nat.MAPF_EINVAL and b'episodes_left: null handle' in lib.mapf_last_error()
    assert lib.mapf_episodes_left(None, None, None) == nat.MAPF_EINVAL       # (both pointers null on a live handle: the GPU test)
    io = nat.MapfRolloutIO(struct_size=ctypes.sizeof(nat.MapfRolloutIO), n_steps=1, step_flags=nat.MAPF_STEP_AUTO_RESET)
    assert lib.mapf_rollout_budgeted(None, ctypes.byref(io), None, None, buf.ctypes.data) == nat.MAPF_EINVAL and b'null handle' in lib.mapf_last_error()
    assert lib.mapf_rollout_budgeted(None, None, None, None, None) == nat.MAPF_EINVAL


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
    # mapf_rollout_budgeted is mapf_rollout_limited plus one pointer
    assert nat.SIGNATURES['mapf_rollout_budgeted'][1] == nat.SIGNATURES['mapf_rollout_limited'][1] + [ctypes.c_void_p]


def test_the_limit_plans_are_what_they_were():
    """the budget launcher takes plan_rollout_lg(..., limited = true) as the limit does: mapf_debug_rollout_plan_limited's answers are
    the geometry rules of the lane-group limit plan, for ragged and full groups, small and LDS-sized batches"""
    lib = nat.load()
    out = (ctypes.c_uint64 * 6)()
    want = {(341, 2, 37): (2, 1, 0, 64, 0, 1), (341, 3, 64): (2, 2, 0, 64, 0, 2), (341, 8, 64): (2, 4, 0, 64, 0, 4),
            (341, 16, 37): (2, 8, 0, 64, 0, 5), (341, 32, 64): (2, 16, 0, 64, 0, 16),
            (341, 8, 65536): (2, 4, 1, 256, 341 * 5 * 16, 1024), (683, 8, 65536): (2, 4, 1, 512, 683 * 5 * 16, 512)}
    for (V, A, E), plan in want.items():
        assert lib.mapf_debug_rollout_plan_limited(V, A, E, 64, 0, 1, 256, None, 4, out) == 0
        assert tuple(out) == plan, ((V, A, E), tuple(out))


@pytest.fixture(scope='module')
def budget_listing():
    """the gfx950 device listing of the budget unit, as the Makefile compiles it"""
    return device_listings.listings('mapf_lg_budget')['mapf_lg_budget']


def test_the_budget_unit_holds_its_declared_instances_free_of_spills_and_scratch(budget_listing):
    kernels = kernel_meta.kernels(budget_listing)
    # the instances of the kernel template by the argument types behind (args, A), as the mangled names spell the pack
    rollout = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'JNS_12EpisodeLimitENS_13EpisodeBudgetEEE' in k['name']]
    table = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'JNS_11TablePolicyENS_12EpisodeLimitENS_13EpisodeBudgetEEE' in k['name']]
    # 7 group sizes x FULL x MV_LDS x RECORD x (STREAM | table), as the unit's family comment declares; nothing else
    assert re.search(r'7 group sizes x FULL x MV_LDS x RECORD x \(STREAM \| table\)', open(os.path.join(CSRC, 'mapf_lg_budget.hip')).read())
    assert (len(rollout), len(table), len(kernels)) == (112, 56, 168)
    for k in kernels:
        assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0), k
