"""CPU-side checks of the episode step limit (include/mapf_hip.h mapf_set_episode_limit): the new entry points validate their
arguments before a handle is touched, header / library / ctypes table agree on them, a launch under a limit never takes a packed
plan, and the limit instances of the lane-group kernels compile without register spills.  No compute is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gym_mapf_amd import _native as nat
from host_shim import device_listings, kernel_meta
from plan_sweeps import ROLLOUT_PLAN_AGENTS, ROLLOUT_PLAN_CELLS, ROLLOUT_PLAN_ENVS, ROLLOUT_PLAN_TUNES

HEADER = os.path.join(ROOT, 'include', 'mapf_hip.h')
NEW_SYMBOLS = ('mapf_set_episode_limit', 'mapf_episode_steps', 'mapf_step_limited', 'mapf_rollout_limited', 'mapf_debug_rollout_plan_limited')


def test_new_entry_points_validate_their_arguments_without_a_device():
    lib = nat.load()
    buf = np.zeros(4, np.uint32)
    assert lib.mapf_set_episode_limit(None, 5) == nat.MAPF_EINVAL and b'null handle' in lib.mapf_last_error()
    assert lib.mapf_episode_steps(None, buf.ctypes.data, None) == nat.MAPF_EINVAL and b'null handle' in lib.mapf_last_error()
    # (checked before the handle is touched, so a value that is never dereferenced shows it)
    fake = ctypes.c_void_p(0x1000)
    assert lib.mapf_episode_steps(fake, None, None) == nat.MAPF_EINVAL and b'both null' in lib.mapf_last_error()
    assert lib.mapf_step_limited(None, None, None, None, None, None, None, None, None, None, 0) == nat.MAPF_EINVAL
    io = nat.MapfRolloutIO(struct_size=ctypes.sizeof(nat.MapfRolloutIO), n_steps=1)
    assert lib.mapf_rollout_limited(None, ctypes.byref(io), buf.ctypes.data, None) == nat.MAPF_EINVAL
    out = (ctypes.c_uint64 * 6)()
    assert lib.mapf_debug_rollout_plan_limited(683, 8, 65536, 64, 1, 0, 256, None, 4, None) == nat.MAPF_EINVAL
    assert lib.mapf_debug_rollout_plan_limited(683, 0, 65536, 64, 1, 0, 256, None, 4, out) == nat.MAPF_EINVAL
    assert lib.mapf_debug_rollout_plan_limited(683, 8, 65536, 64, 1, 0, 256, b'no_such_key=1', 4, out) == nat.MAPF_EINVAL


def test_header_library_and_ctypes_table_agree_on_the_new_names():
    lib = nat.load()
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, text), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
        declared = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
        assert len(declared.split(',')) == len(nat.SIGNATURES[name][1]), name      # one ctypes argument per declared one
    assert lib.mapf_abi_version() == nat.MAPF_ABI_VERSION == 6 and re.search(r'#define\s+MAPF_ABI_VERSION\s+6\b', open(HEADER).read())
    assert b'abi 6' in lib.mapf_version()
    # mapf_rollout_io itself stays as it was: the truncation outputs are mapf_rollout_limited's own arguments
    fields = [f for f, _ in nat.MapfRolloutIO._fields_]
    body = re.search(r'typedef struct mapf_rollout_io \{(.*?)\} mapf_rollout_io;', text, flags=re.S).group(1)
    assert re.findall(r'(\w+);', body) == fields and fields[-1] == 'rec_prob' and ctypes.sizeof(nat.MapfRolloutIO) == 88


def test_no_packed_plan_is_chosen_under_a_limit():
    """the sweep of tests/test_plan_decisions.py's packed rollout group: wherever the launch without a limit takes a packed form
    (and wherever it does not), the launch with one is the lane-group limit instance's -- L lanes per env, whole waves per block,
    a grid that covers the batch, an LDS segment that is the move table or nothing"""
    lib = nat.load()
    out, lim = (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 6)()
    n_packed = 0
    cells = ROLLOUT_PLAN_CELLS[::7] + [683]
    for tune in ROLLOUT_PLAN_TUNES:
        for A in ROLLOUT_PLAN_AGENTS:
            L = 1 << ((A + 1) // 2 - 1).bit_length()
            for E in ROLLOUT_PLAN_ENVS:
                for streamed in (1, 0):
                    for V in cells:
                        packed = lib.mapf_debug_rollout_plan(V, A, E, 64, streamed, 1, 256, tune, out)
                        assert packed in (0, 1)
                        n_packed += packed
                        assert lib.mapf_debug_rollout_plan_limited(V, A, E, 64, streamed, 1, 256, tune, 0, lim) == packed and tuple(lim) == tuple(out)
                        assert lib.mapf_debug_rollout_plan_limited(V, A, E, 64, streamed, 1, 256, tune, 4, lim) == 0
                        k, lanes, mv_lds, block, lds, grid = tuple(lim)
                        ctx = (tune, A, E, streamed, V, tuple(lim))
                        assert (k, lanes) == (2, L) and block in (64, 256, 512, 1024) and block <= (512 if L == 16 else 1024), ctx
                        assert grid * (block // L) >= E > (grid - 1) * (block // L), ctx
                        assert lds == (V * 5 * 16 if mv_lds else 0) and lds + 1024 <= 160 * 1024, ctx
                        if tune == b'mv_lds_max_bytes=0':
                            assert not mv_lds, ctx
    assert n_packed > 3000


@pytest.fixture(scope='module')
def limit_listing():
    """the gfx950 device listing of the limit unit, as the Makefile compiles it"""
    return device_listings.listings('mapf_lg_limit')['mapf_lg_limit']


def test_the_limit_instances_are_free_of_register_spills(limit_listing):
    kernels = kernel_meta.kernels(limit_listing)
    # the instances of the two kernel templates by the argument types behind (args, A), as the mangled names spell the pack
    rollout = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'JNS_12EpisodeLimitEEE' in k['name']]
    table = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'JNS_11TablePolicyENS_12EpisodeLimitEEE' in k['name']]
    step = [k for k in kernels if 'lg_step_kernelI' in k['name'] and 'JNS_12EpisodeLimitEEE' in k['name']]
    # 7 group sizes x FULL x MV_LDS x RECORD x (STREAM | table); 7 x FULL x EXT_UNIFORMS; the ages' reset
    assert (len(rollout), len(table), len(step), len(kernels)) == (112, 56, 28, 197)
    for k in kernels:
        assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0), k
