"""CPU-side checks: the C ABI library loads and exports exactly what include/mapf_hip.h declares,
the product fails loudly without a GPU (no CPU fallback), and the kernels that can be dispatched
compile without register spills.  No compute is launched here."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs.grid import MapfGrid
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from host_shim import device_listings as device_listings_of
from host_shim import CSRC, kernel_meta
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import ROLLOUT_PLAN_AGENTS, ROLLOUT_PLAN_CELLS, ROLLOUT_PLAN_ENVS, ROLLOUT_PLAN_TUNES

HEADER = os.path.join(ROOT, 'include', 'mapf_hip.h')


def _declared_functions():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(mapf_[a-z_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    lib = nat.load()
    declared = _declared_functions()
    assert len(declared) >= 16
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(nat.SIGNATURES) == declared          # the ctypes table covers the header, no more, no less
    assert b'gfx950' in lib.mapf_version()


def test_struct_layouts_match_header():
    # sizes the C side checks via struct_size; offsets follow from natural alignment of the field list
    assert ctypes.sizeof(nat.MapfDesc) == 112
    assert nat.MapfDesc.nbr.offset == 40 and nat.MapfDesc.fail_prob.offset == 64 and nat.MapfDesc.stream.offset == 104
    assert ctypes.sizeof(nat.MapfRolloutIO) == 88
    text = open(HEADER).read()
    for name, value in (('MAPF_MAX_AGENTS', nat.MAPF_MAX_AGENTS), ('MAPF_FLAG_DEVICE_PTRS', nat.MAPF_FLAG_DEVICE_PTRS),
                        ('MAPF_FLAG_THREAD_PER_ENV', nat.MAPF_FLAG_THREAD_PER_ENV),
                        ('MAPF_FLAG_LANE_GROUP', nat.MAPF_FLAG_LANE_GROUP), ('MAPF_STEP_AUTO_RESET', nat.MAPF_STEP_AUTO_RESET)):
        m = re.search(r'#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)u?' % name, text)
        assert m and int(m.group(1), 0) == value, name


def test_argument_validation_happens_before_any_device_work():
    lib = nat.load()
    h = ctypes.c_void_p()
    desc = nat.MapfDesc(struct_size=4)
    assert lib.mapf_create(ctypes.byref(desc), ctypes.byref(h)) == nat.MAPF_EINVAL
    assert b'struct_size' in lib.mapf_last_error()
    assert lib.mapf_create(None, ctypes.byref(h)) == nat.MAPF_EINVAL
    assert lib.mapf_step(None, None, None, None, None, None, None, None, None, 0) == nat.MAPF_EINVAL
    assert lib.mapf_destroy(None) == nat.MAPF_EINVAL
    nbr = np.zeros((4, 5), np.uint16) + np.arange(4, dtype=np.uint16)[:, None]
    cells = np.zeros(2, np.uint16)
    desc = nat.MapfDesc(struct_size=ctypes.sizeof(nat.MapfDesc), n_cells=4, n_agents=200, n_envs=1,
                        nbr=nbr.ctypes.data, start=cells.ctypes.data, goal=cells.ctypes.data)
    assert lib.mapf_create(ctypes.byref(desc), ctypes.byref(h)) == nat.MAPF_EUNSUPPORTED
    desc.n_agents = 2
    bad = nbr.copy(); bad[1, 2] = 9
    desc.nbr = bad.ctypes.data
    assert lib.mapf_create(ctypes.byref(desc), ctypes.byref(h)) == nat.MAPF_EINVAL and b'nbr' in lib.mapf_last_error()


def test_no_cpu_fallback_without_a_gpu():
    if nat.device_count() > 0:
        pytest.skip('a GPU is present')
    grid = MapfGrid(['....', '....'])
    with pytest.raises(nat.MapfNativeError) as err:
        VecMapfEnv(grid, 2, ((0, 0), (1, 1)), ((0, 3), (1, 2)), 0.1, -1.0, 1.0, -1.0, OptimizationCriteria.SoC, n_envs=4)
    assert err.value.code == nat.MAPF_ENODEVICE and 'no CPU fallback' in str(err.value)
    from gym_mapf_amd.envs.mapf_env import MapfEnv
    env = MapfEnv(grid, 2, ((0, 0), (1, 1)), ((0, 3), (1, 2)), 0.1, -1.0, 1.0, -1.0, OptimizationCriteria.SoC)
    assert env.s == env.locations_to_state(((0, 0), (1, 1)))       # host-side tables work anywhere
    with pytest.raises(nat.MapfNativeError):
        env.step(0)                                                # ... stepping needs the device


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'gym-mapf_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.hpp', '.cpp', '.h')):
                text = open(os.path.join(dirpath, f)).read()
                assert 'mapf_oracle' not in text and 'c_oracle' not in text and 'import philox' not in text, f


# kernels per device listing (gym-mapf_amd/csrc/Makefile's table names the listings): a unit or an instance that drops out of the
# library, or one that enters it, has to change this table
KERNELS_PER_LISTING = {
    'mapf_lg_kernels': 32, 'mapf_lg_rollout': 252, 'mapf_lg_limit': 197, 'mapf_lg_budget': 168, 'mapf_transitions': 19, 'mapf_lq_step': 84,
    'mapf_lq_rollout_k8_r1': 24, 'mapf_lq_rollout_k8_r0': 24, 'mapf_lq_rollout_k4_r1': 102, 'mapf_lq_rollout_k4_r0': 102,
    'mapf_lq_rollout_k2_r1': 48, 'mapf_lq_rollout_k2_r0': 48,
    'mapf_lq_limit_k4_r1': 30, 'mapf_lq_limit_k4_r0': 30, 'mapf_lq_limit_k2_r1': 24, 'mapf_lq_limit_k2_r0': 24,
    'mapf_kernels_g0': 16, 'mapf_kernels_g1': 12, 'mapf_kernels_g2': 8, 'mapf_kernels_g3': 8,
}


@pytest.fixture(scope='module')
def device_listings():
    """the gfx950 device listing (code + .amdgpu_metadata) of every kernel-holding compilation of the library, as the Makefile
    compiles it: {name: text}"""
    return device_listings_of.listings()


def test_the_listed_compilations_are_the_makefiles_and_hold_every_kernel(device_listings):
    """The tests' and tools' names are the Makefile's table (`make print-kernel-units`), and a translation unit outside that table
    holds no kernel: a unit cannot enter the library without entering the gates below."""
    table = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, 'print-kernel-units'], universal_newlines=True)
    table = [line.split() for line in table.splitlines()]
    assert [name for name, _ in table] == list(device_listings) == list(device_listings_of.units()) and len(table) == 20
    assert sorted(device_listings) == sorted(KERNELS_PER_LISTING)
    sources = {unit for _, unit in table}
    others = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith('.hip') and f[:-4] not in sources)
    assert others == ['mapf_capi', 'mapf_dispatch', 'mapf_plan', 'mapf_tables']
    for unit, text in device_listings_of.listings(*others).items():
        assert kernel_meta.kernels(text) == [] and '.amdhsa_kernel' not in text, unit


def test_every_dispatchable_kernel_is_free_of_register_spills(device_listings):
    """No code object the launchers can reach may spill registers: a spilling thread-per-env rollout kernel is the
    one place a wrong result was ever observed on the GPU (compiler notes), and spills cost time.  Covers
    every listing of the Makefile's table: the lane-group and packed-layout families with their limit and budget units, the
    transition kernels AND the thread-per-env family (mapf_kernels.hip, one listing per agent-count group); of the latter's
    rollout kernels only those launch_rollout_g* dispatches (A <= kTpeRolloutMaxAgents) are held to it -- the others are
    never launched."""
    max_tpe_rollout = int(re.search(r'#define MAPF_TPE_ROLLOUT_MAX\s+(\d+)', open(os.path.join(CSRC, 'mapf_kernels.hpp')).read()).group(1))
    tpe_step = tpe_rollout = 0
    for listing, text in device_listings.items():
        kernels = kernel_meta.kernels(text)
        assert len(kernels) == len({k['name'] for k in kernels}) == KERNELS_PER_LISTING[listing], (listing, len(kernels))
        for k in kernels:
            m = re.match(r'_ZN4mapf14rollout_kernelILi(\d+)E', k['name'])
            if m and int(m.group(1)) > max_tpe_rollout:
                continue                                          # compiled, never dispatched
            tpe_rollout += bool(m)
            tpe_step += k['name'].startswith('_ZN4mapf11step_kernelILi')
            assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0), (listing, k['name'], k['sgpr_spill'], k['vgpr_spill'], k['scratch'])
    assert tpe_step == 32 and tpe_rollout == max_tpe_rollout


def test_packed_kernels_layout_assumptions_hold_in_the_compiled_objects(device_listings):
    """The packed kernels hard-code two facts about their own code objects; a compiler update that moves either must fail
    HERE (a build-time check on the CPU), not as a wrong address on the GPU:
      * lq_step_kernel<BIG> re-reads its StepArgs block from the kernarg segment at kStepArgsOffset (mapf_lq_step.hip):
        the by-value StepArgs argument must sit at exactly that offset, behind the 14 preloaded dwords;
      * lds_at() names LDS locations by ABSOLUTE byte address (mapf_lq.hpp): the kernel's table image must be the kernel's
        only LDS object, i.e. start at LDS address 0 -- static LDS of exactly sizeof(TableImage) for the plain step (one
        object of the whole fixed size), none at all for the kernels whose image is the dynamic segment."""
    src = open(os.path.join(CSRC, 'mapf_lq_step.hip')).read()
    m = re.search(r'constexpr uint32_t kStepArgsOffset = ([0-9 *+]+);', src)
    args_offset = eval(m.group(1))                                # "5 * 8 + 4 * 4": plain integer arithmetic
    text = device_listings['mapf_lq_step']
    step = {k['name']: k['block'] for k in kernel_meta.kernels(text) if 'lq_step_kernel' in k['name']}
    assert len(step) >= 60                                        # 9 plain (Q, K) x 4 + BIG forms
    n_big = 0
    for name, block in step.items():
        args = [(int(o), int(z), k) for o, z, k in re.findall(r'\.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+(\w+)', block)]
        by_value = [a for a in args if a[2] == 'by_value']
        leading = [a for a in args if a[0] < args_offset]
        assert [a[0] for a in leading] == [0, 8, 16, 24, 32, 40, 44, 48, 52], (name, leading)   # five pointers, four dwords = 14 dwords
        block_arg = [a for a in by_value if a[1] > 64]
        assert len(block_arg) == 1 and block_arg[0][0] == args_offset, (name, block_arg, args_offset)
        lds = int(re.search(r'\.group_segment_fixed_size:\s+(\d+)', block).group(1))
        big = re.search(r'lq_step_kernelILi\d+ELi\d+ELb[01]ELb[01]ELi[123]E', name) is not None   # LDS-table forms: 16-byte rows / delta rows
        n_big += big
        assert lds == (0 if big else 1024), (name, lds)
        # the descriptor asks the command processor for the 14 leading dwords
        desc = text[text.index('.amdhsa_kernel ' + name):]
        desc = desc[:desc.index('.end_amdhsa_kernel')]
        assert re.search(r'\.amdhsa_user_sgpr_kernarg_preload_length\s+14\b', desc), name
    assert n_big >= 40                                            # 3 x 4 (eight agents per lane) + 4 x 4 (four) + 4 x 4 (delta rows) + 4 (delta rows + bitmaps)
    n_rollout = 0
    for listing, text in device_listings.items():
        if not listing.startswith('mapf_lq_rollout_k'):
            continue
        for k in kernel_meta.kernels(text):
            if 'lq_rollout_kernel' in k['name']:
                assert k['lds'] == 0, k['name']
                n_rollout += 1
    assert n_rollout >= 100
    # ... and no trap instruction stands in for these checks in the shipped kernels any more
    for unit in ('mapf_lq_step.hip', 'mapf_lq_rollout.hip'):
        assert '__builtin_trap' not in open(os.path.join(CSRC, unit)).read(), unit


def test_packed_rollout_dispatch_never_plans_past_the_lds_or_launch_bounds(shim):
    """mapf_debug_rollout_plan is the arithmetic the route (route_rollout) runs before every packed rollout launch (no device
    involved).  Swept over map sizes across every form's LDS boundary, agent counts, batch sizes, streamed / in-kernel policy,
    delta rows or not, and the MAPF_TUNE overrides the tests use: whatever form is planned fits the CU's 160 KB of LDS (the limit
    the launcher raises the kernel's dynamic segment to), fills whole blocks, and stays within its instance's launch bounds;
    and the forms end exactly where the next cell would not fit.  Every planned (K, Q, form) is an instance the launcher holds
    (lq_rollout_instance_exists, asked through the host shim)."""
    from gym_mapf_amd import _native
    import ctypes
    lib = _native.load()
    out = (ctypes.c_uint64 * 6)()
    LDS = 160 * 1024

    def plan(n_cells, A, E, streamed, delta, tune, n_cu=256, T=64):
        rc = lib.mapf_debug_rollout_plan(n_cells, A, E, T, streamed, delta, n_cu, tune, out)
        assert rc in (0, 1), (rc, lib.mapf_last_error())
        return rc, tuple(out)

    cells, tunes = ROLLOUT_PLAN_CELLS, ROLLOUT_PLAN_TUNES
    exists = functools.lru_cache(maxsize=None)(lambda K, Q, form: shim.shim_rollout_instance_exists(K, Q, form, 0) == 1)
    seen_forms, n_packed = set(), 0
    for tune in tunes:
        for A in ROLLOUT_PLAN_AGENTS:
            for E in ROLLOUT_PLAN_ENVS:
                for streamed in (1, 0):
                    for delta in (0, 1):
                        for V in cells:
                            rc, (K, Q, form, block, table, total) = plan(V, A, E, streamed, delta, tune)
                            if not rc:
                                continue
                            n_packed += 1
                            seen_forms.add(form)
                            ctx = (tune, A, E, streamed, delta, V, K, Q, form, block, table, total)
                            assert K in (2, 4, 8) and K * Q == A and Q in (1, 2, 4, 8, 16), ctx
                            assert exists(K, Q, form), ctx
                            assert block in (64, 128, 256, 512, 1024) and E % (block // Q) == 0, ctx
                            assert 1024 < table <= total <= LDS, ctx
                            assert (total > table) == (form in (2, 3, 4, 5)), ctx          # bitmaps behind the table
                            if form >= 2:
                                assert A == 32 and K == 4 and total == table + (block // 8) * ((((V + 31) // 32) * 4 + 15) & ~15), ctx
                            if form == 5:
                                assert delta, ctx
                            # launch bounds of the instances (mapf_lq_rollout.hip: 512 threads with eight agents per lane and for the
                            # in-kernel policy behind four 8-byte columns + bitmaps, 1024 otherwise)
                            assert block <= (512 if K == 8 or (form == 2 and not streamed) else 1024), ctx
    assert seen_forms == {0, 1, 2, 3, 4, 5} and n_packed > 50000, (seen_forms, n_packed)
    # the boundaries themselves (32 agents, default tuning), to the cell
    stride = lambda V: (((V + 31) // 32) * 4 + 15) & ~15                                   # noqa: E731  (bytes of one env's bitmap)
    for delta, streamed in ((1, 1), (0, 1), (0, 0)):
        forms = {V: plan(V, 32, 16384, streamed, delta, None) for V in range(3000, 4200)}
        last = max(V for V, (rc, _) in forms.items() if rc)
        assert 1024 + last * 40 <= LDS - 1024 < 1024 + (last + 1) * 40                     # the 8-byte rows' own limit (launcher's reserve kept)
        assert not any(rc for V, (rc, _) in forms.items() if V > last)
        five = [V for V, (rc, o) in forms.items() if rc and o[2] == 3]                     # five columns + 64 bitmaps
        four = [V for V, (rc, o) in forms.items() if rc and o[2] == 2]                     # four columns + 64 bitmaps
        if delta:
            assert not five and not four and all(o[2] == 5 for rc, o in forms.values() if rc)   # delta rows: 24 bytes a cell, fit to the end
        else:
            assert max(five) + 1 == min(four) and max(four) == last
            assert 1024 + max(five) * 40 + 64 * stride(max(five)) <= LDS < 1024 + (max(five) + 1) * 40 + 64 * stride(max(five) + 1)
            assert 1024 + last * 32 + 64 * stride(last) <= LDS
    # a malformed override is an error, not a default
    assert lib.mapf_debug_rollout_plan(683, 8, 65536, 64, 1, 0, 256, b'k=nine', out) < 0
    assert lib.mapf_debug_rollout_plan(683, 8, 65536, 64, 1, 0, 256, b'no_such_key=1', out) < 0
