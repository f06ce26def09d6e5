"""Host-side support of the tests, no test in it: the host shim -- the two host-only units (csrc/mapf_tables.hip, csrc/mapf_plan.hip)
compiled with a small C shim (tests/host_tables_shim.hip) into the run's tmp dir and driven through ctypes -- with its fixture, the
builders of the tables it returns, and the modules of tools/ the host tests read device listings with.  A plain module, not a
conftest: the `shim` fixture reaches a test module by `from host_shim import shim`."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
try:
    import device_listings  # noqa: F401
    import kernel_meta  # noqa: F401
    import compare_kernels  # noqa: F401
finally:
    sys.path.pop(0)

CSRC = os.path.join(ROOT, 'gym-mapf_amd', 'csrc')
SLIP = np.dtype([('q', '<f8', 3), ('th', '<u4', 3), ('n', '<u4'), ('thr', '<u8', 3), ('cum', '<f8', 3), ('th_biased', '<u4'), ('members', '<u4')])
OUTCOME = np.dtype([('reward', '<f8'), ('status', '<u4'), ('pad', '<u4')])


_SHIM = []      # built once per run, whichever module asks first


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if not _SHIM:
        _SHIM.append(load_shim(build_shim(tmp_path_factory.mktemp('host_tables'))))
    return _SHIM[0]


def build_shim(out_dir, csrc=CSRC):
    out = os.path.join(str(out_dir), 'libhost_tables_shim.so')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-shared', '-I' + os.path.join(ROOT, 'include'),
           '-I' + csrc, os.path.join(ROOT, 'tests', 'host_tables_shim.hip'), os.path.join(csrc, 'mapf_tables.hip'),
           os.path.join(csrc, 'mapf_plan.hip'), '-o', out]                          # (the Makefile's flags: no FMA contraction)
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert proc.returncode == 0, proc.stdout.decode('utf-8', 'replace')[-3000:]
    return out


def load_shim(path):
    lib = ctypes.CDLL(path)
    lib.shim_slip_tables.argtypes = [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.shim_outcome_rows.argtypes = [ctypes.c_double] * 3 + [ctypes.c_void_p]
    lib.shim_outcome_status.argtypes = [ctypes.c_uint32]
    lib.shim_outcome_status.restype = ctypes.c_uint32
    lib.shim_sizes.argtypes = [ctypes.c_uint32, ctypes.c_void_p]
    lib.shim_move_tables.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 3
    lib.shim_scen_table.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.shim_scen_table.restype = ctypes.c_uint32
    lib.shim_greedy_cells.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.shim_plan_step.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p]
    lib.shim_plan_rollout_table.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.shim_lq_rollout_name.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p] + \
        [ctypes.c_int] * 5 + [ctypes.c_char_p]
    lib.shim_table_instance_count.argtypes = [ctypes.c_int]
    if hasattr(lib, 'shim_plan_rollout_lg'):
        lib.shim_plan_rollout_lg.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p]
        lib.shim_plan_step_lg.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p]
    if hasattr(lib, 'shim_plan_limit_rollout_lg'):
        lib.shim_plan_limit_rollout_lg.argtypes = lib.shim_plan_rollout_lg.argtypes
        lib.shim_plan_limit_step_lg.argtypes = lib.shim_plan_step_lg.argtypes
    if hasattr(lib, 'shim_rollout_instance_exists'):
        lib.shim_rollout_instance_exists.argtypes = [ctypes.c_int] * 4
    if hasattr(lib, 'shim_step_instance_exists'):
        lib.shim_step_instance_exists.argtypes = [ctypes.c_int] * 3
        lib.shim_lq_step_name.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_char_p]
    if hasattr(lib, 'shim_route_rollout'):
        lib.shim_route_rollout.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p] + \
            [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_char_p]
        lib.shim_route_step.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p] + [ctypes.c_int] * 5 + \
            [ctypes.c_void_p, ctypes.c_char_p]
    return lib


def sizes(lib, V):
    out = np.zeros(6, np.uint64)
    lib.shim_sizes(V, out.ctypes.data)
    mv_cols, delta_cols, row_bias, slip_bytes, outcome_bytes, delta_words = (int(x) for x in out)
    assert slip_bytes == SLIP.itemsize and outcome_bytes == OUTCOME.itemsize and 8 * slip_bytes + 16 * outcome_bytes == 1024
    return mv_cols, delta_cols, row_bias, delta_words


def slip_rows(lib, fail_prob):
    rows = np.zeros(8, SLIP)
    p_cand, flags = np.zeros(3), np.zeros(2, np.uint32)
    assert lib.shim_slip_tables(fail_prob, rows.ctypes.data, p_cand.ctypes.data, flags.ctypes.data) == 1
    return rows, p_cand, flags


def move_tables(lib, nbr, fail_prob):
    V = len(nbr)
    mv_cols, delta_cols, row_bias, delta_words = sizes(lib, V)
    mv, mv8, mv4 = np.zeros((V, mv_cols, 4), np.uint32), np.zeros((V, mv_cols, 2), np.uint32), np.zeros(delta_words, np.uint32)
    nbr = np.ascontiguousarray(nbr, np.uint16)
    delta8 = lib.shim_move_tables(nbr.ctypes.data, V, fail_prob, mv.ctypes.data, mv8.ctypes.data, mv4.ctypes.data)
    assert delta8 in (0, 1)
    return mv, mv8, (mv4 if delta8 else None)


def step_instances(lib):
    """the (Q, K, form) of MAPF_LQ_STEP_INSTANCES (csrc/mapf_layout.hpp): the list the planner asks and the launcher walks"""
    return {(Q, K, form) for K in (2, 4, 8) for Q in range(1, 17) for form in range(4) if lib.shim_step_instance_exists(K, Q, form) == 1}
