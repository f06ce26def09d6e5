"""The planner tests' shared side, no test in it: the sweeps the launch planners (csrc/mapf_plan.hip) are asked over, the numbers of
the planner's enums, the recorded fixtures' paths and readers, and the helpers that ask a planner through the host shim
(tests/host_shim.py) or launch a shape on the GPU and read mapf_last_kernel.  What only one test module uses stays in that module."""
import ctypes
import json
import os

from conftest import GOLDEN

# the sweep of plan_rollout_lq (tests/test_cabi_and_host.py holds its invariants, tests/test_plan_decisions.py digests it, and more)
ROLLOUT_PLAN_CELLS = sorted(set(list(range(2, 200, 7)) + list(range(600, 760, 3)) + list(range(800, 1800, 11)) + list(range(1650, 1720)) +
                                list(range(3000, 3400, 5)) + list(range(4000, 20500, 61)) + list(range(19700, 20300, 3)) + [683, 3278, 4097, 65535]))
ROLLOUT_PLAN_TUNES = [None, b'k=8', b'k=4', b'k=2', b'bitmap_block=1024', b'bitmap_block=512', b'bitmap_pairs=0', b'bitmap_delta=0',
                      b'bitmap_staycol=0', b'mv_lds_max_bytes=163840', b'mv_lds_max_bytes=0', b'quad_min_lanes=0,oct_min_lanes=0']
ROLLOUT_PLAN_AGENTS = (2, 4, 8, 16, 32, 64, 128)
ROLLOUT_PLAN_ENVS = (64, 1000, 1024, 4096, 16384, 16448, 65536, 131072, 262144)

# the sweep of plan_step_lq (tests/test_host_tables.py holds its invariants, tests/test_plan_decisions.py digests it)
STEP_PLAN_CELLS = sorted(set(list(range(2, 200, 13)) + list(range(600, 900, 17)) + list(range(3000, 3400, 23)) + list(range(4000, 7200, 97)) +
                             [682, 683, 852, 853, 3294, 3648, 6783, 6784, 6785, 14818, 47540, 65535]))
STEP_PLAN_TUNES = [None, b'step_big=2', b'step_big=0', b'step_delta=2', b'step_delta=0', b'step_big=2,step_delta=2', b'k=2', b'k=4',
                   b'step_block=512', b'step_block=64', b'bitmap_pairs=0', b'quad_lanes=0']
STEP_PLAN_CUS = (256, 8)
STEP_PLAN_AGENTS = (2, 3, 4, 6, 8, 16, 32, 64, 128)
STEP_PLAN_ENVS = (0, 1, 64, 1000, 1024, 4096, 16384, 65536, 131072, 262144, 1 << 20, 1 << 22)

FIXTURE = os.path.join(GOLDEN, 'plan_decisions.json')
TABLE_AGENTS, TABLE_ENVS = (4, 8, 16, 32, 64), (1024, 16384, 65536, 262144)
TABLE_BYTES = (1, 8, 64)                                               # policy tables of V, 8 V and 64 V action bytes
TABLE_TUNES = (None, b'policy_table_lds=0', b'policy_table_lds=1')
# the lane-group sweep: the smallest shapes at which each rule can go wrong -- odd teams and every group size; batches around one
# wave, the 64 * 256 threads the LDS table needs, the 2^17 threads of the four-wave block and whole / ragged blocks; maps whose
# move table leaves >= 4, 2, 2 and 1 copies per CU (the last only with the limit lifted)
LG_AGENTS = (1, 2, 3, 5, 8, 16, 17, 31, 32, 33, 128)
LG_ENVS = (1, 63, 64, 257, 4096, 8191, 8192, 16384, 65536)
LG_MAPS = ((10, 10), (22, 31), (25, 40), (30, 50))                     # empty maps of 100, 682, 1000 and 1500 free cells
LG_TUNES = (None, b'quad_lanes=0', b'quad_lanes=0,mv_lds_max_bytes=163840', b'mv_lds_max_bytes=0')
LG_ROLLOUTS = tuple((record, policy) for record in (0, 1) for policy in (0, 1, 2))   # policy: streamed actions, policy stream, table policy
LG_STEPS = (0, 1)                                                      # caller uniforms
LG_PACKED = '-'
# the limit instances: every L, full and ragged; one-wave and four-wave blocks, MV_GLOBAL and MV_LDS, ragged and full last blocks; a
# table of 4 copies per CU, of 2, and one no LDS holds
LIMIT_AGENTS = (1, 2, 3, 5, 8, 16, 17, 32, 33, 64, 128)
LIMIT_ENVS = (1, 63, 64, 4096, 65536)
LIMIT_CELLS = (16, 683, 3300)
KERNEL_NAME_BYTES = 160                                                # what mapf_last_kernel keeps of a name (the terminator included)
# the packed names: every launch on the 20 x 20 map of the limit cases (V = 341, delta rows present), a table of LQ_TABLE_ROWS rows
FIXTURE_LQ_NAMES = os.path.join(GOLDEN, 'lq_kernel_names.json')
LQ_TABLE_ROWS = 64
# the packed step's names: every instance on the same map at the smallest batch of full blocks its form accepts -- the plain step in
# one-wave blocks (two agents per lane: k=2), the LDS-table form in its 1024-thread blocks (eight agents per lane unless k=4), the
# delta-row forms in 512-thread blocks
FIXTURE_LQ_STEP_NAMES = os.path.join(GOLDEN, 'lq_step_kernel_names.json')
STEP_FORMS = ('Plain', 'FullRows', 'DeltaRows', 'DeltaRowsBitmap')   # StepForm's numbers (csrc/mapf_layout.hpp)
LQ_STEP_LAUNCHES = {'%s-K%d-Q%d' % (STEP_FORMS[form], K, Q): (form, K, Q, E, tune) for form, K, Q, E, tune in
                    [(0, 4, Q, max(64, 512 // Q), '') for Q in (1, 2, 4, 8, 16)] + [(0, 2, Q, max(64, 512 // Q), 'k=2') for Q in (2, 4, 8, 16)] +
                    [(1, 4, Q, 1024 // Q, 'step_big=2,k=4') for Q in (1, 2, 4, 8)] + [(1, 8, Q, 1024 // Q, 'step_big=2') for Q in (1, 2, 4)] +
                    [(2, 4, Q, 512 // Q, 'step_delta=2,bitmap_pairs=0') for Q in (1, 2, 4, 8)] + [(3, 4, 8, 64, 'step_delta=2')]}


def tune_name(tune):
    return tune.decode() if tune else 'default'


def lg_key(tune, V, A, E):
    return '%s V=%d A=%d E=%d' % (tune_name(tune), V, A, E)


def lg_shapes():
    for tune in LG_TUNES:
        for rows, cols in LG_MAPS:
            for A in LG_AGENTS:
                for E in LG_ENVS:
                    yield tune, rows, cols, A, E


def parse_lg_key(key):
    tune, V, A, E = key.split(' ')
    return (None if tune == 'default' else tune.encode()), int(V[2:]), int(A[2:]), int(E[2:])


def planned_rollout_lg(shim_lib, tune, V, A, E, record, policy):
    """plan_rollout_lg through the shim: (code, grid, lds_bytes, the name the launcher notes)"""
    out, name = (ctypes.c_uint64 * 7)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    rc = shim_lib.shim_plan_rollout_lg(V, A, E, record, policy, tune, out, name)
    assert rc == 1, (rc, tune)
    L, full, mv_lds, dense, block, grid, lds_bytes = out
    return '%d%s%s%s%d' % (L, 'F' if full else 'R', 'L' if mv_lds else 'G', 'D' if dense else 'G', block), grid, lds_bytes, name.value.decode()


def planned_step_lg(shim_lib, A, E, uniforms):
    out, name = (ctypes.c_uint64 * 4)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    assert shim_lib.shim_plan_step_lg(A, E, uniforms, out, name) == 1
    L, full, block, grid = out
    return '%d%s%d' % (L, 'F' if full else 'R', block), grid, name.value.decode()


# the route (route_rollout, route_step: tests/test_route.py has their tests)
AUTO, PREFER_TPE, PREFER_LG = 0, 1, 2                                  # FamilyPreference's numbers (csrc/mapf_kernels.hpp)
TPE, PACKED, LG = 0, 1, 2                                              # KernelFamily's numbers (csrc/mapf_plan.hpp)
N_CU = 256                                                             # the MI355X the fixtures were recorded on


def routed_rollout(shim_lib, V, A, E, prefer, policy, tune=None, *, delta=1, table_bytes=None, n_cu=N_CU, limited=0, budgeted=0, record=0, soc=0, term=0):
    """route_rollout over a one-step launch, through the shim: (family, the plan's nine fields, the name its launcher notes)"""
    out, name = (ctypes.c_uint64 * 9)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    table_bytes = (V if policy == 2 else 0) if table_bytes is None else table_bytes
    family = shim_lib.shim_route_rollout(V, A, E, delta, table_bytes, n_cu, tune, prefer, policy, limited, budgeted, record, soc, term, out, name)
    assert family in (TPE, PACKED, LG), (family, tune)
    return family, tuple(out), name.value.decode()


def routed_step(shim_lib, V, A, E, prefer, uniforms, tune=None, *, delta=1, n_cu=N_CU, limited=0, scen=0, term=0):
    out, name = (ctypes.c_uint64 * 8)(), ctypes.create_string_buffer(2 * KERNEL_NAME_BYTES)
    family = shim_lib.shim_route_step(V, A, E, delta, n_cu, tune, prefer, limited, uniforms, scen, term, out, name)
    assert family in (TPE, PACKED, LG), (family, tune)
    return family, tuple(out), name.value.decode()


def tuned_env(grid, A, E, tune, criteria, start, goal):
    """a handle created under MAPF_TUNE = `tune` (read when the handle is created)"""
    from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
    outer_tune = os.environ.pop('MAPF_TUNE', None)
    os.environ['MAPF_TUNE'] = tune
    try:
        return VecMapfEnv(grid, A, None, None, 0.2, -1000.0, 100.0, -1.0, OptimizationCriteria[criteria], n_envs=E, start_local=start, goal_local=goal)
    finally:
        os.environ.pop('MAPF_TUNE', None)
        if outer_tune is not None:
            os.environ['MAPF_TUNE'] = outer_tune


def launch_lq(grid, A, E, tune, policy, limited, criteria, runs):
    """a handle of that shape under `tune`, and the names of its one-step rollouts `runs` = [(auto_reset, record), ...]"""
    import numpy as np
    V = len(grid.tables()[0])
    env = tuned_env(grid, A, E, tune, criteria, np.arange(A), np.arange(A) + 1)
    try:
        if policy == 'TABLE':
            env.set_policy('table', table=np.zeros((LQ_TABLE_ROWS, V), np.uint8), rows=np.zeros(A, np.uint16))
        if limited:
            env.set_episode_limit(4)
        names = []
        for auto_reset, record in runs:
            env.rollout(1, actions=np.zeros((1, E, A), np.uint8) if policy == 'STREAM' else None, auto_reset=auto_reset, record=record)
            names.append(env.last_kernel('rollout'))
        return names
    finally:
        env.close()


class LaneGroupLauncher:
    """Launches the shapes of the lane-group sweep on the GPU and reads mapf_last_kernel: device-mode handles of the lane-group
    family on empty maps, rows broadcast, inputs shared by all shapes."""

    def __init__(self):
        import numpy as np
        import torch
        from gym_mapf_amd.envs.grid import MapfGrid
        from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
        self.np, self.torch, self.make_grid, self.make_env, self.criteria = np, torch, MapfGrid, VecMapfEnv, OptimizationCriteria.Makespan
        n = max(LG_ENVS) * max(LG_AGENTS)
        self.actions = torch.zeros(n, dtype=torch.uint8, device='cuda')
        self.uniforms = torch.full((n,), 0.5, dtype=torch.float64, device='cuda')
        self.grids = {}

    def names(self, tune, rows, cols, A, E):
        """the kernel names of the shape's six one-step rollouts (LG_ROLLOUTS) and two steps (LG_STEPS)"""
        np, outer_tune = self.np, os.environ.pop('MAPF_TUNE', None)
        if tune:
            os.environ['MAPF_TUNE'] = tune.decode()             # (read when the handle is created)
        if (rows, cols) not in self.grids:
            self.grids[rows, cols] = self.make_grid(['.' * cols] * rows)
        V = rows * cols
        env = self.make_env(self.grids[rows, cols], A, None, None, 0.2, -1000.0, 100.0, -1.0, self.criteria, n_envs=E, device_arrays=True,
                            start_local=np.arange(A) % V, goal_local=(np.arange(A) + 1) % V, kernel='lane_group')
        try:
            rollouts = {}
            for table in (False, True):
                if table:
                    env.set_policy('table', table=np.zeros((1, V), dtype=np.uint8), rows=np.zeros(A, dtype=np.uint16))
                for record, policy in LG_ROLLOUTS:
                    if (policy == 2) == table:
                        env.rollout(1, actions=self.actions[:E * A].view(1, E, A) if policy == 0 else None, record=bool(record))
                        rollouts[record, policy] = env.last_kernel('rollout')
            steps = []
            for uniforms in LG_STEPS:
                env.step(self.actions[:E * A].view(E, A), uniforms=self.uniforms[:E * A].view(E, A) if uniforms else None)
                steps.append(env.last_kernel('step'))
            env.sync()
        finally:
            env.close()
            os.environ.pop('MAPF_TUNE', None)
            if outer_tune is not None:
                os.environ['MAPF_TUNE'] = outer_tune
        return [rollouts[r] for r in LG_ROLLOUTS], steps


def plan_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def lq_fixture():
    with open(FIXTURE_LQ_NAMES) as f:
        return json.load(f)


def lq_step_fixture():
    with open(FIXTURE_LQ_STEP_NAMES) as f:
        return json.load(f)


# ---------------------------------------------------------------- the plan of an env.P[s][a] call (tests/test_transitions_plan.py has its tests)
_PLAN_FIELDS = ('wide', 'max_a', 'all_out', 'qw_log2', 'pieces_max', 'rows_per_wave', 'unscanned_blocks', 'lanes_log2', 'walks', 'chunk', 'chunks_per_query',
                'scan_passes', 'scan_blocks', 'block', 'grid', 'lds_bytes')


def declare(lib):
    shape = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
    lib.shim_plan_transitions.argtypes = shape + [ctypes.c_void_p]
    lib.shim_transitions_kernel_name.argtypes = shape + [ctypes.c_char_p]
    lib.shim_transitions_wave_lds_bytes.argtypes = [ctypes.c_int, ctypes.c_uint32]
    lib.shim_transitions_wave_lds_bytes.restype = ctypes.c_uint64
    lib.shim_transitions_scan_blocks.argtypes = [ctypes.c_uint64]
    lib.shim_transitions_scan_blocks.restype = ctypes.c_uint64
    return lib


_out, _name = (ctypes.c_uint64 * 16)(), ctypes.create_string_buffer(KERNEL_NAME_BYTES)


def planned(lib, shape):
    """(plan as a dict, name), or (None, None) where the planner declines"""
    if lib.shim_plan_transitions(*shape, _out) != 1:
        assert lib.shim_transitions_kernel_name(*shape, _name) == 0
        return None, None
    assert lib.shim_transitions_kernel_name(*shape, _name) == 1
    return dict(zip(_PLAN_FIELDS, _out)), _name.value.decode()
