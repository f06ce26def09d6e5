"""Which kernel family takes a launch: route_rollout and route_step (csrc/mapf_plan.hip), the one statement of the routing order.

The lane-group sweep of tests/golden/plan_decisions.json records, for 1584 shapes x 8 launches on an MI355X, what took each launch of
a handle created with MAPF_FLAG_LANE_GROUP: a lane-group instance (its plan's fields) or a packed kernel ('-').  The route is asked
for every one of them on the CPU.  The rules that sweep does not reach -- the other two preferences, the episode limit and budget,
limit_packed -- are asserted over the shapes of the limit sweep.

The thread-per-env kernels are named by tpe_step_kernel_name / tpe_rollout_kernel_name.  tests/golden/tpe_kernel_names.json holds what
mapf_last_kernel said after a launch of every agent count these kernels exist for -- steps for A = 1..16 with and without caller
uniforms at a batch on each side of the block rule's 2^18 boundary, one-step rollouts for A = 1..6 with and without the table policy
at the smaller batch -- on an MI355X, from the library of the commit whose launchers still formatted these names themselves
(MAPF_HIP_LIB; generation_info.json says how):

    python tests/test_route.py --record-tpe-names [OUT.json]"""
import ctypes
import json
import os
import sys

import pytest

from conftest import GOLDEN
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import (AUTO, KERNEL_NAME_BYTES, LG, LG_MAPS, LG_PACKED, LG_ROLLOUTS, LG_STEPS, LIMIT_AGENTS, LIMIT_CELLS, LIMIT_ENVS, N_CU, PACKED, PREFER_LG,
                         PREFER_TPE, TPE, LaneGroupLauncher, launch_lq, lg_key, lg_shapes, lq_fixture, parse_lg_key, plan_fixture, planned_rollout_lg, planned_step_lg,
                         routed_rollout, routed_step)

FIXTURE_TPE = os.path.join(GOLDEN, 'tpe_kernel_names.json')
TPE_ENVS = (1 << 18, (1 << 18) + 1)                                    # the block rule: 64 threads up to 2^18 envs, 256 beyond
TPE_STEP_AGENTS, TPE_ROLLOUT_AGENTS = range(1, 17), range(1, 7)
PREFERENCES = {'auto': AUTO, 'thread_per_env': PREFER_TPE, 'lane_group': PREFER_LG}   # by VecMapfEnv's `kernel`


def test_routes_of_the_lane_group_sweep_are_the_recorded_ones(shim):  # noqa: F811
    """every launch of the recorded sweep (handles that prefer the lane-group family, 256 CUs, the table policy's table of V bytes, delta
    rows as every one of these empty maps of at most 127 rows has them): packed exactly where a packed kernel took the launch on the GPU,
    elsewhere lane-group with the very plan and name plan_rollout_lg / plan_step_lg give"""
    recorded = plan_fixture()
    rollouts, steps = recorded['plan_rollout_lg'], recorded['plan_step_lg']
    assert all(rows <= 127 for rows, _ in LG_MAPS)
    n, n_packed, wrong = 0, 0, []
    for tune, rows, cols, A, E in lg_shapes():
        key, V = lg_key(tune, rows * cols, A, E), rows * cols
        for (record, policy), want in zip(LG_ROLLOUTS, rollouts[key].split(' ')):
            family, out, name = routed_rollout(shim, V, A, E, PREFER_LG, policy, tune, record=record)
            n, n_packed = n + 1, n_packed + (want == LG_PACKED)
            if want == LG_PACKED:
                ok = family == PACKED and name.startswith('lq_rollout_kernel')
            else:
                code, grid, lds_bytes, lg_name = planned_rollout_lg(shim, tune, V, A, E, record, policy)
                L, full, mv, dense, block = out[:5]
                ok = family == LG and code == want and name == lg_name and out[5:] == (grid, lds_bytes, 0, 0) and \
                    code == '%d%s%s%s%d' % (L, 'F' if full else 'R', 'L' if mv else 'G', 'D' if dense else 'G', block)
            if not ok:
                wrong.append((key, record, policy, want, family, out, name))
        for uniforms, want in zip(LG_STEPS, steps[key].split(' ')):
            family, out, name = routed_step(shim, V, A, E, PREFER_LG, uniforms, tune)
            n, n_packed = n + 1, n_packed + (want == LG_PACKED)
            if want == LG_PACKED:
                ok = family == PACKED and name.startswith('lq_step_kernel')
            else:
                code, grid, lg_name = planned_step_lg(shim, A, E, uniforms)
                ok = family == LG and code == want and name == lg_name and out[3:] == (grid, 0, 0, 0, 0) and code == '%d%s%d' % (out[0], 'F' if out[1] else 'R', out[2])
            if not ok:
                wrong.append((key, 'step', uniforms, want, family, out, name))
    assert not wrong, '%d of %d launches are routed differently: %s' % (len(wrong), n, wrong[:8])
    assert n == 4 * 4 * 11 * 9 * 8 and 0 < n_packed <= n // 2, (n, n_packed)


RULE_AGENTS = tuple(sorted(set(LIMIT_AGENTS) | {6, 7}))               # ... and both sides of the thread-per-env rollouts' last agent count
RULE_TUNES = (None, b'limit_packed=1')


def test_routing_rules(shim):  # noqa: F811
    """the rules the recorded sweep does not reach, over the limit sweep's shapes, the three preferences, with and without limit_packed=1"""
    n_limit_packed, n_packed_steps, table_plan = 0, 0, (ctypes.c_uint64 * 9)()
    for A in RULE_AGENTS:
        for E in LIMIT_ENVS:
            for V in LIMIT_CELLS:
                for prefer in PREFERENCES.values():
                    ctx = (A, E, V, prefer)
                    prefers_tpe = prefer == PREFER_TPE or (prefer == AUTO and A <= 2)
                    for tune in RULE_TUNES:
                        for policy in (0, 1, 2):
                            # no limit, no budget: thread-per-env exactly where the handle prefers it and its rollout kernels exist (A <= 6)
                            family, out, name = routed_rollout(shim, V, A, E, prefer, policy, tune)
                            assert (family == TPE) == (prefers_tpe and A <= 6) and (family != TPE or out[:2] == (64, -(-E // 64))), ctx
                            # a budget, with or without a limit: the lane-group budget plan, whatever else holds
                            for limited in (0, 1):
                                family, out, name = routed_rollout(shim, V, A, E, prefer, policy, tune, budgeted=1, limited=limited)
                                assert family == LG and out[7:] == (1, 1) and out[3] == 0 and '_budget_guarded<' in name, ctx
                            # a limit: never thread-per-env; packed only with the table policy and limit_packed=1, without the lane-group flag
                            family, out, name = routed_rollout(shim, V, A, E, prefer, policy, tune, limited=1)
                            assert family != TPE, ctx
                            rc = shim.shim_plan_rollout_table(V, A, E, 1, 1, V, N_CU, tune, 1, table_plan, None)
                            allowed = policy == 2 and tune == b'limit_packed=1' and prefer != PREFER_LG
                            assert (family == PACKED) == (allowed and rc == 1), ctx
                            if family == PACKED:
                                n_limit_packed += 1
                                assert out == tuple(table_plan) and out[8] == 1 and '_table_limit<' in name, ctx
                            else:
                                assert out[7:] == (1, 0) and out[3] == 0 and '_limit_guarded<' in name, ctx
                    for uniforms in LG_STEPS:
                        family, out, name = routed_step(shim, V, A, E, prefer, uniforms)
                        assert (family == TPE) == (prefers_tpe and A <= 16) and (uniforms == 0 or family != PACKED), ctx
                        n_packed_steps += family == PACKED
                        family, out, name = routed_step(shim, V, A, E, prefer, uniforms, limited=1)
                        assert family == LG and out[4] == 1 and name.startswith('lg_step_kernel_limit<'), ctx
    assert n_limit_packed > 0 and n_packed_steps > 0, (n_limit_packed, n_packed_steps)


def tpe_launches():
    """(key, kind, A, E, caller uniforms or table policy) of the thread-per-env fixture"""
    for A in TPE_STEP_AGENTS:
        for E in TPE_ENVS:
            for uniforms in (0, 1):
                yield 'step A=%d E=%d uniforms=%d' % (A, E, uniforms), 'step', A, E, uniforms
    for A in TPE_ROLLOUT_AGENTS:
        for table in (0, 1):
            yield 'rollout A=%d E=%d table=%d' % (A, TPE_ENVS[0], table), 'rollout', A, TPE_ENVS[0], table


def test_thread_per_env_names_are_the_recorded_ones(shim):  # noqa: F811
    """plan_tpe and the two name functions (through the route of a handle that prefers thread-per-env) against what the launchers' own
    format strings printed on the GPU: byte for byte"""
    with open(FIXTURE_TPE) as f:
        recorded = json.load(f)['names']
    wanted = list(tpe_launches())
    assert sorted(recorded) == sorted(w[0] for w in wanted) and len(wanted) == 16 * 2 * 2 + 6 * 2
    for key, kind, A, E, flag in wanted:
        family, out, name = routed_step(shim, 100, A, E, PREFER_TPE, flag) if kind == 'step' else routed_rollout(shim, 100, A, E, PREFER_TPE, 2 if flag else 1)
        assert family == TPE and name == recorded[key] and len(name) < KERNEL_NAME_BYTES and out[:2] == (64 if E <= 1 << 18 else 256, -(-E // (64 if E <= 1 << 18 else 256))), \
            (key, name, recorded[key])
    assert len(set(recorded.values())) == 16 * 2 * 2 + 6 * 2


def record_tpe_names():
    """{'names': {key: full name}}: device-mode handles of the thread-per-env family on the empty 10 x 10 map, rows broadcast"""
    import numpy as np
    import torch
    from gym_mapf_amd.envs.grid import MapfGrid
    from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
    grid, names = MapfGrid(['.' * 10] * 10), {}
    actions = torch.zeros(max(TPE_ENVS) * 16, dtype=torch.uint8, device='cuda')
    uniforms = torch.full((max(TPE_ENVS) * 16,), 0.5, dtype=torch.float64, device='cuda')
    for A in TPE_STEP_AGENTS:
        for E in TPE_ENVS:
            env = VecMapfEnv(grid, A, None, None, 0.2, -1000.0, 100.0, -1.0, OptimizationCriteria.Makespan, n_envs=E, device_arrays=True,
                             start_local=np.arange(A), goal_local=np.arange(A) + 1, kernel='thread_per_env')
            try:
                for flag in (0, 1):
                    env.step(actions[:E * A].view(E, A), uniforms=uniforms[:E * A].view(E, A) if flag else None)
                    names['step A=%d E=%d uniforms=%d' % (A, E, flag)] = env.last_kernel('step')
                if A in TPE_ROLLOUT_AGENTS and E == TPE_ENVS[0]:
                    for flag in (0, 1):
                        if flag:
                            env.set_policy('table', table=np.zeros((1, 100), dtype=np.uint8), rows=np.zeros(A, dtype=np.uint16))
                        env.rollout(1)
                        names['rollout A=%d E=%d table=%d' % (A, E, flag)] = env.last_kernel('rollout')
                env.sync()
            finally:
                env.close()
        print('launched A=%d' % A, flush=True)
    assert sorted(names) == sorted(w[0] for w in tpe_launches())
    return {'names': names}


def smallest_packed(codes, index_of):
    """the smallest shape of the recorded sweep one of whose launches a packed kernel took: (key, the launch's index)"""
    found = [(A * E, key, codes[key].split(' ').index(LG_PACKED)) for key in codes for _, _, A, E in [parse_lg_key(key)] if LG_PACKED in codes[key].split(' ')]
    return min(found, key=lambda f: (f[0], index_of[f[1]]))[1:]


@pytest.mark.gpu
def test_every_route_branch_launches_what_the_route_names(shim):  # noqa: F811
    """one one-step launch per branch of the route, on the smallest shape that reaches it: mapf_last_kernel says the name the route
    gives for that shape with the device's CU count.  An empty handle (E = 0 is legal) launches nothing and notes nothing: the name
    noted before it stays in place"""
    import numpy as np
    import torch
    import episode_limit_cases as ec
    from gym_mapf_amd.envs.grid import MapfGrid
    from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
    n_cu, grid, V = torch.cuda.get_device_properties(0).multi_processor_count, MapfGrid(['.' * 10] * 10), 100

    def env_of(A, E, kernel):
        return VecMapfEnv(grid, A, None, None, 0.2, -1000.0, 100.0, -1.0, OptimizationCriteria.Makespan, n_envs=E, start_local=np.arange(A),
                          goal_local=np.arange(A) + 1, kernel=kernel)

    def launched(env, limited=0, budgeted=0):
        """the names of a one-step rollout (when `budgeted`: that alone -- such a handle takes no single step) and of a step after it"""
        A, E, prefer = env.n_agents, env.n_envs, PREFERENCES[env.kernel]
        env.rollout(1)
        found = [env.last_kernel('rollout')]
        want = [routed_rollout(shim, V, A, E, prefer, 1, n_cu=n_cu, limited=limited, budgeted=budgeted)]
        if not budgeted:
            env.step(np.zeros((E, A), np.uint8), auto_reset=True)
            found.append(env.last_kernel('step'))
            want.append(routed_step(shim, V, A, E, prefer, 0, n_cu=n_cu, limited=limited))
        return found, want

    last = None
    for A, E, kernel, families in ((2, 3, 'auto', [TPE, TPE]), (7, 5, 'thread_per_env', [LG, TPE]), (3, 63, 'lane_group', [LG, LG])):
        env = env_of(A, E, kernel)
        try:
            found, want = launched(env)
            assert found == [w[2] for w in want] and [w[0] for w in want] == families, (A, E, kernel, found, want)
            if kernel == 'lane_group':
                env.set_episode_limit(4)
                found, want = launched(env, limited=1)
                assert found == [w[2] for w in want] and all('_limit' in name and ',LIMIT> ' in name for name in found), (found, want)
                env.set_episode_limit(0)
                env.set_episode_budget(1)
                found, want = launched(env, limited=1, budgeted=1)
                assert found == [w[2] for w in want] and '_budget_guarded<' in found[0], (found, want)
                last = found[0]
        finally:
            env.close()
    empty = env_of(2, 0, 'auto')
    try:
        empty.rollout(1)
        empty.step(np.zeros((0, 2), np.uint8))
        assert empty.last_kernel('rollout') == empty.last_kernel('step') == last and empty.t == 2
    finally:
        empty.close()
    # packed rollout and packed step: the smallest shapes of the lane-group sweep whose fixture code is '-'
    recorded, launcher = plan_fixture(), LaneGroupLauncher()
    index_of = {lg_key(tune, rows * cols, A, E): i for i, (tune, rows, cols, A, E) in enumerate(lg_shapes())}
    for codes, kind in ((recorded['plan_rollout_lg'], 'rollout'), (recorded['plan_step_lg'], 'step')):
        key, i = smallest_packed(codes, index_of)
        tune, V_key, A, E = parse_lg_key(key)
        rows, cols = [m for m in LG_MAPS if m[0] * m[1] == V_key][0]
        rollout_names, step_names = launcher.names(tune, rows, cols, A, E)
        if kind == 'rollout':
            record, policy = LG_ROLLOUTS[i]
            family, _, name = routed_rollout(shim, V_key, A, E, PREFER_LG, policy, tune, n_cu=n_cu, record=record)
            assert family == PACKED and rollout_names[i] == name and A * E <= 32768, (key, i, rollout_names[i], name)
        else:   # (the step without caller uniforms, right after the launcher's auto-reset rollouts: no env can be terminal)
            family, _, name = routed_step(shim, V_key, A, E, PREFER_LG, 0, tune, n_cu=n_cu)
            assert i == 0 and family == PACKED and step_names[0] == name and A * E <= 32768, (key, i, step_names[0], name)
    # packed under a limit: the smallest case of tests/limit_packed_cases.py, as the packed-name fixture launches it
    launch = lq_fixture()['launches']['k2-4x512 lds=0 limit=1']
    found = launch_lq(ec.random_map(3), launch['A'], launch['E'], launch['tune'], 'TABLE', True, 'Makespan', [(True, False)])
    family, out, name = routed_rollout(shim, launch['V'], launch['A'], launch['E'], AUTO, 2, launch['tune'].encode(), table_bytes=launch['table_bytes'], n_cu=n_cu,
                                       limited=1)
    assert family == PACKED and out[8] == 1 and found == [name] and '_table_limit<' in name, (found, name)


if __name__ == '__main__':
    if len(sys.argv) < 2 or sys.argv[1] != '--record-tpe-names':
        sys.exit(__doc__)
    from gym_mapf_amd import _native
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE_TPE, 'w') as f:
        json.dump(record_tpe_names(), f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded the thread-per-env names from %s' % _native.LIB_PATH)
