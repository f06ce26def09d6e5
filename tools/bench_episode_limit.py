#!/usr/bin/env python3
"""Throughput of the fused rollout under an episode step limit (mapf_set_episode_limit) next to the same rollout without one, and
next to what a caller with a step budget had to do before: leave the fused rollout and loop on the host.  One JSON line.

    python tools/bench_episode_limit.py --label this --write profiles/episode_limit_bench.json      # on a MI355X
    python tools/bench_episode_limit.py --label parent --write profiles/episode_limit_bench.json    # on the commit before the
                                                                   # feature: only the legs that need no API newer than
                                                                   # set_policy('table') / prepare_step / graph_begin run there

Shape: BASELINE configs[2] (room-32-32-4, 8 agents, 65536 envs, slip 0.2), T = 256, the shortest-path table policy.  Each leg:
preroll, then HIP events around `launches` launches of T env-steps, median of `blocks` blocks; the legs of a run share ONE process
and alternate block by block.  --write merges the run into the file under its label, so the file holds both commits' runs.
  lg_unlimited     (a) the lane-group rollout without a limit (MAPF_TUNE=quad_lanes=0): the yardstick, taken on the parent commit
  packed_unlimited     the default dispatch without a limit (a packed kernel): what a limit form of the packed kernels would aim at
  limit_far        (b) N = 2^31: the limit instance runs and the limit is never reached
  limit_64         (c) N = 64
  limit_far_packed     (b) with MAPF_TUNE=limit_packed=1: the packed table instance's limit form (lq_rollout_kernel_table_limit)
  limit_64_packed      (c) likewise; both are skipped on a tree whose library does not know the key
  host_loop        (d) the loop the feature replaces, N = 64: T x (torch gather of the table actions, mapf_step with auto-reset, a
                       torch age update, mapf_reset(mask of the envs whose age reached N)), recorded into a hipGraph where that
                       works, else plain launches
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gym-mapf_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402  (initialise torch's HIP runtime first)
import bench  # noqa: E402
from bench_policy_table import bfs_table, make_env, time_legs  # noqa: E402
from gym_mapf_amd.envs.vec_env import VecMapfEnv  # noqa: E402

T, N_LIMIT, N_FAR = 256, 64, 1 << 31
HAS_LIMIT = hasattr(VecMapfEnv, 'set_episode_limit')
LEGS = {'lg_unlimited': ('quad_lanes=0', None), 'packed_unlimited': (None, None), 'limit_far': (None, N_FAR), 'limit_64': (None, N_LIMIT),
        'limit_far_packed': ('limit_packed=1', N_FAR), 'limit_64_packed': ('limit_packed=1', N_LIMIT)}


def has_limit_packed():
    """does the library know the MAPF_TUNE key limit_packed?  (asked of the planner's debug entry, which parses a tune string without a device)"""
    import ctypes
    from gym_mapf_amd import _native as nat
    lib = nat.load()
    if not HAS_LIMIT or not hasattr(lib, 'mapf_debug_rollout_plan_limited'):
        return False
    out = (ctypes.c_uint64 * 6)()
    return lib.mapf_debug_rollout_plan_limited(683, 8, 65536, T, 0, 1, 256, b'limit_packed=1', N_LIMIT, out) == 0


class RolloutLeg:
    """The fused rollout under the table policy: launch() enqueues T env-steps."""

    def __init__(self, kind, cfg, grid, start, goal, table, rows, record):
        self.kind, self.record = kind, record
        tune, limit = LEGS[kind]
        self.env = env = make_env(cfg, grid, start, goal, tune)
        env.set_policy('table', table=table, rows=rows)
        if limit:
            env.set_episode_limit(limit)
        self.out = env.rollout(T, auto_reset=True, record=record)
        env.sync()

    def launch(self):
        self.out = self.env.rollout(T, auto_reset=True, record=self.record, out=self.out)

    def kernel(self):
        return self.env.last_kernel('rollout')

    def extra(self):
        self.env.sync()
        if 'truncations' not in self.out:
            return {}
        return {'truncations_per_launch': int(self.out['truncations'].sum().item()), 'episodes_per_launch': int(self.out['episodes'].sum().item())}


class HostLoopLeg:
    """What a caller with a step budget did before the limit existed: per env-step the table gather, one mapf_step (auto-reset on
    done), its own age counter in torch, and a masked mapf_reset of the envs that ran out of budget."""

    def __init__(self, cfg, grid, start, goal, table, rows, record):
        self.kind, self.record = 'host_loop', record
        self.stream = stream = torch.cuda.Stream()                # the caller's stream: torch's kernels and the steps share it
        self.env = env = make_env(cfg, grid, start, goal, stream=stream.cuda_stream)
        E, A, V = env.n_envs, env.n_agents, table.shape[1]
        flat = torch.from_numpy(table.reshape(-1).copy()).cuda()
        base = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(rows.reshape(-1, A), (E, A))).astype(np.int64) * V).cuda()
        view = env.state_view()
        acts = torch.empty((E, A), dtype=torch.uint8, device='cuda')
        idx = torch.empty((E, A), dtype=torch.int64, device='cuda')
        age = torch.zeros((E,), dtype=torch.int32, device='cuda')
        over = torch.zeros((E,), dtype=torch.bool, device='cuda')
        mask = torch.zeros((E,), dtype=torch.uint8, device='cuda')
        ended = torch.zeros((E,), dtype=torch.bool, device='cuda')
        self.truncations = torch.zeros((E,), dtype=torch.int32, device='cuda')   # (every tensor exists before the recording: no allocation in it)
        torch.cuda.synchronize()
        call, out = env.prepare_step(acts, auto_reset=True, write_local=record)
        done = out['done']

        def before():
            with torch.cuda.stream(stream):
                idx.copy_(view)                                   # cell
                idx.add_(base)                                    # row * V + cell
                torch.take(flat, idx, out=acts)

        def after():
            with torch.cuda.stream(stream):
                age.add_(1)
                torch.ne(done, 0, out=ended)
                age.masked_fill_(ended, 0)                        # (the step's auto-reset began a new episode)
                torch.ge(age, N_LIMIT, out=over)
                age.masked_fill_(over, 0)
                mask.copy_(over)
                self.truncations.add_(over)
            env.reset(mask)

        self.graph, self.note = None, 'hipGraph of T x (torch gather + mapf_step + torch age update + mapf_reset(mask))'
        before(); call(); after(); env.sync()                     # warm: torch picks its kernels outside the recording
        try:
            env.graph_begin()
            for _ in range(T):
                before()
                call()
                after()
            self.graph = env.graph_end()
        except Exception as exc:                                  # noqa: BLE001  (the torch part could not be recorded on this box)
            self.note = 'plain launches (recording failed: %s)' % type(exc).__name__
            self.graph = None
        self._parts = (before, call, after)
        self.launch()
        env.sync()

    def launch(self):
        if self.graph is not None:
            self.graph.launch(1)
        else:
            before, call, after = self._parts
            for _ in range(T):
                before()
                call()
                after()

    def kernel(self):
        return self.env.last_kernel('step') + ' | ' + self.note

    def extra(self):
        self.env.sync()
        torch.cuda.synchronize()
        return {'truncations_total': int(self.truncations.sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', required=True, help="which commit runs: 'parent' or 'this' (the key of the run in the file)")
    ap.add_argument('--legs', default=None, help='comma list (default: every leg this checkout has the API for)')
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--preroll-ms', type=float, default=60.0)
    ap.add_argument('--write', default=None, help='merge the run into this file under its label')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_episode_limit.py needs a GPU')
    packed_limit = has_limit_packed()
    default = ['lg_unlimited', 'packed_unlimited'] + (['limit_far', 'limit_64'] if HAS_LIMIT else []) + \
              (['limit_far_packed', 'limit_64_packed'] if packed_limit else []) + ['host_loop']
    kinds = [k for k in (args.legs.split(',') if args.legs else default) if k and (packed_limit or not k.endswith('_packed'))]
    cfg = bench.CONFIGS['c3']
    E = 65536
    grid, _, nbr, start, goal = bench.workload_tables(cfg, E, 0)
    table, lookup = bfs_table(nbr, goal)
    rows = lookup[goal.astype(np.int64)].astype(np.uint16)
    A = cfg['agents']
    run = {'tool': 'bench_episode_limit', 'label': args.label, 'device': torch.cuda.get_device_name(0), 'T': T, 'limit': N_LIMIT, 'launches': args.launches,
           'blocks': args.blocks, 'unit': 'agent-steps/s', 'has_episode_limit': HAS_LIMIT, 'has_limit_packed': packed_limit,
           'workload': '%s: %s, %d agents, slip %g, %d envs, shortest-path table policy' % (cfg['baseline'], cfg['map'], A, cfg['fail_prob'], E)}
    for record in (False, True):
        legs = [HostLoopLeg(cfg, grid, start, goal, table, rows, record) if k == 'host_loop' else RolloutLeg(k, cfg, grid, start, goal, table, rows, record)
                for k in kinds]
        ms = time_legs(legs, args.launches, args.blocks, args.preroll_ms)
        res = {}
        for leg in legs:
            res[leg.kind] = dict({'value': float(T) * E * A / (ms[id(leg)] * 1e-3), 'ms_per_launch': ms[id(leg)], 'last_kernel': leg.kernel()}, **leg.extra())
        run['recording' if record else 'totals'] = res
        for leg in legs:
            if getattr(leg, 'graph', None) is not None:
                leg.graph.close()
            leg.env.close()
    print(json.dumps(run))
    if args.write:
        merged = {'tool': 'bench_episode_limit', 'runs': {}}
        if os.path.exists(args.write):
            with open(args.write) as f:
                merged = json.load(f)
        merged['runs'][args.label] = run
        with open(args.write, 'w') as f:
            f.write(json.dumps(merged, indent=1) + '\n')


if __name__ == '__main__':
    main()
