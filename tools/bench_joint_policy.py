#!/usr/bin/env python3
"""What the joint table policy (mapf_set_policy_joint) costs and what it buys -- every leg in ONE process, the legs alternating block
by block.  One JSON line.

    python tools/bench_joint_policy.py --write profiles/joint_policy_bench.json    # on a MI355X

Method of tools/bench_conflict_pairs.py: preroll, then HIP events around `launches` launches, `blocks` blocks per leg (median, with
min and max: the session's spread).  The shape is the README's evaluation shape: BASELINE configs[2] (room-32-32-4, 8 agents, 65536
envs, slip 0.2) with limit 64 and budget 8; a `launch` is one evaluation -- re-arm, reset, two launches of 256 steps accumulated into
one set of totals.  The plan is the shortest-path plan with k agent pairs -- (0, 1), (2, 3), ... -- merged and replanned by
policies.pair_shortest_path_rows, per scenario (the batch has six distinct goal rows: a pair's two [V, V] arrays per scenario).
  (0) table_k0     k = 0 under set_policy('table'): the kernel of the commit before the mode, the price's baseline;
  (1) joint_k1     k = 1 under set_policy('joint');
  (2) joint_k4     k = 4, every agent merged;
  (3) host_loop_k4 the only route to the k = 4 plan without the mode: a replayed hipGraph of 256 x (torch gather of the joint action +
                   mapf_step + torch's age, episode and totals updates + mapf_reset(mask)), twice per evaluation, as
                   tools/bench_episode_limit.py builds its host loop; its torch code parks an env after 8 episodes as the budget does.
Before anything is timed, (3)'s totals are compared with (2)'s: they must be equal."""
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
from bench_policy_table import bfs_table, make_env  # noqa: E402
from gym_mapf_amd import _native as nat  # noqa: E402
from gym_mapf_amd.envs import policies  # noqa: E402

T, N_LIMIT, B_EVAL = 256, 64, 8
N_LAUNCHES = -(-B_EVAL * N_LIMIT // T)


def joint_plan(grid, goal, table, lookup, k):
    """(table u8 [N], offsets u32 [E, A], partners u16 [E, A]): the shortest-path plan with pairs (0, 1) .. (2k - 2, 2k - 1) merged, one
    policies.join_plan per distinct goal row, the tables concatenated"""
    E, A = goal.shape
    V = table.shape[1]
    rows, scen = np.unique(goal, axis=0, return_inverse=True)
    scen = scen.reshape(-1)
    parts, offs, partners, at = [], [], None, 0
    for g in rows:
        solo = {i: table[lookup[int(g[i])]] for i in range(2 * k, A)}
        pairs = {(2 * p, 2 * p + 1): policies.pair_shortest_path_rows(grid, g[2 * p], g[2 * p + 1]) for p in range(k)}
        t, o, partners = policies.join_plan(V, A, solo, pairs)
        parts.append(t)
        offs.append(o.astype(np.int64) + at)
        at += t.size
    return np.concatenate(parts), np.stack(offs)[scen].astype(np.uint32), np.ascontiguousarray(np.broadcast_to(partners, (E, A)))


class Leg:
    """a fused evaluation: launch() enqueues re-arm, reset and the two accumulated launches"""

    def __init__(self, kind, work, policy):
        self.kind = kind
        cfg, grid, start, goal = work
        self.env = env = make_env(cfg, grid, start, goal)
        env.set_policy(**policy)
        self.table_bytes = int(np.asarray(policy['table']).size)
        env.set_episode_limit(N_LIMIT)
        env.set_episode_budget(B_EVAL)
        self.out = env.rollout(T, auto_reset=True)
        self.launch()
        env.sync()

    def launch(self):
        env = self.env
        env.set_episode_budget(B_EVAL)
        env.reset()
        env.set_state(t=0)
        env.set_episode_limit(N_LIMIT)
        self.out = env.rollout(T, auto_reset=True, out=self.out)
        for _ in range(N_LAUNCHES - 1):
            env.rollout(T, auto_reset=True, accumulate_into=self.out)

    def totals(self):
        self.env.sync()
        return {k: self.out[k].cpu().numpy() for k in ('returns', 'episodes', 'collisions', 'truncations', 'live_steps')}

    def extra(self):
        tot = self.totals()
        return {'last_kernel': self.env.last_kernel('rollout'), 'policy_table_bytes': self.table_bytes,
                'collisions_per_launch': int(tot['collisions'].sum()), 'goal_ends_per_launch': int(tot['episodes'].sum() - tot['collisions'].sum()),
                'truncations_per_launch': int(tot['truncations'].sum())}


class HostLoopLeg:
    """(3): per env-step the torch gather of the joint action, one mapf_step (auto-reset on done), the caller's own ages, episode
    counts and totals in torch, and a masked mapf_reset of the envs that ran out of steps"""

    def __init__(self, kind, work, plan):
        self.kind = kind
        cfg, grid, start, goal = work
        table, offsets, partners = plan
        self.table_bytes = int(table.size)
        self.stream = stream = torch.cuda.Stream()                # the caller's stream: torch's kernels and the steps share it
        self.env = env = make_env(cfg, grid, start, goal, stream=stream.cuda_stream)
        E, A, V = env.n_envs, env.n_agents, len(grid.tables()[0])
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
        flat, base, part = dev(table, np.uint8), dev(offsets, np.int64), dev(partners, np.int64)
        stride = dev(np.where(partners != np.arange(A)[None, :], V, 0), np.int64)
        view = env.state_view()
        acts = torch.empty((E, A), dtype=torch.uint8, device='cuda')
        cell, other, idx = (torch.empty((E, A), dtype=torch.int64, device='cuda') for _ in range(3))
        age = torch.zeros((E,), dtype=torch.int32, device='cuda')
        self.left = left = torch.zeros((E,), dtype=torch.int32, device='cuda')
        over, ended, live, hit = (torch.zeros((E,), dtype=torch.bool, device='cuda') for _ in range(4))
        mask = torch.zeros((E,), dtype=torch.uint8, device='cuda')
        hit_i = torch.zeros((E,), dtype=torch.int32, device='cuda')
        gain = torch.zeros((E,), dtype=torch.float64, device='cuda')
        self.tot = tot = {'returns': torch.zeros((E,), dtype=torch.float64, device='cuda')}
        for key in ('episodes', 'collisions', 'truncations', 'live_steps'):
            tot[key] = torch.zeros((E,), dtype=torch.int32, device='cuda')   # (every tensor exists before the recording: no allocation in it)
        self.age = age
        torch.cuda.synchronize()
        call, out = env.prepare_step(acts, auto_reset=True, write_local=False)
        done, coll, reward = out['done'], out['collision'], out['reward']

        def before():
            with torch.cuda.stream(stream):
                cell.copy_(view)
                torch.gather(cell, 1, part, out=other)            # the partner's cell (a solo agent: its own)
                torch.mul(cell, stride, out=idx)                  # offset + cell * (V | 0) + partner's cell
                idx.add_(other)
                idx.add_(base)
                torch.take(flat, idx, out=acts)
                torch.gt(left, 0, out=live)                       # the envs the budget has not parked

        def after():
            with torch.cuda.stream(stream):
                age.add_(1)
                torch.ne(done, 0, out=ended)
                age.masked_fill_(ended, 0)                        # (the step's auto-reset began a new episode)
                torch.ge(age, N_LIMIT, out=over)
                age.masked_fill_(over, 0)
                mask.copy_(over)
                torch.mul(reward, live, out=gain)
                tot['returns'].add_(gain)
                tot['live_steps'].add_(live)
                torch.logical_and(ended, live, out=hit)
                hit_i.copy_(hit)
                tot['episodes'].add_(hit_i)
                left.sub_(hit_i)                                  # an episode ends with done or truncated: one off the env's budget
                torch.logical_and(over, live, out=hit)
                hit_i.copy_(hit)
                tot['truncations'].add_(hit_i)
                left.sub_(hit_i)
                torch.ne(coll, 0, out=hit)
                hit.logical_and_(live)
                tot['collisions'].add_(hit)
            env.reset(mask)

        self.note = 'hipGraph of %d x (torch gather of the joint action + mapf_step + torch ages / episode counts / totals + mapf_reset(mask))' % T
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
        env = self.env
        env.reset()
        env.set_state(t=0)
        with torch.cuda.stream(self.stream):
            self.age.zero_()
            self.left.fill_(B_EVAL)
            for v in self.tot.values():
                v.zero_()
        for _ in range(N_LAUNCHES):
            if self.graph is not None:
                self.graph.launch(1)
            else:
                before, call, after = self._parts
                for _ in range(T):
                    before()
                    call()
                    after()

    def totals(self):
        self.env.sync()
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.tot.items()}

    def extra(self):
        return {'last_kernel': self.env.last_kernel('step') + ' | ' + self.note, 'policy_table_bytes': self.table_bytes}


def time_legs(legs, launches, blocks, preroll_ms):
    """ms per launch of every leg, one value per block; the legs alternate block by block"""
    for leg in legs:
        t_end = time.perf_counter() + preroll_ms * 1e-3
        while time.perf_counter() < t_end:
            leg.launch()
            leg.env.sync()
    ms = {id(leg): [] for leg in legs}
    for _ in range(blocks):
        for leg in legs:
            leg.env.sync()
            torch.cuda.synchronize()
            leg.env.timer_begin()
            for _ in range(launches):
                leg.launch()
            ms[id(leg)].append(leg.env.timer_end() / launches)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--preroll-ms', type=float, default=60.0)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--write', default=None, help='also write the result to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_joint_policy.py needs a GPU')
    cfg, E = bench.CONFIGS['c3'], args.envs
    A = cfg['agents']
    grid, _, nbr, start, goal = bench.workload_tables(cfg, E, 0)
    table, lookup = bfs_table(nbr, goal)
    rows = lookup[goal.astype(np.int64)].astype(np.uint16)
    work = (cfg, grid, start, goal)
    plans = {k: joint_plan(grid, goal.astype(np.int64), table, lookup, k) for k in (1, A // 2)}
    joint = lambda k: dict(policy='joint', table=plans[k][0], offsets=plans[k][1], partners=plans[k][2])
    legs = [Leg('table_k0', work, dict(policy='table', table=table, rows=rows)), Leg('joint_k1', work, joint(1)), Leg('joint_k4', work, joint(A // 2)),
            HostLoopLeg('host_loop_k4', work, plans[A // 2])]
    fused, loop = legs[2].totals(), legs[3].totals()
    same = all(np.array_equal(fused[k], loop[k].astype(fused[k].dtype)) for k in fused)
    assert same, 'the host loop must reach the totals of the fused evaluation: %r' % {k: (int(fused[k].sum()), int(loop[k].sum())) for k in fused}
    ms = time_legs(legs, args.launches, args.blocks, args.preroll_ms)
    run = {'tool': 'bench_joint_policy', 'device': torch.cuda.get_device_name(0), 'T': T, 'limit': N_LIMIT, 'budget': B_EVAL, 'launches': args.launches,
           'blocks': args.blocks, 'unit': 'agent-steps/s (value), ms per launch (ms_*)', 'this': nat.version(),
           'workload': '%s: %s, %d agents, slip %g, %d envs, V = %d, shortest-path plan with k pairs merged, limit %d, budget %d' % (
               cfg['baseline'], cfg['map'], A, cfg['fail_prob'], E, table.shape[1], N_LIMIT, B_EVAL),
           'host_loop_totals_equal_joint_k4': same}
    for leg in legs:
        v = sorted(ms[id(leg)])
        med = v[(len(v) - 1) // 2]
        run[leg.kind] = dict({'value': float(T * N_LAUNCHES) * E * A / (med * 1e-3), 'ms_per_launch': med, 'ms_min': v[0], 'ms_max': v[-1],
                              'steps_per_launch': T * N_LAUNCHES}, **leg.extra())
    t0, j1, j4, loop = (run[k]['ms_per_launch'] for k in ('table_k0', 'joint_k1', 'joint_k4', 'host_loop_k4'))
    run['ratios'] = {'joint_k1_ms_over_table_k0_ms': j1 / t0, 'joint_k4_ms_over_table_k0_ms': j4 / t0, 'host_loop_k4_ms_over_joint_k4_ms': loop / j4}
    for leg in legs:
        if getattr(leg, 'graph', None) is not None:
            leg.graph.close()
        leg.env.close()
    print(json.dumps(run))
    if args.write:
        with open(args.write, 'w') as f:
            f.write(json.dumps(run, indent=1) + '\n')


if __name__ == '__main__':
    main()
