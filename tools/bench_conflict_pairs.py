#!/usr/bin/env python3
"""What the conflict matrix (mapf_set_conflict_pairs) costs and what it buys -- every leg in ONE process, the legs alternating block
by block.  One JSON line.

    python tools/bench_conflict_pairs.py --write profiles/conflict_pairs_bench.json    # on a MI355X

Method of tools/bench_episode_budget.py: preroll, then HIP events around `launches` launches, `blocks` blocks per leg (median, with
min and max: the session's spread).  Two shapes, each with
  (1) pairs_on    the totals-only launch with the mode on: the lane-group instance that counts, the matrix left in device memory;
  (2) pairs_off   the same launch with the mode off: whatever kernel the route picks today (a packed one where it applies);
  (1s) pairs_on_slot_per_env  the mode on with one slot per env: the same attributed pass and as many atomic adds, spread over E
                  matrices instead of one -- what of (1)'s price is the contention on a handful of addresses;
  (2b) lane_group_off  the mode off on a handle whose tuning never takes a packed layout (MAPF_TUNE quad_lanes=0): the lane-group
                  kernel (1) runs, minus the counting -- (1) / (2b) is the price of the attributed pass and its atomics alone,
                  (1) / (2) also has the family's speed in it;
  (3) record_pass the only route to the same matrix without the mode (the device code of such a handle is the parent commit's:
                  tests/test_conflict_pairs_host.py compares the listings): a recording rollout of the same steps, then a torch pass
                  over rec_local that rebuilds the cells on entry and forms the same counts, a few steps at a time.
Before anything is timed, (3)'s matrix is compared with (1)'s: they must be equal.
Shapes:
  bench    BASELINE configs[2] (room-32-32-4, 8 agents, 65536 envs, slip 0.2) under its shortest-path table plan with limit 64 and
           budget 8: a `launch` is one evaluation -- re-arm, reset, two launches of 256 accumulated into one set of totals;
  c5share  BASELINE configs[4]'s share of one of eight devices (random-64-64-20, 32 agents, 16384 envs, slip 0.2) under the random
           policy stream, T = 256, auto-reset: collisions are frequent, the atomic traffic at its worst."""
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

T, N_LIMIT, B_EVAL = 256, 64, 8


class Leg:
    """a totals-only rollout leg: launch() enqueues one `launch` of the shape (see the module's docstring)"""

    def __init__(self, kind, shape, work, pairs, per_env=False, **kw):
        self.kind, self.shape, self.pairs = kind, shape, pairs
        cfg, grid, start, goal, table, rows = work
        self.env = env = make_env(cfg, grid, start, goal, **kw)
        self.evaluate = shape == 'bench'
        if self.evaluate:
            env.set_policy('table', table=table, rows=rows)
            env.set_episode_limit(N_LIMIT)
            env.set_episode_budget(B_EVAL)
        if pairs:
            env.set_conflict_pairs(*((env.n_envs, np.arange(env.n_envs)) if per_env else ()))
        self.n_launches = -(-B_EVAL * N_LIMIT // T) if self.evaluate else 1
        self.out = env.rollout(T, auto_reset=True)
        self.launch()
        env.sync()

    def begin(self):
        """a launch starts from the same state every time: the start cells, step index 0 and, under the budget, fresh episodes"""
        env = self.env
        if self.evaluate:
            env.set_episode_budget(B_EVAL)
        env.reset()
        env.set_state(t=0)
        if self.evaluate:
            env.set_episode_limit(N_LIMIT)
        if self.pairs:
            nat.check(env._lib.mapf_conflict_pairs(env._h, None, 1))     # clears the counts (enqueued)

    def launch(self):
        self.begin()
        env = self.env
        self.out = env.rollout(T, auto_reset=True, out=self.out)
        for _ in range(self.n_launches - 1):
            env.rollout(T, auto_reset=True, accumulate_into=self.out)

    def result(self):
        """the matrix of the last launch, int64 [A, A] on the host"""
        m = self.env.conflict_pairs()
        self.env.sync()
        return m.cpu().numpy().astype(np.int64).sum(axis=0)

    def steps(self):
        return T * self.n_launches

    def extra(self):
        self.env.sync()
        res = {'last_kernel': self.env.last_kernel('rollout'), 'collisions_per_launch': int(self.out['collisions'].sum().item())}
        if self.pairs:
            m = self.result()
            res.update(vertex_counts=int(np.triu(m, 1).sum()), swap_counts=int(np.tril(m, -1).sum()), pairs_with_a_count=int(((m + m.T) != 0).sum() // 2))
        return res


class RecordPassLeg:
    """(3): record the same steps with the mode off, then form the counts in torch from rec_local, `chunk` steps at a time"""

    def __init__(self, kind, shape, work, chunk):
        self.kind, self.shape, self.chunk = kind, shape, chunk
        cfg, grid, start, goal, table, rows = work
        self.stream = stream = torch.cuda.Stream()                # the caller's stream: torch's pass and the rollout share it
        self.env = env = make_env(cfg, grid, start, goal, stream=stream.cuda_stream)
        self.evaluate = shape == 'bench'
        if self.evaluate:
            env.set_policy('table', table=table, rows=rows)
            env.set_episode_limit(N_LIMIT)
        self.n_steps = B_EVAL * N_LIMIT if self.evaluate else T
        A = env.n_agents
        with torch.cuda.stream(stream):
            self.start = torch.from_numpy(np.ascontiguousarray(start).astype(np.int32)).to('cuda')
            self.upper = torch.triu(torch.ones((A, A), dtype=torch.bool, device='cuda'), 1)
        self.out = env.rollout(self.n_steps, auto_reset=True, record=True)
        self.m = None
        self.launch()
        env.sync()
        torch.cuda.synchronize()

    def launch(self):
        env = self.env
        env.reset()
        env.set_state(t=0)
        if self.evaluate:
            env.set_episode_limit(N_LIMIT)                        # (zeroes the ages: fresh episodes)
        out = self.out = env.rollout(self.n_steps, auto_reset=True, record=True, out=self.out)
        with torch.cuda.stream(self.stream):
            done = out['done'] != 0
            ended = done | (out['truncated'] != 0) if self.evaluate else done
            # a step counts when it was live: not a terminal no-op (done with prob 0) and, under the budget, among the env's first B episodes
            live = ~(done & (out['prob'] == 0))
            if self.evaluate:
                before = torch.cumsum(ended, dim=0, dtype=torch.int32) - ended.to(torch.int32)
                live &= before < B_EVAL
            A = self.env.n_agents
            m = torch.zeros((A, A), dtype=torch.int64, device='cuda')
            local = out['local']
            for t0 in range(0, self.n_steps, self.chunk):
                t1 = min(t0 + self.chunk, self.n_steps)
                nxt = local[t0:t1].to(torch.int32)
                # the cells on entry: the step before's, or the start cells after an episode end (and at the first step)
                prev = torch.empty_like(nxt)
                if t0 == 0:
                    prev[0] = self.start
                    prev[1:] = torch.where(ended[t0:t1 - 1, :, None], self.start[None], nxt[:-1])
                else:
                    before_cells = local[t0 - 1:t1 - 1].to(torch.int32)
                    prev[:] = torch.where(ended[t0 - 1:t1 - 1, :, None], self.start[None], before_cells)
                on = live[t0:t1, :, None, None]
                vertex = (nxt[:, :, :, None] == nxt[:, :, None, :]) & on
                swap = (prev[:, :, :, None] == nxt[:, :, None, :]) & (prev[:, :, None, :] == nxt[:, :, :, None]) & on
                m += (vertex & self.upper).sum(dim=(0, 1)) + (swap & self.upper.T).sum(dim=(0, 1))
            self.m = m

    def result(self):
        self.env.sync()
        torch.cuda.synchronize()
        return self.m.cpu().numpy()

    def steps(self):
        return self.n_steps

    def extra(self):
        self.env.sync()
        torch.cuda.synchronize()
        return {'last_kernel': self.env.last_kernel('rollout') + ' | torch: cells on entry from rec_local, A x A equality masks, masked sums, %d steps at a time' % self.chunk}


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
    ap.add_argument('--write', default=None, help='also write the result to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_conflict_pairs.py needs a GPU')
    run = {'tool': 'bench_conflict_pairs', 'device': torch.cuda.get_device_name(0), 'T': T, 'limit': N_LIMIT, 'budget': B_EVAL, 'launches': args.launches,
           'blocks': args.blocks, 'unit': 'agent-steps/s (value), ms per launch (ms_*)', 'this': nat.version()}
    for shape, key, E, chunk in (('bench', 'c3', 65536, 4), ('c5share', 'c5', 16384, 2)):
        cfg = bench.CONFIGS[key]
        A = cfg['agents']
        grid, _, nbr, start, goal = bench.workload_tables(cfg, E, 0)
        table, lookup = bfs_table(nbr, goal) if shape == 'bench' else (None, None)
        work = (cfg, grid, start, goal, table, lookup[goal.astype(np.int64)].astype(np.uint16) if table is not None else None)
        legs = [Leg('pairs_on', shape, work, True), Leg('pairs_off', shape, work, False), Leg('lane_group_off', shape, work, False, tune='quad_lanes=0'),
                RecordPassLeg('record_pass', shape, work, chunk), Leg('pairs_on_slot_per_env', shape, work, True, per_env=True)]
        same = bool(np.array_equal(legs[0].result(), legs[3].result()) and np.array_equal(legs[0].result(), legs[4].result()))
        assert same, 'the torch pass over the recording must form the matrix the launch counted'
        ms = time_legs(legs, args.launches, args.blocks, args.preroll_ms)
        res = {'workload': '%s: %s, %d agents, slip %g, %d envs, %s' % (cfg['baseline'], cfg['map'], A, cfg['fail_prob'], E,
                                                                       'shortest-path table policy, limit 64, budget 8' if shape == 'bench' else 'random policy stream'),
               'record_pass_matrix_equals_pairs_on': same}
        for leg in legs:
            v = sorted(ms[id(leg)])
            med = v[(len(v) - 1) // 2]
            res[leg.kind] = dict({'value': float(leg.steps()) * E * A / (med * 1e-3), 'ms_per_launch': med, 'ms_min': v[0], 'ms_max': v[-1],
                                  'steps_per_launch': leg.steps()}, **leg.extra())
        on, off, lg_off, rec, spread = (res[k]['ms_per_launch'] for k in ('pairs_on', 'pairs_off', 'lane_group_off', 'record_pass', 'pairs_on_slot_per_env'))
        res['ratios'] = {'on_ms_over_off_ms': on / off, 'on_ms_over_lane_group_off_ms': on / lg_off, 'record_pass_ms_over_on_ms': rec / on,
                         'on_is_faster_than_record_pass': on < rec, 'on_slot_per_env_ms_over_lane_group_off_ms': spread / lg_off}
        run[shape] = res
        for leg in legs:
            leg.env.close()
        del legs
        torch.cuda.empty_cache()
    print(json.dumps(run))
    if args.write:
        with open(args.write, 'w') as f:
            f.write(json.dumps(run, indent=1) + '\n')


if __name__ == '__main__':
    main()
