#!/usr/bin/env python3
"""Throughput of the fused rollout under the table policy (MAPF_POLICY_TABLE) next to the other ways of feeding it, and
next to what a caller with a table policy had to do before: one launch per env-step.  One JSON line.

    python tools/bench_policy_table.py                       # every leg, on a MI355X
    python tools/bench_policy_table.py --legs stepwise       # only the pre-table-policy caller's path: uses no API newer
                                                             # than prepare_step / graph_begin, so it runs on older checkouts
    python tools/bench_policy_table.py --write profiles/policy_table_bench.json

Shapes: c3 = BASELINE configs[2] (65536 envs x 8 agents, room-32-32-4), c2 = configs[1] (4096 x 4, empty-16-16), c5s =
configs[4]'s share of one GPU (16384 x 32, synthetic 64x64 map).  Each leg: preroll, then HIP events around `launches`
launches of T = 256 env-steps, median of `blocks` blocks; recording (all five trajectory arrays) and totals-only.  The
legs of a shape run in ONE process, alternating, so clock and thermal state are shared.
  table / table_lds / table_global   the table policy: default dispatch, and the two forms pinned (MAPF_TUNE policy_table_lds)
  greedy / random / streamed         the other in-kernel policies and pre-written actions on the same shape
  stepwise                           a hipGraph of T x (torch gather table[rows, state_view] -> u8 actions, prepare_step)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gym-mapf_amd'), ROOT]
import torch  # noqa: E402  (initialise torch's HIP runtime first)
import bench  # noqa: E402
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv  # noqa: E402

SHAPES = {'c3': ('c3', 65536), 'c2': ('c2', 4096), 'c5s': ('c5', 16384)}
T = 256


def bfs_table(nbr, goals):
    """Shortest-path rows for the distinct goal cells, restated here (numpy only) so that the stepwise leg needs nothing a
    checkout without envs/policies.py lacks: first of UP, RIGHT, DOWN, LEFT that is one step closer, else STAY."""
    V = nbr.shape[0]
    moves = nbr[:, 1:5].astype(np.int64)
    goals = np.unique(np.asarray(goals, np.int64))
    table = np.zeros((goals.size, V), np.uint8)
    for r, goal in enumerate(goals):
        dist = np.full(V, -1, np.int64)
        dist[goal] = 0
        frontier, d = np.asarray([goal]), 0
        while frontier.size:
            d += 1
            nxt = np.unique(moves[frontier].ravel())
            nxt = nxt[dist[nxt] < 0]
            dist[nxt] = d
            frontier = nxt
        undecided = dist > 0
        for a in (1, 2, 3, 4):
            tgt = dist[moves[:, a - 1]]
            take = undecided & (tgt >= 0) & (tgt == dist - 1)
            table[r, take] = a
            undecided &= ~take
    lookup = np.zeros(V, np.int64)
    lookup[goals] = np.arange(goals.size)
    return table, lookup


def workload(shape):
    name, E = SHAPES[shape]
    cfg = bench.CONFIGS[name]
    grid, _, nbr, start, goal = bench.workload_tables(cfg, E, 0)
    # c5s: goals are random cells -- rows for the goals of the first 64 envs (2048 rows x V: beyond any LDS), reused by the others
    plan_goals = goal if cfg['scen_ids'] is not None else goal[:64]
    table, lookup = bfs_table(nbr, plan_goals)
    if cfg['scen_ids'] is not None:
        rows = lookup[goal.astype(np.int64)]
    else:
        rows = np.random.RandomState(5).randint(0, table.shape[0], size=goal.shape)
        rows[:64] = lookup[goal[:64].astype(np.int64)]
    return cfg, grid, start, goal, table, rows.astype(np.uint16)


def make_env(cfg, grid, start, goal, tune=None, **kw):
    old = os.environ.get('MAPF_TUNE')
    if tune:
        os.environ['MAPF_TUNE'] = tune                            # (read when the handle is created)
    try:
        return VecMapfEnv(grid, cfg['agents'], None, None, cfg['fail_prob'], bench.R_CLASH, bench.R_GOAL, bench.R_LIVING,
                          OptimizationCriteria.Makespan, seed=bench.SEED, device=torch.cuda.current_device(), device_arrays=True,
                          start_local=start, goal_local=goal, **kw)
    finally:
        if tune:
            if old is None:
                del os.environ['MAPF_TUNE']
            else:
                os.environ['MAPF_TUNE'] = old


class RolloutLeg:
    """One way of feeding the fused rollout: launch() enqueues T env-steps."""

    def __init__(self, kind, cfg, grid, start, goal, table, rows, record):
        self.kind, self.record = kind, record
        tune = {'table_lds': 'policy_table_lds=1', 'table_global': 'policy_table_lds=0'}.get(kind)
        self.env = env = make_env(cfg, grid, start, goal, tune)
        self.actions = env.fill_random_actions(0, T) if kind == 'streamed' else None
        if kind.startswith('table'):
            env.set_policy('table', table=table, rows=rows)
        elif kind == 'greedy':
            env.set_policy('greedy')
        self.out = env.rollout(T, actions=self.actions, auto_reset=True, record=record)
        env.sync()

    def launch(self):
        self.out = self.env.rollout(T, actions=self.actions, auto_reset=True, record=self.record, out=self.out)

    def kernel(self):
        return self.env.last_kernel('rollout')


class StepwiseLeg:
    """What a caller with a table policy did before the table policy existed: per env-step one torch gather
    table[rows, state] -> u8 actions and one mapf_step, the T pairs recorded into a hipGraph (the caller's kernels are
    recorded with the steps, as tests/test_gpu_step_graph.py shows) and replayed; launch() replays it once."""

    def __init__(self, cfg, grid, start, goal, table, rows, record):
        self.kind, self.record = 'stepwise', record
        self.stream = stream = torch.cuda.Stream()                # the caller's stream: torch's kernels and the steps share it
        self.env = env = make_env(cfg, grid, start, goal, stream=stream.cuda_stream)
        E, A, V = env.n_envs, env.n_agents, table.shape[1]
        flat = torch.from_numpy(table.reshape(-1).copy()).cuda()
        base = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(rows.reshape(-1, A), (E, A))).astype(np.int64) * V).cuda()
        view = env.state_view()
        acts = torch.empty((E, A), dtype=torch.uint8, device='cuda')
        idx = torch.empty((E, A), dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()

        def gather():
            with torch.cuda.stream(stream):
                idx.copy_(view)                                   # cell
                idx.add_(base)                                    # row * V + cell
                torch.take(flat, idx, out=acts)
        self.graph, self.note = None, 'hipGraph of T x (torch gather + mapf_step)'
        call, _ = env.prepare_step(acts, auto_reset=True, write_local=record)
        gather(); call(); env.sync()                              # warm: torch picks its kernels outside the recording
        try:
            env.graph_begin()
            for _ in range(T):
                gather()
                call()
            self.graph = env.graph_end()
        except Exception as exc:                                  # noqa: BLE001  (the gather could not be recorded on this box)
            self.note = 'plain launches (recording the gather failed: %s)' % type(exc).__name__
            self.graph = None
            self._gather, self._call = gather, call
        self.launch()
        env.sync()

    def launch(self):
        if self.graph is not None:
            self.graph.launch(1)
        else:
            for _ in range(T):
                self._gather()
                self._call()

    def kernel(self):
        return self.env.last_kernel('step') + ' | ' + self.note


def time_legs(legs, launches, blocks, preroll_ms):
    """Median ms per launch of every leg; the legs alternate block by block."""
    for leg in legs:
        t_end = time.perf_counter() + preroll_ms * 1e-3
        while time.perf_counter() < t_end:
            leg.launch()
            leg.env.sync()
    ms = {id(leg): [] for leg in legs}
    for _ in range(blocks):
        for leg in legs:
            leg.env.sync()
            leg.env.timer_begin()
            for _ in range(launches):
                leg.launch()
            ms[id(leg)].append(leg.env.timer_end() / launches)
    return {key: sorted(v)[(len(v) - 1) // 2] for key, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c3,c2,c5s')
    ap.add_argument('--legs', default='table,table_lds,table_global,greedy,random,streamed,stepwise')
    ap.add_argument('--launches', type=int, default=6)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--preroll-ms', type=float, default=60.0)
    ap.add_argument('--write', default=None, help='also write the line to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_policy_table.py needs a GPU')
    kinds = [k for k in args.legs.split(',') if k]
    line = {'tool': 'bench_policy_table', 'device': torch.cuda.get_device_name(0), 'T': T, 'launches': args.launches, 'blocks': args.blocks,
            'unit': 'agent-steps/s', 'shapes': {}}
    for shape in [s for s in args.shapes.split(',') if s]:
        cfg, grid, start, goal, table, rows = workload(shape)
        E, A = start.shape[0], cfg['agents']
        entry = {'workload': '%s: %s, %d agents, slip %g, %d envs' % (cfg['baseline'], cfg['map'], A, cfg['fail_prob'], E),
                 'table_rows': int(table.shape[0]), 'table_bytes': int(table.size)}
        for record in (False, True):
            legs = [StepwiseLeg(cfg, grid, start, goal, table, rows, record) if k == 'stepwise'
                    else RolloutLeg(k, cfg, grid, start, goal, table, rows, record) for k in kinds]
            ms = time_legs(legs, args.launches, args.blocks, args.preroll_ms)
            res = {}
            for leg in legs:
                res[leg.kind] = {'value': float(T) * E * A / (ms[id(leg)] * 1e-3), 'ms_per_launch': ms[id(leg)], 'last_kernel': leg.kernel()}
            if 'table' in res:
                for other in ('greedy', 'random', 'streamed', 'stepwise'):
                    if other in res:
                        res['table_over_' + other] = res['table']['value'] / res[other]['value']
            if 'table_lds' in res and 'table_global' in res:
                res['table_lds_over_table_global'] = res['table_lds']['value'] / res['table_global']['value']
            entry['recording' if record else 'totals'] = res
            for leg in legs:
                if getattr(leg, 'graph', None) is not None:
                    leg.graph.close()
                leg.env.close()
        line['shapes'][shape] = entry
    text = json.dumps(line)
    print(text)
    if args.write:
        with open(args.write, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
