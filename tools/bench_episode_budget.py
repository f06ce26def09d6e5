#!/usr/bin/env python3
"""What the episode budget (mapf_set_episode_budget) costs and what it buys, against the commit before it -- both libraries in ONE
process, the legs alternating block by block.  One JSON line.

    make -C <checkout of the parent commit>/gym-mapf_amd/csrc            # the parent's libmapf_hip.so
    python tools/bench_episode_budget.py --parent-lib <that libmapf_hip.so> --write profiles/episode_budget_bench.json    # on a MI355X

Shape and method of tools/bench_episode_limit.py: BASELINE configs[2] (room-32-32-4, 8 agents, 65536 envs, slip 0.2), T = 256, the
shortest-path table policy, preroll, then HIP events around `launches` launches, `blocks` blocks per leg (median, with min and max:
the session's spread).  Every leg runs totals-only and recording.
  parent_limit_64   (a) the parent's library, N = 64: the yardstick
  parent_limit_64_again  (a) once more, as the last rollout leg of the round: a second handle of the same library.  It measures how far
                        two handles of ONE library lie apart in this session (`a_again_over_a`); the bar of (b) stays (a)'s own spread
  limit_64          (b) this tree's library, N = 64, no budget: the same kernel, unchanged
  budget_far        (c) N = 64, B = 2^31: the budget instance runs and no env ever parks -- the price of the budget itself
  budget_8          (d) N = 64, B = 8: re-arm, reset, two launches of 256 -- the evaluation use case; a `launch` is the whole of it,
                        ending with the five per-env statistics in device memory (recording: ONE launch of 512 into arrays made
                        before the timing -- accumulate_into= would allocate a fresh trajectory per launch)
  parent_record_512 (e) the parent's only route to the same numbers: a recording limit rollout of 512 steps and a torch pass over the
                        T x E arrays that keeps each env's first 8 episode ends (totals-only section only: it has no other form)
"""
import argparse
import ctypes
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

T, N_LIMIT, B_FAR, B_EVAL = 256, 64, 1 << 31, 8


def load_parent(path):
    """the parent commit's library beside this tree's: its own copy of every entry point it has, typed from the same table"""
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in nat.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def make_env_on(lib, *args, **kw):
    """make_env with `lib` as the library the handle is created from and bound to (None: this tree's)"""
    if lib is None:
        return make_env(*args, **kw)
    mine = nat.load()
    nat._lib = lib
    try:
        return make_env(*args, **kw)
    finally:
        nat._lib = mine


class RolloutLeg:
    """a fused rollout of T steps under the table policy and N = 64: launch() enqueues it"""

    def __init__(self, kind, lib, budget, work, record):
        self.kind, self.record = kind, record
        cfg, grid, start, goal, table, rows = work
        self.env = env = make_env_on(lib, cfg, grid, start, goal)
        env.set_policy('table', table=table, rows=rows)
        env.set_episode_limit(N_LIMIT)
        if budget:
            env.set_episode_budget(budget)
        self.out = env.rollout(T, auto_reset=True, record=record)
        env.sync()

    def launch(self):
        self.out = self.env.rollout(T, auto_reset=True, record=self.record, out=self.out)

    def steps(self):
        return T

    def extra(self):
        self.env.sync()
        return {'last_kernel': self.env.last_kernel('rollout'), 'episodes_per_launch': int(self.out['episodes'].sum().item()),
                'truncations_per_launch': int(self.out['truncations'].sum().item())}


class EvaluateLeg(RolloutLeg):
    """(d): B episodes per env -- set_episode_budget (re-arms), reset, then launches of T steps accumulated into one set of totals"""

    def __init__(self, kind, lib, budget, work, record):
        super().__init__(kind, lib, budget, work, record)
        self.n_launches = 1 if record else -(-B_EVAL * N_LIMIT // T)
        self.n_steps = B_EVAL * N_LIMIT // self.n_launches
        if record:
            self.out = self.env.rollout(self.n_steps, auto_reset=True, record=True)
        self.launch()
        self.env.sync()
        left = self.env.episodes_left().cpu().numpy()
        assert not left.any(), 'every env is parked after B * N steps'

    def launch(self):
        env = self.env
        env.set_episode_budget(B_EVAL)
        env.reset()
        self.out = env.rollout(self.n_steps, auto_reset=True, record=self.record, out=self.out)
        for _ in range(self.n_launches - 1):
            env.rollout(self.n_steps, auto_reset=True, accumulate_into=self.out)

    def steps(self):
        return self.n_steps * self.n_launches

    def extra(self):
        res = super().extra()
        live = int(self.out['live_steps'].sum().item())
        return dict(res, live_steps_per_evaluation=live, live_fraction=live / float(self.steps() * self.env.n_envs))


class RecordPassLeg:
    """(e): the parent's route -- record B * N steps under the limit, then keep each env's first B episode ends in torch"""

    def __init__(self, kind, lib, work):
        self.kind, self.record = kind, True
        cfg, grid, start, goal, table, rows = work
        self.stream = stream = torch.cuda.Stream()                # the caller's stream: torch's pass and the rollout share it
        self.env = env = make_env_on(lib, cfg, grid, start, goal, stream=stream.cuda_stream)
        env.set_policy('table', table=table, rows=rows)
        env.set_episode_limit(N_LIMIT)
        self.n_steps = B_EVAL * N_LIMIT
        self.out = env.rollout(self.n_steps, auto_reset=True, record=True)
        self.stats = None
        self.launch()
        env.sync()
        torch.cuda.synchronize()

    def launch(self):
        env = self.env
        env.reset()
        env.set_episode_limit(N_LIMIT)                            # (zeroes the ages: fresh episodes, as (d)'s reset does)
        out = self.out = env.rollout(self.n_steps, auto_reset=True, record=True, out=self.out)
        with torch.cuda.stream(self.stream):
            done, trunc = out['done'] != 0, out['truncated'] != 0
            ended = done | trunc
            before = torch.cumsum(ended, dim=0, dtype=torch.int32) - ended.to(torch.int32)      # episode ends before this step
            keep = before < B_EVAL
            noop = done & (out['prob'] == 0)
            self.stats = {'returns': (out['reward'] * keep).sum(dim=0), 'episodes': (done & keep).sum(dim=0, dtype=torch.int32),
                          'collisions': ((out['collision'] != 0) & keep).sum(dim=0, dtype=torch.int32),
                          'truncations': (trunc & keep).sum(dim=0, dtype=torch.int32), 'live_steps': (keep & ~noop).sum(dim=0, dtype=torch.int32)}

    def steps(self):
        return self.n_steps

    def extra(self):
        self.env.sync()
        torch.cuda.synchronize()
        return {'last_kernel': self.env.last_kernel('rollout') + ' | torch: cumsum of done | truncated over T, five masked sums',
                'live_steps_per_evaluation': int(self.stats['live_steps'].sum().item()), 'episodes_kept': int(self.stats['episodes'].sum().item())}


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
    ap.add_argument('--parent-lib', required=True, help="the parent commit's libmapf_hip.so")
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--preroll-ms', type=float, default=60.0)
    ap.add_argument('--write', default=None, help='also write the result to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_episode_budget.py needs a GPU')
    parent = load_parent(args.parent_lib)
    assert not hasattr(parent, 'mapf_set_episode_budget'), '--parent-lib must be the library of the commit before the budget'
    cfg = bench.CONFIGS['c3']
    E, A = 65536, cfg['agents']
    grid, _, nbr, start, goal = bench.workload_tables(cfg, E, 0)
    table, lookup = bfs_table(nbr, goal)
    work = (cfg, grid, start, goal, table, lookup[goal.astype(np.int64)].astype(np.uint16))
    run = {'tool': 'bench_episode_budget', 'device': torch.cuda.get_device_name(0), 'T': T, 'limit': N_LIMIT, 'budget_far': B_FAR, 'budget_eval': B_EVAL,
           'launches': args.launches, 'blocks': args.blocks, 'unit': 'agent-steps/s (value), ms per launch (ms_*)',
           'parent': parent.mapf_version().decode(), 'this': nat.version(),
           'workload': '%s: %s, %d agents, slip %g, %d envs, shortest-path table policy' % (cfg['baseline'], cfg['map'], A, cfg['fail_prob'], E)}
    for record in (False, True):
        legs = [RolloutLeg('parent_limit_64', parent, 0, work, record), RolloutLeg('limit_64', None, 0, work, record),
                RolloutLeg('budget_far', None, B_FAR, work, record), EvaluateLeg('budget_8', None, B_EVAL, work, record),
                RolloutLeg('parent_limit_64_again', parent, 0, work, record)]
        if not record:
            legs.append(RecordPassLeg('parent_record_512', parent, work))
        ms = time_legs(legs, args.launches, args.blocks, args.preroll_ms)
        res = {}
        for leg in legs:
            v = sorted(ms[id(leg)])
            med = v[(len(v) - 1) // 2]
            res[leg.kind] = dict({'value': float(leg.steps()) * E * A / (med * 1e-3), 'ms_per_launch': med, 'ms_min': v[0], 'ms_max': v[-1],
                                  'steps_per_launch': leg.steps()}, **leg.extra())
        a, b, c, d = (res[k]['ms_per_launch'] for k in ('parent_limit_64', 'limit_64', 'budget_far', 'budget_8'))
        pa, again = res['parent_limit_64'], res['parent_limit_64_again']
        res['ratios'] = {'b_over_a': a / b, 'c_over_a': a / c, 'c_over_b': b / c, 'a_again_over_a': a / again['ms_per_launch'],
                         'b_inside_parent_spread': pa['ms_min'] <= b <= pa['ms_max'], 'parent_spread_ms': [pa['ms_min'], pa['ms_max']],
                         'b_inside_parent_again_spread': again['ms_min'] <= b <= again['ms_max']}
        if not record:
            res['ratios']['e_ms_over_d_ms'] = res['parent_record_512']['ms_per_launch'] / d
        run['recording' if record else 'totals'] = res
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
