#!/usr/bin/env python3
"""What the episode log (mapf_set_episode_log) costs and what it buys, in ONE process, the legs alternating block by block.  One JSON line.

    make -C <checkout of the parent commit>/gym-mapf_amd/csrc            # the parent's libmapf_hip.so
    python tools/bench_episode_log.py --parent-lib <that libmapf_hip.so> --write profiles/episode_log_bench.json    # on a MI355X

Shape and method of tools/bench_episode_budget.py: BASELINE configs[2] (room-32-32-4, 8 agents, 65536 envs, slip 0.2), the
shortest-path table policy, N = 64, B = 8: an evaluation is re-arm, reset and two totals-only launches of 256 steps.  Preroll, then
HIP events around `launches` evaluations, `blocks` blocks per leg (median, with min and max: the session's spread).
  eval_log       (a) the evaluation with the log on (C = 8): it ends with the totals AND the 8 records per env in device memory
  eval_plain     (b) the same evaluation with the log off, in the same session
  eval_log_again     (a) once more on a second handle, as the last fused leg of the round: how far two handles of one mode lie apart
  parent_record_512  (c) the parent commit's only route to the same records: a recording limit rollout of 512 steps, then a torch pass
                         that cuts rec_reward, rec_done, rec_truncated (and rec_collision, for the outcome) into each env's first 8 episodes
  stream_log / stream_plain   the budget launch of 256 steps with STREAMED (random) actions, B = 2^31, log on (C = 32, cleared before
                         every launch: a 32 MB memset inside the timing) and off: whether the scattered record stores sit behind
                         the streamed instances' wait for the action word
Before anything is timed the records of (a) are compared with those of (c): the integers exactly, the returns to 1e-9 (torch's
segmented sums associate differently).  Without --parent-lib (c) runs on this tree's library with the log off -- the same kernel
code (tests/test_episode_log_host.py, tools/compare_device_listings.sh) -- and the result says so.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gym-mapf_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402  (initialise torch's HIP runtime first)
import bench  # noqa: E402
from bench_episode_budget import load_parent, make_env_on, time_legs  # noqa: E402
from bench_policy_table import bfs_table  # noqa: E402
from gym_mapf_amd import _native as nat  # noqa: E402

T, N_LIMIT, B_EVAL = 256, 64, 8
C_STREAM = 32       # the streamed legs' capacity: cleared before every launch, so that the launch's first 32 episode ends per env store a record


class EvaluateLeg:
    """(a), (b): B episodes per env -- set_episode_budget (re-arms), [clear the log,] reset, two launches of T steps into one set of totals"""

    def __init__(self, kind, work, log):
        self.kind, self.log = kind, log
        cfg, grid, start, goal, table, rows = work
        self.env = env = make_env_on(None, cfg, grid, start, goal)
        env.set_policy('table', table=table, rows=rows)
        env.set_episode_limit(N_LIMIT)
        env.set_episode_budget(B_EVAL)
        if log:
            env.set_episode_log(B_EVAL)
            E = env.n_envs
            self.raw = {'records': torch.zeros((E, B_EVAL, 16), dtype=torch.uint8, device='cuda'), 'count': torch.zeros(E, dtype=torch.uint32, device='cuda')}
        self.n_launches = -(-B_EVAL * N_LIMIT // T)
        self.out = env.rollout(T, auto_reset=True)
        self.launch()
        env.sync()
        assert not env.episodes_left().cpu().numpy().any(), 'every env is parked after B * N steps'

    def launch(self):
        env = self.env
        env.set_episode_budget(B_EVAL)
        env.reset()
        if self.log:     # (the previous evaluation's records go: enqueued, like everything here)
            nat.check(env._lib.mapf_episode_log(env._h, None, None, 1))
        self.out = env.rollout(T, auto_reset=True, out=self.out)
        for _ in range(self.n_launches - 1):
            env.rollout(T, auto_reset=True, accumulate_into=self.out)

    def steps(self):
        return T * self.n_launches

    def records(self):
        got = self.env.episode_log(out=self.raw)
        return {k: got[k].cpu().numpy() for k in ('returns', 'steps', 'outcome', 'count')}

    def extra(self):
        self.env.sync()
        res = {'last_kernel': self.env.last_kernel('rollout'), 'live_steps_per_evaluation': int(self.out['live_steps'].sum().item()),
               'episodes_per_evaluation': int(self.out['episodes'].sum().item()) + int(self.out['truncations'].sum().item())}
        if self.log:
            rec = self.records()
            res.update(records_per_evaluation=int(np.minimum(rec['count'], B_EVAL).sum()), count_min=int(rec['count'].min()), count_max=int(rec['count'].max()),
                       record_bytes=int(self.env.n_envs) * B_EVAL * 16)
        return res


class StreamLeg:
    """one budget launch of T steps with streamed actions (random, generated once), far from parking: B = 2^31"""

    def __init__(self, kind, work, log):
        self.kind = kind
        cfg, grid, start, goal, table, rows = work
        self.env = env = make_env_on(None, cfg, grid, start, goal)
        env.set_episode_limit(N_LIMIT)
        env.set_episode_budget(1 << 31)
        self.log = log
        if log:
            env.set_episode_log(C_STREAM)
        self.actions = env.fill_random_actions(0, T)
        self.out = env.rollout(T, actions=self.actions, auto_reset=True)
        env.sync()

    def launch(self):
        if self.log:
            nat.check(self.env._lib.mapf_episode_log(self.env._h, None, None, 1))
        self.out = self.env.rollout(T, actions=self.actions, auto_reset=True, out=self.out)

    def steps(self):
        return T

    def extra(self):
        self.env.sync()
        res = {'last_kernel': self.env.last_kernel('rollout'), 'episodes_per_launch': int(self.out['episodes'].sum().item()) + int(self.out['truncations'].sum().item())}
        if self.log:
            count = self.env.episode_log()['count'].cpu().numpy()
            res['records_stored_per_launch'] = int(np.minimum(count, C_STREAM).sum())
        return res


class RecordPassLeg:
    """(c): record B * N steps under the limit (no budget, no log), then cut the trajectory into each env's first B episodes in torch"""

    def __init__(self, kind, lib, work):
        self.kind = kind
        cfg, grid, start, goal, table, rows = work
        self.stream = stream = torch.cuda.Stream()                # the caller's stream: torch's pass and the rollout share it
        self.env = env = make_env_on(lib, cfg, grid, start, goal, stream=stream.cuda_stream)
        env.set_policy('table', table=table, rows=rows)
        env.set_episode_limit(N_LIMIT)
        self.n_steps = B_EVAL * N_LIMIT
        self.out = env.rollout(self.n_steps, auto_reset=True, record=True)
        self.rec = None
        self.launch()
        env.sync()
        torch.cuda.synchronize()

    def launch(self):
        env = self.env
        env.reset()
        env.set_episode_limit(N_LIMIT)                            # (zeroes the ages: fresh episodes, as the evaluation's reset does)
        out = self.out = env.rollout(self.n_steps, auto_reset=True, record=True, out=self.out)
        with torch.cuda.stream(self.stream):
            E = out['done'].shape[1]
            done, trunc = out['done'] != 0, out['truncated'] != 0
            ended = done | trunc
            index = torch.cumsum(ended, dim=0, dtype=torch.int64) - ended.to(torch.int64)       # the episode a step belongs to
            keep = index < B_EVAL
            slot = torch.where(keep, index, torch.full_like(index, B_EVAL))                      # (later steps: a column that is dropped)
            noop = done & (out['prob'] == 0)                                                     # a terminal start's no-op: no live step
            returns = torch.zeros((B_EVAL + 1, E), dtype=torch.float64, device=done.device).scatter_add_(0, slot, out['reward'])
            steps = torch.zeros((B_EVAL + 1, E), dtype=torch.int64, device=done.device).scatter_add_(0, slot, (~noop).to(torch.int64))
            how = done.to(torch.int64) | (out['collision'] != 0).to(torch.int64) << 1 | trunc.to(torch.int64) << 2
            outcome = torch.zeros((B_EVAL + 1, E), dtype=torch.int64, device=done.device).scatter_add_(0, slot, how * ended)
            self.rec = {'returns': returns[:B_EVAL].t().contiguous(), 'steps': steps[:B_EVAL].t().contiguous(), 'outcome': outcome[:B_EVAL].t().contiguous(),
                        'count': torch.clamp(ended.sum(dim=0), max=B_EVAL)}

    def steps(self):
        return self.n_steps

    def records(self):
        self.env.sync()
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.rec.items()}

    def extra(self):
        rec = self.records()
        return {'last_kernel': self.env.last_kernel('rollout') + ' | torch: cumsum of done | truncated over T, three scatter_adds into [B + 1, E]',
                'records_per_evaluation': int(rec['count'].sum()), 'trajectory_bytes': int(sum(v.numel() * v.element_size() for v in self.out.values()))}


def same_records(a, c):
    """(a)'s records against (c)'s: counts, lengths and outcomes exactly, the returns to 1e-9"""
    stored = np.arange(B_EVAL)[None, :] < np.minimum(a['count'], B_EVAL)[:, None]
    ok = np.array_equal(np.minimum(a['count'], B_EVAL), c['count']) and np.array_equal(a['steps'][stored], c['steps'][stored]) \
        and np.array_equal(a['outcome'][stored], c['outcome'][stored])
    worst = float(np.abs(a['returns'][stored] - c['returns'][stored]).max(initial=0.0))
    return bool(ok and worst < 1e-9), worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libmapf_hip.so (default: leg (c) on this tree's library, log off)")
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--preroll-ms', type=float, default=60.0)
    ap.add_argument('--write', default=None, help='also write the result to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_episode_log.py needs a GPU')
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    assert parent is None or not hasattr(parent, 'mapf_set_episode_log'), '--parent-lib must be the library of the commit before the log'
    cfg = bench.CONFIGS['c3']
    E, A = args.envs, cfg['agents']
    grid, _, nbr, start, goal = bench.workload_tables(cfg, E, 0)
    table, lookup = bfs_table(nbr, goal)
    work = (cfg, grid, start, goal, table, lookup[goal.astype(np.int64)].astype(np.uint16))
    run = {'tool': 'bench_episode_log', 'device': torch.cuda.get_device_name(0), 'T': T, 'limit': N_LIMIT, 'budget': B_EVAL, 'capacity': B_EVAL,
           'launches': args.launches, 'blocks': args.blocks, 'unit': 'ms per evaluation (eval_*, parent_record_512), ms per launch (stream_*)',
           'parent': parent.mapf_version().decode() if parent else "this tree's library, log off", 'this': nat.version(),
           'workload': '%s: %s, %d agents, slip %g, %d envs, shortest-path table policy' % (cfg['baseline'], cfg['map'], A, cfg['fail_prob'], E)}
    legs = [EvaluateLeg('eval_log', work, True), EvaluateLeg('eval_plain', work, False), StreamLeg('stream_log', work, True),
            StreamLeg('stream_plain', work, False), EvaluateLeg('eval_log_again', work, True), RecordPassLeg('parent_record_512', parent, work)]
    for leg in (legs[0], legs[-1]):       # the same step indices, so the same random numbers: one evaluation each from t = 0
        leg.env.sync()
        leg.env.set_state(t=0)
        leg.launch()
    run['records_agree'], run['records_worst_return_difference'] = same_records(legs[0].records(), legs[-1].records())
    assert run['records_agree'], run
    ms = time_legs(legs, args.launches, args.blocks, args.preroll_ms)
    res = {}
    for leg in legs:
        v = sorted(ms[id(leg)])
        med = v[(len(v) - 1) // 2]
        res[leg.kind] = dict({'ms': med, 'ms_min': v[0], 'ms_max': v[-1], 'steps': leg.steps(), 'agent_steps_per_s': float(leg.steps()) * E * A / (med * 1e-3)}, **leg.extra())
    a, b, c = (res[k]['ms'] for k in ('eval_log', 'eval_plain', 'parent_record_512'))
    res['ratios'] = {'a_over_b': a / b, 'c_over_a': c / a, 'a_again_over_a': res['eval_log_again']['ms'] / a,
                     'stream_log_over_stream_plain': res['stream_log']['ms'] / res['stream_plain']['ms'],
                     'b_spread_ms': [res['eval_plain']['ms_min'], res['eval_plain']['ms_max']], 'a_spread_ms': [res['eval_log']['ms_min'], res['eval_log']['ms_max']]}
    run['results'] = res
    for leg in legs:
        leg.env.close()
    print(json.dumps(run))
    if args.write:
        with open(args.write, 'w') as f:
            f.write(json.dumps(run, indent=1) + '\n')


if __name__ == '__main__':
    main()
