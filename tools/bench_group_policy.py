#!/usr/bin/env python3
"""What the group policy (mapf_set_policy_group) costs and what it buys -- every leg in ONE process, the legs alternating block by
block.  One JSON line.

    python tools/bench_group_policy.py --write profiles/group_policy_bench.json    # on a MI355X

Method and shape of tools/bench_joint_policy.py (its Leg and its timing loop are used as they are): preroll, then HIP events around
`launches` launches, `blocks` blocks per leg (median, with min and max); BASELINE configs[2] (room-32-32-4, 8 agents, 65536 envs, slip
0.2) with limit 64 and budget 8; a `launch` is one evaluation -- re-arm, reset, two launches of 256 steps accumulated into one set
of totals.
  (0) table          the shortest-path plan under set_policy('table'): the kernel of the commit before the mode, the baseline;
  (1) group_empty    the same plan under set_policy('group') with agents (0, 1), (2, 3), ... merged on EMPTY books: every step reads the
                     members' cells and misses; the mode's price;
  (2) group_pairs    the pairs with repair books;
  (3) group_fours    two groups of four, (0..3) and (4..7), with repair books;
  (4) host_loop_fours  leg (3)'s plan by the only route without the mode: a replayed hipGraph of 256 x (torch lookup of the group
                     action -- the keys of all books in one sorted tensor, torch.searchsorted -- + mapf_step + torch's age, episode
                     and totals updates + mapf_reset(mask)), twice per evaluation.
A repair book is per scenario (the batch has six distinct start / goal rows): policies.group_shortest_path_entries over the cells
within `radius` moves of the members' start cells, towards the cells the members' own shortest paths reach after `radius` moves
(made distinct by walking on); the radius is 3, or the largest below it at which the region's joint cells stay within --max-joint.
Before anything is timed, (4)'s totals are compared with (3)'s: they must be equal."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gym-mapf_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402  (initialise torch's HIP runtime first)
import bench  # noqa: E402
from bench_joint_policy import B_EVAL, N_LAUNCHES, N_LIMIT, Leg, T, time_legs  # noqa: E402
from bench_policy_table import bfs_table, make_env  # noqa: E402
from gym_mapf_amd import _native as nat  # noqa: E402
from gym_mapf_amd.envs import policies  # noqa: E402

PAD = policies.GROUP_PAD


def ball(nbr, cells, radius):
    """the cells within `radius` moves of `cells`, sorted"""
    seen = set(int(c) for c in cells)
    frontier = set(seen)
    for _ in range(radius):
        frontier = {int(n) for c in frontier for n in nbr[c]} - seen
        seen |= frontier
    return sorted(seen)


def repair_book(grid, nbr, table, lookup, start, goal, group, radius, max_joint):
    """(cells, actions, radius used) of a group's repair book in one scenario"""
    G = len(group)
    while radius > 0 and len(ball(nbr, [start[m] for m in group], radius)) ** G > max_joint:
        radius -= 1
    region = ball(nbr, [start[m] for m in group], radius)
    inside, targets = set(region), []
    for m in group:                                         # where the member's own shortest path is after `radius` moves, made distinct
        at, row = int(start[m]), table[lookup[int(goal[m])]]
        path = [at]
        for _ in range(radius):
            at = int(nbr[at, row[at]])
            path.append(at)
        free = [c for c in reversed(path) if c in inside and c not in targets]
        targets.append(free[0] if free else next(c for c in region if c not in targets))
    cells, actions = policies.group_shortest_path_entries(grid, targets, region)
    return cells, actions, radius


def group_plan(grid, nbr, start, goal, table, lookup, groups, radius, max_joint, empty=False):
    """the arrays of set_policy('group') for the batch: the shortest-path rows, `groups` (tuples of agents) merged in every env, one book
    per (scenario, group) -- empty books when `empty`"""
    E, A = goal.shape
    scen_rows, scen = np.unique(np.concatenate([start, goal], axis=1), axis=0, return_inverse=True)
    scen = scen.reshape(-1)
    members = np.full((A, 4), PAD, np.uint16)
    members[:, 0] = np.arange(A)
    slot = np.zeros(A, np.int64)                            # the agent's group number
    for k, group in enumerate(groups):
        for i in group:
            members[i, :len(group)], members[i, len(group):], slot[i] = group, PAD, k
    begin, cells, actions, used = [0], [], [], []
    for row in scen_rows:
        for group in groups:
            if not empty:
                c, a, r = repair_book(grid, nbr, table, lookup, row[:A], row[A:], group, radius, max_joint)
                cells.append(c)
                actions.append(a)
                used.append(r)
            begin.append(begin[-1] + (0 if empty else cells[-1].shape[0]))
    book = (scen[:, None] * max(len(groups), 1) + slot[None, :]).astype(np.uint32)
    rows = lookup[goal.astype(np.int64)].astype(np.uint16)
    plan = dict(policy='group', table=table, rows=rows, members=np.ascontiguousarray(np.broadcast_to(members, (E, A, 4))), book=book,
                entry_cells=np.concatenate(cells) if cells else np.zeros((0, 4), np.uint16),
                entry_actions=np.concatenate(actions) if actions else np.zeros((0, 4), np.uint8), book_begin=np.asarray(begin, np.uint32))
    return plan, (min(used) if used else None)


class GroupLeg(Leg):
    def extra(self):
        slots, chain = self.env.policy_group_stats()
        return dict(Leg.extra(self), table_slots=slots, longest_chain=chain)


class HostLoopLeg:
    """(4): per env-step the torch lookup of the group action, one mapf_step (auto-reset on done), the caller's own ages, episode counts
    and totals in torch, and a masked mapf_reset of the envs that ran out of steps"""

    def __init__(self, kind, work, plan, groups):
        self.kind = kind
        cfg, grid, start, goal = work
        self.stream = stream = torch.cuda.Stream()                # the caller's stream: torch's kernels and the steps share it
        self.env = env = make_env(cfg, grid, start, goal, stream=stream.cuda_stream)
        E, A, V = env.n_envs, env.n_agents, len(grid.tables()[0])
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
        # every book's keys in one sorted tensor: book * V^4 + sum cell[k] * V^k (a padded position counts as cell V - 1 + 1 = V: base V + 1)
        W = V + 1
        begin, ecells = plan['book_begin'].astype(np.int64), plan['entry_cells'].astype(np.int64)
        ecells = np.where(ecells == PAD, V, ecells)
        which = np.repeat(np.arange(begin.size - 1), np.diff(begin))
        keys = which * W ** 4 + sum(ecells[:, k] * W ** k for k in range(4))
        order = np.argsort(keys)
        self.table_bytes = int(plan['table'].size + 12 * keys.size)
        skeys, sacts = dev(keys[order], np.int64), dev(plan['entry_actions'][order], np.uint8)
        flat, base = dev(plan['table'].reshape(-1), np.uint8), dev(plan['rows'].astype(np.int64) * V, np.int64)
        group_cols = [dev(np.asarray(g), np.int64) for g in groups]
        weights = [dev(np.asarray([W ** k for k in range(len(g))]), np.int64) for g in groups]
        pad_part = [sum(V * W ** k for k in range(len(g), 4)) for g in groups]
        book_part = [dev(plan['book'][:, g[0]].astype(np.int64) * W ** 4, np.int64) for g in groups]
        view = env.state_view()
        acts = torch.empty((E, A), dtype=torch.uint8, device='cuda')
        cell, idx = (torch.empty((E, A), dtype=torch.int64, device='cuda') for _ in range(2))
        n_keys = int(keys.size)
        # every temporary of the lookup exists before the recording: no allocation in it
        i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device='cuda')
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device='cuda')
        tmp = [dict(mine=i64(E, len(g)), key=i64(E), pos=i64(E), got=i64(E), found=torch.zeros((E,), dtype=torch.bool, device='cuda'), ent=u8(E, 4), cur=u8(E, len(g)))
               for g in groups]
        age = torch.zeros((E,), dtype=torch.int32, device='cuda')
        self.left = left = torch.zeros((E,), dtype=torch.int32, device='cuda')
        over, ended, live, hit = (torch.zeros((E,), dtype=torch.bool, device='cuda') for _ in range(4))
        mask = torch.zeros((E,), dtype=torch.uint8, device='cuda')
        hit_i = torch.zeros((E,), dtype=torch.int32, device='cuda')
        gain = torch.zeros((E,), dtype=torch.float64, device='cuda')
        self.tot = tot = {'returns': torch.zeros((E,), dtype=torch.float64, device='cuda')}
        for key in ('episodes', 'collisions', 'truncations', 'live_steps'):
            tot[key] = torch.zeros((E,), dtype=torch.int32, device='cuda')
        self.age = age
        torch.cuda.synchronize()
        call, out = env.prepare_step(acts, auto_reset=True, write_local=False)
        done, coll, reward = out['done'], out['collision'], out['reward']

        def before():
            with torch.cuda.stream(stream):
                cell.copy_(view)
                torch.add(cell, base, out=idx)                    # the row bytes of every agent
                torch.take(flat, idx, out=acts)
                for cols, w, pad, book, b in zip(group_cols, weights, pad_part, book_part, tmp):
                    if n_keys == 0:
                        break
                    torch.index_select(cell, 1, cols, out=b['mine'])
                    b['mine'].mul_(w)
                    torch.sum(b['mine'], dim=1, out=b['key'])
                    b['key'].add_(pad)
                    b['key'].add_(book)
                    torch.searchsorted(skeys, b['key'], out=b['pos'])
                    b['pos'].clamp_(max=n_keys - 1)
                    torch.index_select(skeys, 0, b['pos'], out=b['got'])
                    torch.eq(b['got'], b['key'], out=b['found'])
                    torch.index_select(sacts, 0, b['pos'], out=b['ent'])
                    torch.index_select(acts, 1, cols, out=b['cur'])
                    torch.where(b['found'][:, None], b['ent'][:, :cols.numel()], b['cur'], out=b['cur'])
                    acts.index_copy_(1, cols, b['cur'])
                acts.clamp_(max=4)                                # (an action byte indexes the move table: never out of range)
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

        self.note = 'hipGraph of %d x (torch lookup of the group action + mapf_step + torch ages / episode counts / totals + mapf_reset(mask))' % T
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--preroll-ms', type=float, default=60.0)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--radius', type=int, default=3)
    ap.add_argument('--max-joint', type=int, default=1 << 19, help='most joint cells of a repair region (the radius shrinks to fit)')
    ap.add_argument('--write', default=None, help='also write the result to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_group_policy.py needs a GPU')
    cfg, E = bench.CONFIGS['c3'], args.envs
    A = cfg['agents']
    grid, _, nbr, start, goal = bench.workload_tables(cfg, E, 0)
    nbr = np.asarray(nbr).astype(np.int64)
    table, lookup = bfs_table(nbr, goal)
    rows = lookup[goal.astype(np.int64)].astype(np.uint16)
    work = (cfg, grid, start, goal)
    pairs = [(2 * p, 2 * p + 1) for p in range(A // 2)]
    fours = [tuple(range(4 * q, 4 * q + 4)) for q in range(A // 4)]
    make = lambda groups, empty=False: group_plan(grid, nbr, start.astype(np.int64), goal.astype(np.int64), table, lookup, groups, args.radius, args.max_joint, empty)
    (empty, _), (paired, r_pairs), (foured, r_fours) = make(pairs, True), make(pairs), make(fours)
    legs = [Leg('table', work, dict(policy='table', table=table, rows=rows)), GroupLeg('group_empty', work, empty), GroupLeg('group_pairs', work, paired),
            GroupLeg('group_fours', work, foured), HostLoopLeg('host_loop_fours', work, foured, fours)]
    fused, loop = legs[3].totals(), legs[4].totals()
    same = all(np.array_equal(fused[k], loop[k].astype(fused[k].dtype)) for k in fused)
    assert same, 'the host loop must reach the totals of the fused evaluation: %r' % {k: (int(fused[k].sum()), int(loop[k].sum())) for k in fused}
    plain, none = legs[0].totals(), legs[1].totals()
    assert all(np.array_equal(plain[k], none[k]) for k in plain), 'empty books must give the table plan\'s totals'
    ms = time_legs(legs, args.launches, args.blocks, args.preroll_ms)
    run = {'tool': 'bench_group_policy', 'device': torch.cuda.get_device_name(0), 'T': T, 'limit': N_LIMIT, 'budget': B_EVAL, 'launches': args.launches,
           'blocks': args.blocks, 'unit': 'agent-steps/s (value), ms per launch (ms_*)', 'this': nat.version(),
           'workload': '%s: %s, %d agents, slip %g, %d envs, V = %d, shortest-path plan with groups merged on repair books, limit %d, budget %d' % (
               cfg['baseline'], cfg['map'], A, cfg['fail_prob'], E, table.shape[1], N_LIMIT, B_EVAL),
           'repair_radius': {'pairs': r_pairs, 'fours': r_fours}, 'entries': {'pairs': int(paired['entry_cells'].shape[0]), 'fours': int(foured['entry_cells'].shape[0])},
           'host_loop_totals_equal_group_fours': same}
    for leg in legs:
        v = sorted(ms[id(leg)])
        med = v[(len(v) - 1) // 2]
        run[leg.kind] = dict({'value': float(T * N_LAUNCHES) * E * A / (med * 1e-3), 'ms_per_launch': med, 'ms_min': v[0], 'ms_max': v[-1],
                              'steps_per_launch': T * N_LAUNCHES}, **leg.extra())
    t0, g0, g2, g4, loop = (run[k]['ms_per_launch'] for k in ('table', 'group_empty', 'group_pairs', 'group_fours', 'host_loop_fours'))
    run['ratios'] = {'group_empty_ms_over_table_ms': g0 / t0, 'group_pairs_ms_over_table_ms': g2 / t0, 'group_fours_ms_over_table_ms': g4 / t0,
                     'host_loop_fours_ms_over_group_fours_ms': loop / g4}
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
