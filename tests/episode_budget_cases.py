"""The reference and the workload of the episode-budget tests (include/mapf_hip.h, mapf_set_episode_budget).

The reference is a COMPOSITION over tests/episode_limit_cases.py's LimitOracle (itself a composition of the unchanged C oracle),
following the definition's rules literally.  Per step of an auto-reset rollout under a budget B:
  0. parked = left == 0: the env's cells and age are saved before the oracle's step and put back after it, and its row of the
     step's outputs becomes (current cells, reward +0.0, prob +0.0, done 0, collision 0, truncated 0);
  1. every other env takes the LimitOracle's step (N == 0: the plain C oracle's, truncated always 0);
  2. live = ~parked & ~was_terminal;
  3. left[~parked] -= done | truncated.
Expected totals are summed left to right over the steps, and a parked step adds NOTHING to returns (not +0.0).

The workload is episode_limit_cases.Workload: the 20 x 20 random map, the INEXACT rewards, LAUNCHES = (5, 1, 18, 12).
tests/test_episode_budget_cases.py recomputes on the CPU that it shows every outcome the GPU tests rely on."""
import numpy as np

import episode_limit_cases as ec

SHAPES = ((2, 37), (3, 64), (8, 64), (16, 37), (32, 64))
# (N, slip, B): the issue's passes -- every env parks under B = 3; B = 10 leaves envs running; a budget without a limit
PASSES = ((4, 0.2, 3), (2, 0.0, 3), (4, 0.2, 10), (0, 0.2, 2))
TOTALS = ('returns', 'episodes', 'collisions', 'truncations', 'live_steps')
RECORDED = ('local', 'reward', 'prob', 'done', 'collision', 'truncated')


class BudgetOracle:
    """A LimitOracle stepped under an episode budget B: see the module's docstring."""

    def __init__(self, limit_oracle, B):
        self.lim, self.co = limit_oracle, limit_oracle.co
        self.B = int(B)
        self.left = np.full(self.co.E, self.B, np.uint32)

    @property
    def age(self):
        return self.lim.age

    def set_budget(self, B):
        self.B = int(B)
        self.left[:] = self.B                  # every mapf_set_episode_budget call re-arms every env; state and ages stay

    def step(self, actions):
        parked = self.left == 0
        cells, ages = self.co.state[parked].copy(), self.lim.age[parked].copy()
        ref = self.lim.step(actions, auto_reset=True)
        self.co.state[parked] = cells
        self.lim.age[parked] = ages
        ref['local'][parked] = cells
        for key in ('reward', 'prob'):
            ref[key][parked] = 0.0
        for key in ('done', 'collision', 'truncated'):
            ref[key][parked] = 0
        ref['parked'] = parked
        ref['live'] = (~parked & (ref['was_terminal'] == 0)).astype(np.uint8)
        ended = (ref['done'] != 0) | (ref['truncated'] != 0)
        self.left = self.left - ended.astype(np.uint32)     # (a parked row ends nothing: the count stops at 0)
        ref['parked_now'] = ended & (self.left == 0)
        return ref

    def run(self, workload, source, n_steps):
        """n_steps reference steps under the action source; every step's dict also keeps its joint `actions` (a parked env's are
        computed like the others' and never used)"""
        refs = []
        for _ in range(n_steps):
            actions = workload.actions(source, self)
            refs.append(dict(self.step(actions), actions=actions))
        return refs


def oracle(w, N, slip, B, criteria='Makespan', offset=0):
    return BudgetOracle(w.oracle(N, slip, criteria, offset=offset), B)


def totals_of(refs, base=None):
    """the five totals of the steps, added in step order (to `base` when a call accumulates); parked steps add nothing"""
    E = refs[0]['reward'].shape[0]
    tot = {k: np.zeros(E, np.float64 if k == 'returns' else np.uint32) for k in TOTALS} if base is None else {k: v.copy() for k, v in base.items()}
    for r in refs:
        tot['returns'] = np.where(r['parked'], tot['returns'], tot['returns'] + r['reward'])
        tot['episodes'] = tot['episodes'] + r['done'].astype(np.uint32)
        tot['collisions'] = tot['collisions'] + r['collision'].astype(np.uint32)
        tot['truncations'] = tot['truncations'] + r['truncated'].astype(np.uint32)
        tot['live_steps'] = tot['live_steps'] + r['live'].astype(np.uint32)
    return tot


def park_counts(launch_refs):
    """Of a pass given as one list of reference steps per launch: (parks per launch, parks by goal end / collision end / truncation /
    terminal-start no-op, envs still running at the end)."""
    per_launch = [sum(int(r['parked_now'].sum()) for r in refs) for refs in launch_refs]
    kinds = np.zeros(4, np.int64)
    for refs in launch_refs:
        for r in refs:
            now = r['parked_now']
            noop = now & (r['was_terminal'] != 0)
            coll = now & (r['collision'] != 0)
            trunc = now & (r['truncated'] != 0)
            kinds += (int((now & ~noop & ~coll & ~trunc).sum()), int(coll.sum()), int(trunc.sum()), int(noop.sum()))
    return per_launch, tuple(int(k) for k in kinds)


def run_launches(ref, w, source):
    return [ref.run(w, source, n) for n in ec.LAUNCHES]
