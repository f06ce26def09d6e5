"""The reference of the episode-log tests (include/mapf_hip.h, mapf_set_episode_log), no test in it.

The reference is a COMPOSITION over tests/episode_budget_cases.py's BudgetOracle (itself a composition over the unchanged C oracle),
following the definition's rules literally.  Per env it keeps acc (f64), len (u32), count (u32) and C records; per step, after the
BudgetOracle's step has produced reward, done, collision and truncated:
  0. an env that was parked on entry: nothing changes;
  1. otherwise acc = acc + reward (one float64 add; the terminal-on-entry no-op adds its +0.0) and len += live;
  2. where the step reports done or truncated: the record (acc, len, done | collision << 1 | truncated << 2) goes to
     records[e][count] if count < C; then count += 1 (saturating), acc = +0.0, len = 0.
The workload, the shapes, the passes and the launches are episode_budget_cases' and episode_limit_cases': the 20 x 20 random map, the
INEXACT rewards, bc.SHAPES, bc.PASSES, ec.LAUNCHES = (5, 1, 18, 12).  tests/test_episode_log_cases.py recomputes on the CPU that the
reference alone shows every outcome the GPU tests rely on."""
import numpy as np

import episode_budget_cases as bc
import episode_limit_cases as ec

RECORD = np.dtype([('ret', '<f8'), ('steps', '<u4'), ('outcome', '<u4')])
COUNT_MAX = 0xFFFFFFFF
GOAL, COLLISION, TRUNCATED = 1, 3, 4           # the outcomes an episode can have: done | collision << 1 | truncated << 2


class LogOracle:
    """A BudgetOracle -- or a conflict_pairs_cases.PairsOracle around one, whose matrix reads through -- stepped under an episode log
    of capacity C: see the module's docstring."""

    def __init__(self, inner, C):
        self.inner = inner
        self.bud = getattr(inner, 'inner', inner)          # the BudgetOracle itself: its counts are set through it
        assert isinstance(self.bud, bc.BudgetOracle)
        self.lim, self.co = self.bud.lim, self.bud.co
        self.set_log(C)

    def __getattr__(self, name):                           # (only what the wrapper itself lacks: M, take, B, ...)
        return getattr(self.inner, name)

    # what the GPU modules read of a reference, whichever oracle it is
    @property
    def age(self):
        return self.bud.age

    @property
    def left(self):
        return self.bud.left

    @left.setter
    def left(self, value):
        self.bud.left = value

    def set_log(self, C):
        """every mapf_set_episode_log call: no record, no count, no running episode"""
        E = self.co.E
        self.C = int(C)
        self.records, self.count = np.zeros((E, self.C), RECORD), np.zeros(E, np.uint32)
        self.acc, self.len = np.zeros(E, np.float64), np.zeros(E, np.uint32)

    def clear(self):
        """mapf_episode_log(clear != 0): records and counts go, the partials stay"""
        self.records[:] = np.zeros((), RECORD)
        self.count[:] = 0

    def set_budget(self, B):
        self.bud.set_budget(B)                 # (re-arms; leaves acc and len alone)

    def reset(self, mask=None):
        """mapf_reset(mask): the cells and the ages as under the limit, and the running episodes of the reset envs are dropped"""
        self.lim.reset(mask)
        which = slice(None) if mask is None else np.asarray(mask).astype(bool)
        self.acc[which], self.len[which] = 0.0, 0

    def set_state(self, cells):
        """mapf_set_state with cells: every running episode is dropped (and the ages are zeroed, as under the limit)"""
        self.co.state[:] = cells
        self.lim.age[:] = 0
        self.acc[:], self.len[:] = 0.0, 0

    def step(self, actions):
        ref = self.inner.step(actions)
        stepped = ~ref['parked']                               # rule 0: a parked env changes nothing
        self.acc[stepped] = self.acc[stepped] + ref['reward'][stepped]          # rule 1: one float64 add per env and step
        self.len[stepped] += ref['live'][stepped].astype(np.uint32)
        ended = stepped & ((ref['done'] != 0) | (ref['truncated'] != 0))        # rule 2
        room = np.flatnonzero(ended & (self.count < self.C))
        outcome = ref['done'].astype(np.uint32) | ref['collision'].astype(np.uint32) << 1 | ref['truncated'].astype(np.uint32) << 2
        for field, values in (('ret', self.acc), ('steps', self.len), ('outcome', outcome)):
            self.records[field][room, self.count[room]] = values[room]
        self.count[ended] += (self.count[ended] != COUNT_MAX).astype(np.uint32)
        self.acc[ended], self.len[ended] = 0.0, 0
        return ref

    def run(self, workload, source, n_steps):
        refs = []
        for _ in range(n_steps):
            actions = workload.actions(source, self)
            refs.append(dict(self.step(actions), actions=actions))
        return refs


def oracle(w, N, slip, B, C, criteria='Makespan', offset=0):
    return LogOracle(bc.oracle(w, N, slip, B, criteria, offset), C)


def stored(ref):
    """the records an env has room for: [E, C] bool, True in the first min(count, C) columns"""
    return np.arange(ref.C)[None, :] < np.minimum(ref.count, ref.C)[:, None]


def run_launches(ref, w, source):
    return [ref.run(w, source, n) for n in ec.LAUNCHES]
