"""Step indices, seeds and env ids that need all 64 bits: the windows, the seeds, the case table of kernel forms and the oracle side,
shared by tests/test_wide_counter_cases.py (no GPU: the oracles agree on every window, every narrowing of a 64-bit quantity shows
in the oracle's own output, the ledger) and tests/test_gpu_wide_counters.py (every case on the GPU against the values built here).
A plain module, not a conftest.

Every random draw is a Philox call whose counter and key are built from the handle's step index t, the seed and the global env id
(oracle/philox.py is the definition); the kernels split the three into 32-bit halves by hand.  The windows below put the step at
which a half wraps, carries or is masked INSIDE a launch, the env whose id carries inside the first blocks of a batch, and use
seeds whose halves are all ones.

The seed belongs to the handle (mapf_create; nothing reseeds), so "one seed per crossing point, in rotation" means one handle per
(case, crossing point): both passes of a crossing point run on that handle, repositioned with set_state."""
import functools

import numpy as np

import c_oracle
import mapf_oracle as mo
import philox
from totals_cases import EXACT, FORM_NAME, FORMS, _random_map_tables   # noqa: F401  (FORMS, FORM_NAME: for the ledger)

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
# X: the first step index on the far side of ...
CROSSINGS = (1 << 32,   # t's low word wraps (the packed step's t_lo)
             1 << 33,   # h = t >> 1: its low word wraps, the carry goes from counter word 2 into word 3
             1 << 34,   # the same for the policy stream's m = t >> 2 (refresh_policy((t >> 2) + 1) makes the carrying call at X - 1)
             1 << 49)   # the 16-bit field of h's high word is 0xFFFF below X and wraps to 0 at X, right below the quad field
SEEDS = (0xFFFFFFFF,            # slip key (0xFFFFFFFF, 0), policy key (0, 1)
         0xFFFFFFFFFFFFFFFF,    # the policy key wraps to (0, 0)
         0x9E3779B97F4A7C15)    # both halves non-trivial
OFFSET = (1 << 32) - 37         # env 37 is the first whose id has a high word: between two envs of a wave at every lanes-per-env
SLIP, REWARDS = 0.2, EXACT
NARROW_ENVS = 300               # the narrowings are evaluated on a batch's first 300 envs (the smallest case has 300)


def seed_of(index, X):
    """one seed per crossing point, in rotation: the four crossing points show every case all three seeds"""
    return SEEDS[(index + CROSSINGS.index(X)) % len(SEEDS)]


class Window:
    """`lengths` launches from step t0 on; mode: 'streamed' (host actions, not the policy stream's), 'policy' (the in-kernel random
    policy), 'table' (the table policy), 'cycle8' (eight action arrays used over and over: a recorded graph's)"""

    def __init__(self, name, t0, lengths, mode):
        self.name, self.t0, self.lengths, self.mode = name, t0, tuple(lengths), mode
        self.n_steps = sum(lengths)


def rollout_windows(X, table=False):
    """Pass A: from X - 5 (phase 3, off the four-step boundary), launches of 5 and 7 steps -- the second launch's first step is X.
    Pass B: from X - 6, one 12-step launch under the in-kernel policy -- X inside the aligned, unrolled part."""
    a = Window('A', X - 5, (5, 7), 'table' if table else 'streamed')
    return (a,) if table else (a, Window('B', X - 6, (12,), 'policy'))


def step_window(X):
    """eight single steps from X - 4: the fifth call is step X"""
    return Window('S', X - 4, (1,) * 8, 'streamed')


def graph_window(X):
    """eight recorded steps replayed three times from X - 12 (the second replay runs X - 4 .. X + 3), then two plain steps"""
    return Window('G', X - 12, (8, 8, 8, 1, 1), 'cycle8')


GRAPH_CROSSINGS = (1 << 32, 1 << 33)
FILL_CROSSINGS = (1 << 32, 1 << 34)          # fill_random_actions(t0 = X - 3, n_steps = 9)
FILL_SHAPES = ((8, 70), (5, 70))             # (agents, envs): full quads; a ragged quad


class Case:
    """One row of a table: the batch, the MAPF_TUNE keys that pin the kernel form, what the kernel's name must contain."""

    def __init__(self, id, n_agents, n_envs, layout, tune=None, kernel='auto', form=None, table=False, scen=None, device=False, map_seed=0):
        self.id, self.A, self.E, self.layout, self.tune, self.kernel = id, n_agents, n_envs, layout, dict(tune or {}), kernel
        self.form, self.table, self.scen, self.device = form, table, scen, device
        self.map_seed = map_seed      # (the way to repair a case whose inputs could not show a narrowing)
        self.index = None             # its place in its table: set below

    def tune_text(self):
        return ','.join('%s=%s' % kv for kv in self.tune.items())

    def seed(self, X):
        return seed_of(self.index, X)


def _r(id, n_agents, n_envs, layout, form=None, **tune):
    kernel = 'thread_per_env' if layout.startswith('rollout_kernel') else 'auto'
    return Case(id, n_agents, n_envs, layout, {k: str(v) for k, v in tune.items()}, kernel=kernel, form=form)


# the rows of test_goal_reaching_episodes_against_c_oracle (tests/test_gpu_parity.py): (agents, envs, what the kernel's name must hold, MAPF_TUNE)
GOAL_ROWS = [
    (4, 16384, 'lq_rollout_kernel<Q=1,K=4', {'k': '4'}), (4, 16512, 'lq_rollout_kernel<Q=2,K=2', {'k': '2'}),
    (8, 8192, 'lq_rollout_kernel<Q=2,K=4', {'k': '4'}), (8, 16448, 'lq_rollout_kernel<Q=4,K=2', {'k': '2'}),
    (8, 16448, 'lg_rollout_kernel<L=4,FULL,MV_LDS', {'quad_lanes': '0'}),
    (16, 4096, 'lq_rollout_kernel<Q=4,K=4', {'k': '4'}), (16, 4128, 'lq_rollout_kernel<Q=8,K=2', {'k': '2'}),
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,NO_TERMINAL> block=', {'k': '4', 'bitmap_pairs': '0'}),
    # (32 agents, full table rows in LDS: occupancy bitmaps behind them -- what MAPF_TUNE k=4 or a batch of one wave per SIMD gets)
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,NO_TERMINAL,BITMAP> block=', {'k': '4'}),
    (32, 1024, 'lq_rollout_kernel<Q=16,K=2', {'k': '2'}),
    (32, 1024, 'lg_rollout_kernel<L=16,FULL,MV_GLOBAL', {'mv_lds_max_bytes': '0'}),
    # eight agents per lane (the default only for batches of two waves per SIMD and more)
    (8, 8192, 'lq_rollout_kernel<Q=1,K=8', {'k': '8'}), (16, 4096, 'lq_rollout_kernel<Q=2,K=8', {'k': '8'}),
    (32, 2048, 'lq_rollout_kernel<Q=4,K=8', {'k': '8'}),
    (32, 2048, 'lq_rollout_kernel<Q=4,K=8,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL> block=512', {'mv_lds_max_bytes': '2048', 'k': '8'}),
    # (a full table "too large" for the LDS budget: the 8-byte-row form of the packed kernel, 512- and 1024-thread blocks)
    (16, 4096, 'lq_rollout_kernel<Q=4,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL> block=512', {'mv_lds_max_bytes': '2048'}),
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL> block=512', {'mv_lds_max_bytes': '2048', 'bitmap_pairs': '0'}),
    # (32 agents, 8-byte rows: collisions through per-env LDS occupancy bitmaps instead of the 496 agent pairs -- the default)
    # (five-column table where it leaves room for the bitmaps -- here it does -- else four columns and a made-up STAY row)
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL,BITMAP5> block=512', {'mv_lds_max_bytes': '2048', 'bitmap_delta': '0'}),
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL,BITMAP> block=512', {'mv_lds_max_bytes': '2048', 'bitmap_staycol': '0', 'bitmap_delta': '0'}),
    # (... in 1024-thread blocks, 128 bitmaps behind the table: what a batch that fills every CU with such a block gets)
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL,BITMAP> block=1024', {'mv_lds_max_bytes': '2048', 'bitmap_block': '1024', 'bitmap_staycol': '0', 'bitmap_delta': '0'}),
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL,BITMAP5> block=1024', {'mv_lds_max_bytes': '2048', 'bitmap_block': '1024', 'bitmap_delta': '0'}),
    # (... behind 4-byte delta rows -- the default wherever a map's neighbour ids lie within +-127 of their cell's)
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL,BITMAPD> block=512', {'mv_lds_max_bytes': '2048'}),
    (32, 2048, 'lq_rollout_kernel<Q=8,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL,BITMAPD> block=1024', {'mv_lds_max_bytes': '2048', 'bitmap_block': '1024'}),
    (64, 16384, 'lq_rollout_kernel<Q=16,K=4,RECORD,STREAM,MAKESPAN,COMPACT,NO_TERMINAL> block=1024', {'mv_lds_max_bytes': '2048'}),
    (8, 300, 'lg_rollout_kernel<L=4,FULL,MV_GLOBAL', {}), (5, 600, 'lg_rollout_kernel<L=4,RAGGED', {}),
    (8, 16417, 'lg_rollout_kernel<L=4,FULL,MV_LDS', {}), (6, 512, 'rollout_kernel<A=6>', {})]
_FULL = 'lq_rollout_kernel<Q=%d,K=%d,RECORD,STREAM,MAKESPAN%s,NO_TERMINAL%s> block=%s'
# The fused rollout: (agents, envs, the kernel's name, MAPF_TUNE) as test_goal_reaching_episodes_against_c_oracle has them -- the
# smallest batch that reaches each form (tests/test_wide_counter_cases.py holds every row against that list).  `form`: the
# TableForm the planner must choose for a packed case (totals_cases.FORMS).
ROLLOUT_CASES = [
    _r('A4-Q1K4', 4, 16384, 'lq_rollout_kernel<Q=1,K=4', 'FullRows', k=4), _r('A4-Q2K2', 4, 16512, 'lq_rollout_kernel<Q=2,K=2', 'FullRows', k=2),
    _r('A8-Q2K4', 8, 8192, 'lq_rollout_kernel<Q=2,K=4', 'FullRows', k=4), _r('A8-Q4K2', 8, 16448, 'lq_rollout_kernel<Q=4,K=2', 'FullRows', k=2),
    _r('A8-Q1K8', 8, 8192, 'lq_rollout_kernel<Q=1,K=8', 'FullRows', k=8),
    _r('A16-Q4K4', 16, 4096, 'lq_rollout_kernel<Q=4,K=4', 'FullRows', k=4), _r('A16-Q8K2', 16, 4128, 'lq_rollout_kernel<Q=8,K=2', 'FullRows', k=2),
    _r('A16-Q2K8', 16, 4096, 'lq_rollout_kernel<Q=2,K=8', 'FullRows', k=8),
    _r('A32-Q8K4-pairs', 32, 2048, _FULL % (8, 4, '', '', ''), 'FullRows', k=4, bitmap_pairs=0),
    _r('A32-Q8K4-BITMAP', 32, 2048, _FULL % (8, 4, '', ',BITMAP', ''), 'FullRowsBitmap', k=4),
    _r('A32-Q16K2', 32, 1024, 'lq_rollout_kernel<Q=16,K=2', 'FullRows', k=2), _r('A32-Q4K8', 32, 2048, 'lq_rollout_kernel<Q=4,K=8', 'FullRows', k=8),
    _r('A32-Q4K8-COMPACT', 32, 2048, _FULL % (4, 8, ',COMPACT', '', '512'), 'Rows8', mv_lds_max_bytes=2048, k=8),
    _r('A16-Q4K4-COMPACT', 16, 4096, _FULL % (4, 4, ',COMPACT', '', '512'), 'Rows8', mv_lds_max_bytes=2048),
    _r('A32-Q8K4-COMPACT-pairs', 32, 2048, _FULL % (8, 4, ',COMPACT', '', '512'), 'Rows8', mv_lds_max_bytes=2048, bitmap_pairs=0),
    _r('A32-BITMAP5-512', 32, 2048, _FULL % (8, 4, ',COMPACT', ',BITMAP5', '512'), 'Rows8x5Bitmap', mv_lds_max_bytes=2048, bitmap_delta=0),
    _r('A32-BITMAP-512', 32, 2048, _FULL % (8, 4, ',COMPACT', ',BITMAP', '512'), 'Rows8x4Bitmap', mv_lds_max_bytes=2048, bitmap_staycol=0, bitmap_delta=0),
    _r('A32-BITMAP-1024', 32, 2048, _FULL % (8, 4, ',COMPACT', ',BITMAP', '1024'), 'Rows8x4Bitmap', mv_lds_max_bytes=2048, bitmap_block=1024,
       bitmap_staycol=0, bitmap_delta=0),
    _r('A32-BITMAP5-1024', 32, 2048, _FULL % (8, 4, ',COMPACT', ',BITMAP5', '1024'), 'Rows8x5Bitmap', mv_lds_max_bytes=2048, bitmap_block=1024, bitmap_delta=0),
    _r('A32-BITMAPD-512', 32, 2048, _FULL % (8, 4, ',COMPACT', ',BITMAPD', '512'), 'DeltaRowsBitmap', mv_lds_max_bytes=2048),
    _r('A32-BITMAPD-1024', 32, 2048, _FULL % (8, 4, ',COMPACT', ',BITMAPD', '1024'), 'DeltaRowsBitmap', mv_lds_max_bytes=2048, bitmap_block=1024),
    _r('lg-A8-MV_LDS', 8, 16448, 'lg_rollout_kernel<L=4,FULL,MV_LDS', quad_lanes=0), _r('lg-A8-MV_GLOBAL', 8, 300, 'lg_rollout_kernel<L=4,FULL,MV_GLOBAL'),
    _r('lg-A5-RAGGED', 5, 600, 'lg_rollout_kernel<L=4,RAGGED'), _r('lg-A32-MV_GLOBAL', 32, 1024, 'lg_rollout_kernel<L=16,FULL,MV_GLOBAL', mv_lds_max_bytes=0),
    _r('tpe-A6', 6, 512, 'rollout_kernel<A=6>'),
    # the table policy draws from the slip stream alone: pass A only (the shape of tests/test_gpu_policy_table.py's packed cases)
    Case('A8-Q4K2-table', 8, 8192, 'lq_rollout_kernel_table<Q=4,K=2', table=True),
]
# goal-test rows left out: 64 agents x 16384 envs (Q = 16 is here at 32 agents; its oracle side alone would take longer than every other
# case together) and 8 x 16417 (the MV_LDS form again, with a ragged last block)
GOAL_ROWS_LEFT_OUT = {(64, 16384), (8, 16417)}


def _s(id, n_agents, n_envs, layout, kernel='auto', scen=None, form=None, device=False, **tune):
    return Case(id, n_agents, n_envs, layout, {k: str(v) for k, v in tune.items()}, kernel=kernel, scen=scen, form=form, device=device)


# The single step.  scen: True = start / goal rows from five scenarios (the host builds the scenario table), False = the same rows with
# MAPF_TUNE scen_table=0, None = every env its own rows (no table).  form: plan_step_lq's StepForm (0 Plain, 1 FullRows = BIG, 2 DeltaRows,
# 3 DeltaRowsBitmap).  `layout` is the name of the FIRST call (after set_state: an env may be terminal); from the second call on
# the packed step's name carries NO_TERMINAL after its SCEN tag.
STEP_CASES = [
    _s('A8-Q2K4-SCEN', 8, 512, 'lq_step_kernel<Q=2,K=4,SCEN> block=', scen=True, form=0),
    _s('A8-Q2K4', 8, 512, 'lq_step_kernel<Q=2,K=4> block=', scen=False, form=0, scen_table=0),
    _s('A8-Q4K2', 8, 512, 'lq_step_kernel<Q=4,K=2> block=', form=0, k=2),
    _s('A16-Q2K8-BIG', 16, 1024, 'lq_step_kernel<Q=2,K=8,BIG> block=1024', form=1, step_big=2),
    _s('A8-Q2K4-BIG-SCEN', 8, 1024, 'lq_step_kernel<Q=2,K=4,SCEN,BIG> block=1024', scen=True, form=1, step_big=2, k=4),
    _s('A32-DELTA', 32, 512, 'lq_step_kernel<Q=8,K=4,DELTA> block=512', form=2, step_delta=2, bitmap_pairs=0),
    _s('A32-DELTA-BITMAP', 32, 512, 'lq_step_kernel<Q=8,K=4,DELTA,BITMAP> block=512', form=3, step_delta=2),
    _s('lg-A5', 5, 300, 'lg_step_kernel<L=4,RAGGED,PHILOX> block='), _s('lg-A3', 3, 257, 'lg_step_kernel<L=2,RAGGED,PHILOX> block='),
    _s('tpe-A6', 6, 512, 'step_kernel<A=6,PHILOX> block=', kernel='thread_per_env'),
]
# A recorded graph of eight steps: one packed and one lane-group form (device arrays: only such a handle records)
GRAPH_CASES = [
    _s('graph-A8-Q2K4', 8, 1024, 'lq_step_kernel<Q=2,K=4', form=0, device=True),
    _s('graph-lg-A5', 5, 300, 'lg_step_kernel<L=4,RAGGED,PHILOX> block=', device=True),
]
for _table in (ROLLOUT_CASES, STEP_CASES, GRAPH_CASES):
    for _i, _case in enumerate(_table):
        _case.index = _i


def step_name(case, call):
    """what mapf_last_kernel('step') must begin with after call number `call` (0 = the first after set_state) of a step case"""
    if call == 0 or not case.layout.startswith('lq_step_kernel'):
        return case.layout
    head, tail = case.layout.split('>', 1)
    parts = head.split(',')
    at = 3 if (len(parts) > 2 and parts[2] == 'SCEN') else 2
    return ','.join(parts[:at] + ['NO_TERMINAL'] + parts[at:]) + '>' + tail


# ----------------------------------------------------------------------- tables
@functools.lru_cache(maxsize=2)
def tables_of(case):
    """(grid, nbr, start, goal) of a case -- family R of tests/totals_cases.py: a seeded random map with walls -- and, for the table
    policy, (table, rows).  Built once per case, never written."""
    grid, nbr, rc, start, goal, near = _random_map_tables(case.A, case.E, 700 + case.map_seed)
    if case.scen is not None:                                         # five scenarios, dealt to the envs
        which = (np.arange(case.E) * 7 + 3) % 5
        start, goal = np.ascontiguousarray(start[which]), np.ascontiguousarray(goal[which])
    policy = None
    if case.table:
        rs = np.random.RandomState(900 + case.map_seed)
        policy = (rs.randint(0, 5, size=(9, nbr.shape[0])).astype(np.uint8), rs.randint(0, 9, size=(case.E, case.A)).astype(np.uint16))
    for a in (nbr, start, goal) + (policy or ()):
        a.setflags(write=False)
    return grid, nbr, start, goal, policy


def policy_actions(seed, ids, t, n_agents):
    """what the in-kernel random policy draws (key seed + 1)"""
    return philox.random_actions_np(seed, ids, t, n_agents)


def streamed_actions(seed, ids, t, n_agents):
    """host-side actions of the streamed windows: any stream will do, so not the in-kernel one"""
    return philox.random_actions_np((seed + 1000) & M64, ids, t, n_agents)


class WindowRun:
    """The C oracle's side of one window of one case at one crossing point: stepped once on its own stream, every step's actions, the
    cells before it and its result kept."""

    def __init__(self, case, X, window, tables=None):
        grid, self.nbr, self.start, self.goal, policy = tables or tables_of(case)
        self.case, self.X, self.window, self.seed, self.t0 = case, X, window, case.seed(X), window.t0
        A, E = case.A, case.E
        self.ids = OFFSET + np.arange(E, dtype=np.uint64)
        co = c_oracle.COracle(self.nbr, A, self.start, self.goal, SLIP, *REWARDS, mo.MAKESPAN, seed=self.seed, env_id_offset=OFFSET)
        co.t = self.t0
        cycle = [streamed_actions(self.seed, self.ids, k, A) for k in range(8)] if window.mode == 'cycle8' else None
        self.acts, self.prevs, self.refs = [], [], []
        for s in range(window.n_steps):
            if window.mode == 'policy':
                a = policy_actions(self.seed, self.ids, co.t, A)
            elif window.mode == 'streamed':
                a = streamed_actions(self.seed, self.ids, co.t, A)
            elif window.mode == 'table':
                a = policy[0][policy[1].astype(np.int64), co.state.astype(np.int64)]
            else:
                a = cycle[s % 8]
            self.prevs.append(co.state.copy())
            self.acts.append(a)
            self.refs.append(co.step(a, auto_reset=True))
        self.state, self.t_end = co.state.copy(), co.t
        assert self.t0 < X < self.t_end

    def totals(self, lo, hi):
        """returns summed left to right from zero, episode and collision counts: what a launch over steps lo .. hi - 1 leaves"""
        E = self.case.E
        ret, epi, col = np.zeros(E), np.zeros(E, np.uint32), np.zeros(E, np.uint32)
        for ref in self.refs[lo:hi]:
            ret = ret + ref['reward']
            epi = epi + ref['done'].astype(np.uint32)
            col = col + ref['collision'].astype(np.uint32)
        return dict(returns=ret, episodes=epi, collisions=col)


@functools.lru_cache(maxsize=4)
def window_run(case, X, name):
    """the runs of a case, shared by the tests of one process that need them"""
    windows = {'S': [step_window(X)], 'G': [graph_window(X)]}.get(name) or rollout_windows(X, case.table)
    return WindowRun(case, X, [w for w in windows if w.name == name][0])


# ----------------------------------------------------------------------- wrong models: what the oracle's output must tell apart
def _model_step(run, s, n, seed=None, ids=None, t=None, acts=None, quad_shift=0):
    """`local` of the first n envs after step s of `run` when the slip uniforms come from (seed, ids, t) and the actions are `acts`
    (default: the run's own): the C oracle stepped from the run's cells before step s with INJECTED uniforms.  quad_shift: every
    agent takes the draw of the agent `quad_shift` quads up (the quad field of counter word 3 is off by that much)."""
    A = run.case.A
    seed = run.seed if seed is None else seed
    ids = run.ids[:n] if ids is None else ids
    t = run.t0 + s if t is None else t
    u = philox.slip_uniforms_np(seed, ids, t, A + 4 * quad_shift)[:, 4 * quad_shift:]
    co = c_oracle.COracle(run.nbr, A, run.start[:n], run.goal[:n], SLIP, *REWARDS, mo.MAKESPAN)
    co.state[:] = run.prevs[s][:n]
    return co.step(run.acts[s][:n] if acts is None else acts, uniforms=np.ascontiguousarray(u), auto_reset=True)['local']


def narrowings(run, n=NARROW_ENVS):
    """{wrong model: (the first step it applies to, the number of the first n envs whose `local` it changes at that step)}.

      seed & 0xFFFFFFFF                 the seed held in 32 bits (the identity for the seed 0xFFFFFFFF: left out there)
      env id & 0xFFFFFFFF               the global env id held in 32 bits (envs 37 .. wrap to 0 ..)
      t - X from step X on              a dropped carry, or a high half held from the launch's start -- below 2^49 only: at X = 2^49
                                        the slip counter of t - X is BY DEFINITION the counter of t (the 16-bit field wraps) ...
      h hi unmasked in the quad field   ... and what a kernel can get wrong there is the mask: (h >> 32) = 0x10000 added into word 3
                                        moves every agent to the next quad's draw (X = 2^49 only)
      policy at t - X from step X on    the policy stream loses its carry while the slip stream is right (in-kernel policy only)
      policy key (seed_lo + 1, seed_hi) the key's 64-bit add done in 32 bits (in-kernel policy, the two seeds whose add carries)
    """
    case, X, seed = run.case, run.X, run.seed
    A, n = case.A, min(n, case.E)
    ids, s_x, policy = run.ids[:n], X - run.t0, run.window.mode == 'policy'
    assert np.array_equal(_model_step(run, 0, n), run.refs[0]['local'][:n])          # the model with nothing narrowed is the run itself
    assert np.array_equal(_model_step(run, s_x, n), run.refs[s_x]['local'][:n])
    found = {}

    def note(name, s, local):
        found[name] = (s, int((local != run.refs[s]['local'][:n]).any(axis=1).sum()))

    if seed >> 32:
        note('seed & 0xFFFFFFFF', 0, _model_step(run, 0, n, seed=seed & M32, acts=policy_actions(seed & M32, ids, run.t0, A) if policy else None))
    low = ids & np.uint64(M32)
    note('env id & 0xFFFFFFFF', 0, _model_step(run, 0, n, ids=low, acts=policy_actions(seed, low, run.t0, A) if policy else None))
    if X < (1 << 49):
        note('t - X from step X on', s_x, _model_step(run, s_x, n, t=0))
    else:
        note('h hi unmasked in the quad field', s_x, _model_step(run, s_x, n, quad_shift=1))
    if policy:
        note('policy at t - X from step X on', s_x, _model_step(run, s_x, n, acts=policy_actions(seed, ids, 0, A)))
        if (seed + 1) & M32 == 0:
            wrong_key = (seed & ~M32 & M64) | ((seed + 1) & M32)                      # (seed_lo + 1 mod 2^32, seed_hi)
            note('policy key (seed_lo + 1, seed_hi)', 0, _model_step(run, 0, n, acts=policy_actions((wrong_key - 1) & M64, ids, run.t0, A)))
    return found


NARROWINGS = ('seed & 0xFFFFFFFF', 'env id & 0xFFFFFFFF', 't - X from step X on', 'h hi unmasked in the quad field',
              'policy at t - X from step X on', 'policy key (seed_lo + 1, seed_hi)')
