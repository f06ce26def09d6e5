"""The totals-only sweep (``rollout(record=False)``): its case table and its oracle side, shared by tests/test_totals_cases.py (no
GPU: the ledger, the reachability of every case and the proof that its inputs can show an error) and tests/test_gpu_totals.py
(every case on the GPU against the values built here).  A plain module, not a conftest.

Every packed rollout instance is compiled once for RECORD and once for TOTALS; the launcher picks one of six TOTALS instances per
(K, Q, TableForm) -- {STREAM, POLICY} x {SOC, MAKESPAN, MAKESPAN + NO_TERMINAL} -- so the 20 entries of MAPF_LQ_ROLLOUT_INSTANCES
are 120 TOTALS instances, and the six passes below name the six of a case one to one (SOC instances always handle terminal
states: the launcher folds nothing).  Lane-group and thread-per-env cases run the four passes of the random-map family."""
import math
from fractions import Fraction

import numpy as np

import c_oracle
import mapf_oracle as mo
import philox
from gym_mapf_amd.envs.grid import MapfGrid
from parity_checks import EXACT, INEXACT, bits

SLIP = {EXACT: 0.2, INEXACT: 0.15}

# the ABI's form numbers (mapf_layout.hpp TableForm) and what a packed kernel's name says about each: (COMPACT, the form's tag)
FORMS = ('FullRows', 'Rows8', 'Rows8x4Bitmap', 'Rows8x5Bitmap', 'FullRowsBitmap', 'DeltaRowsBitmap')
FORM_NAME = {'FullRows': ('', ''), 'Rows8': (',COMPACT', ''), 'Rows8x4Bitmap': (',COMPACT', ',BITMAP'), 'Rows8x5Bitmap': (',COMPACT', ',BITMAP5'),
             'FullRowsBitmap': ('', ',BITMAP'), 'DeltaRowsBitmap': (',COMPACT', ',BITMAPD')}

FIRST_STEP = 3                        # every pass starts off the slip stream's four-step boundary
LENGTHS = (1, 6, 9)                   # a plain launch, then two that accumulate into its totals
LENGTHS_CHAIN = (8, 1, 16)            # ... of the systolic RECORD instances' chain length, one shorter and two chains (32 agents, Q = 16)
OVERWRITE_STEPS, RECORD_STEPS = 5, 4  # a plain launch with out= the accumulated totals; pass 1's last launch records
MIN_TIES, TIE_EXEMPT_BELOW = 4, 250000


class Case:
    """One row of the table: the batch, the MAPF_TUNE keys that pin the kernel form and what the kernel's name must say."""

    def __init__(self, n_agents, n_envs, tune=None, K=None, Q=None, form=None, kernel='auto', lg=None, seed=0):
        self.A, self.E, self.tune, self.K, self.Q, self.form, self.kernel, self.lg = n_agents, n_envs, dict(tune or {}), K, Q, form, kernel, lg
        self.packed = K is not None
        self.seed = seed              # (moves every seed of the case: the way to repair a case whose inputs could not show an error)
        assert not self.packed or (K * Q == n_agents and form in FORMS)

    @property
    def id(self):
        if self.packed:
            return 'K%d-Q%d-%s' % (self.K, self.Q, self.form)
        return '%s-A%d-E%d' % ('tpe' if self.kernel == 'thread_per_env' else 'lg', self.A, self.E)

    @property
    def passes(self):
        return (1, 2, 3, 4, 5, 6) if self.packed else (1, 2, 4, 6)

    @property
    def chain_pass(self):
        """pass 1 runs a second time with LENGTHS_CHAIN in the 32-agent and the Q = 16 cases"""
        return self.packed and (self.A == 32 or self.Q == 16)

    @property
    def agent_steps(self):
        return self.A * self.E * (sum(LENGTHS) + OVERWRITE_STEPS) * len(self.passes)

    @property
    def tie_exempt(self):
        return not self.packed and self.agent_steps < TIE_EXEMPT_BELOW

    @property
    def soc_counts_apply(self):
        """Two agents have the counts A - stayed = 2 and 1 only (both staying on their goals is a terminal state), and no n <= 2
        at which n * living + r_x rounds twice: the SoC rounding condition cannot hold for them."""
        return self.A >= 3

    @property
    def ends_at_once_without_reset(self):
        """64 and more agents on the at most 490 free cells of a family R map, moved by the random policy: every env has a
        collision within its first two steps (about 2.5 colliding pairs are expected per step at 64 agents, 10 at 128), so
        without auto-reset a return has at most two non-zero terms and every order of summation gives the same bits.  No seed
        changes that; the conditions on the return chain are asserted in the case's auto-reset passes (2, 3 and 4) only."""
        return self.A >= 64

    def tune_text(self):
        return ','.join('%s=%s' % kv for kv in self.tune.items())

    def kernel_name(self, p):
        """what mapf_last_kernel must begin with after a totals-only launch of pass `p`"""
        stream = 'STREAM' if p.streamed else 'POLICY'
        if self.packed:
            compact, tag = FORM_NAME[self.form]
            crit = 'SOC' if p.soc else 'MAKESPAN'
            no_terminal = ',NO_TERMINAL' if (not p.soc and p.auto_reset and not p.start_terminal) else ''
            return 'lq_rollout_kernel<Q=%d,K=%d,TOTALS,%s,%s%s%s%s> block=' % (self.Q, self.K, stream, crit, compact, no_terminal, tag)
        if self.kernel == 'thread_per_env':
            return 'rollout_kernel<A=%d> block=' % self.A              # (one instance, recording or not, streamed or not)
        L, full, mv = self.lg
        return 'lg_rollout_kernel<L=%d,%s,%s,TOTALS,%s,' % (L, full, mv, stream)


def _packed(K, Q, form, n_envs, **tune):
    return Case(K * Q, n_envs, tune, K=K, Q=Q, form=form)


# One entry per (K, Q, TableForm) of MAPF_LQ_ROLLOUT_INSTANCES, in its order, at the smallest full-block batch of each form (the
# shapes of test_goal_reaching_episodes_against_c_oracle: 2048 envs at 32 agents, 4096 at 16, 8192 .. 16448 at 8, 16384 at 4;
# 1024 at 64).  mv_lds_max_bytes=2048 declares the full table too large: the 8-byte (and 4-byte) rows.
PACKED_CASES = [
    _packed(8, 4, 'Rows8', 2048, mv_lds_max_bytes=2048, k=8), _packed(8, 1, 'FullRows', 8192, k=8), _packed(8, 2, 'FullRows', 4096, k=8),
    _packed(8, 4, 'FullRows', 2048, k=8),
    _packed(4, 8, 'DeltaRowsBitmap', 2048, mv_lds_max_bytes=2048), _packed(4, 8, 'FullRowsBitmap', 2048, k=4),
    _packed(4, 8, 'Rows8x5Bitmap', 2048, mv_lds_max_bytes=2048, bitmap_delta=0),
    _packed(4, 8, 'Rows8x4Bitmap', 2048, mv_lds_max_bytes=2048, bitmap_staycol=0, bitmap_delta=0),
    _packed(4, 4, 'Rows8', 4096, mv_lds_max_bytes=2048), _packed(4, 8, 'Rows8', 2048, mv_lds_max_bytes=2048, bitmap_pairs=0),
    _packed(4, 16, 'Rows8', 1024, mv_lds_max_bytes=2048),
    _packed(4, 1, 'FullRows', 16384, k=4), _packed(4, 2, 'FullRows', 8192, k=4), _packed(4, 4, 'FullRows', 4096, k=4),
    _packed(4, 8, 'FullRows', 2048, k=4, bitmap_pairs=0), _packed(4, 16, 'FullRows', 1024, k=4),
    _packed(2, 2, 'FullRows', 16512, k=2), _packed(2, 4, 'FullRows', 16448, k=2), _packed(2, 8, 'FullRows', 4128, k=2),
    _packed(2, 16, 'FullRows', 1024, k=2),
]
# Lane-group and thread-per-env: every group size, ragged groups, ragged last blocks, the move table in LDS and in global memory.
# lg = (L, FULL | RAGGED, MV_LDS | MV_GLOBAL).  (16 agents x 512 envs would run the packed K = 2 form: quad_lanes=0 keeps it here.)
# Cases below TIE_EXEMPT_BELOW agent-steps (3 x 257 and 8 x 300) are exempt from the slip-tie count: Case.tie_exempt.
LANE_GROUP_CASES = [
    Case(2, 2048, kernel='lane_group', lg=(1, 'FULL', 'MV_GLOBAL')), Case(3, 257, kernel='lane_group', lg=(2, 'RAGGED', 'MV_GLOBAL')),
    Case(5, 600, lg=(4, 'RAGGED', 'MV_GLOBAL')), Case(7, 1000, lg=(4, 'RAGGED', 'MV_GLOBAL')), Case(8, 300, lg=(4, 'FULL', 'MV_GLOBAL')),
    Case(8, 16448, {'quad_lanes': 0}, lg=(4, 'FULL', 'MV_LDS')), Case(16, 512, {'quad_lanes': 0}, lg=(8, 'FULL', 'MV_GLOBAL')),
    Case(32, 1024, {'mv_lds_max_bytes': 0}, lg=(16, 'FULL', 'MV_GLOBAL')), Case(33, 100, lg=(32, 'RAGGED', 'MV_GLOBAL')),
    Case(64, 512, lg=(32, 'FULL', 'MV_LDS')), Case(128, 256, lg=(64, 'FULL', 'MV_LDS')),
    Case(6, 512, kernel='thread_per_env'),
]
CASES = PACKED_CASES + LANE_GROUP_CASES


class Pass:
    """One row of the pass table: how the actions arrive, criteria, auto-reset, start-terminal envs, constants, map family."""

    def __init__(self, number, mode, soc, auto_reset, start_terminal, rewards, family, lengths=LENGTHS, record_tail=False):
        self.number, self.mode, self.soc, self.auto_reset, self.start_terminal = number, mode, soc, auto_reset, start_terminal
        self.rewards, self.fail_prob, self.family, self.lengths, self.record_tail = rewards, SLIP[rewards], family, lengths, record_tail
        self.streamed = mode.startswith('streamed')
        self.policy = None if self.streamed else mode                 # what set_policy gets

    @property
    def tag(self):
        return 'pass %s' % (self.number if self.lengths == LENGTHS else '%d (launches of %r)' % (self.number, self.lengths))


PASSES = {
    1: Pass(1, 'streamed', False, True, False, EXACT, 'R', record_tail=True),
    2: Pass(2, 'streamed', False, True, True, INEXACT, 'R'),
    3: Pass(3, 'streamed greedy', True, True, False, INEXACT, 'G'),
    4: Pass(4, 'random', False, True, False, INEXACT, 'R'),
    5: Pass(5, 'greedy', False, False, False, EXACT, 'G'),
    6: Pass(6, 'random', True, False, False, INEXACT, 'R'),
}
CHAIN_PASS = Pass(1, 'streamed', False, True, False, EXACT, 'R', lengths=LENGTHS_CHAIN)


def passes_of(case):
    return [PASSES[n] for n in case.passes] + ([CHAIN_PASS] if case.chain_pass else [])


# ----------------------------------------------------------------------- the two map families
def _goal_scenario_tables(n_agents, n_envs, seed):
    import goal_scenarios
    lines, start_loc, goal_loc = goal_scenarios.goal_scenario(n_agents, n_envs, seed)
    grid = MapfGrid(lines)
    valid, l2i, nbr = grid.tables()
    ids = np.zeros((len(lines), len(lines[0])), np.uint16)
    for loc, k in l2i.items():
        ids[loc] = k
    start = np.ascontiguousarray(ids[start_loc[..., 0], start_loc[..., 1]])
    goal = np.ascontiguousarray(ids[goal_loc[..., 0], goal_loc[..., 1]])
    rc = np.asarray([r | (c << 16) for r, c in valid], np.uint32)
    return grid, nbr, rc, start, goal


def _random_map_tables(n_agents, n_envs, seed):
    """Family R: a seeded random map with walls, 20x20 .. 24x24 at p = 0.15 (delta rows apply; merged movement lists occur away
    from the border), random distinct start cells and random distinct goal cells per env.  Every eighth env (e % 8 == 3) is
    a NEAR env: every agent but the last starts on its goal and the last one move from its goal, so that streamed greedy actions
    end its episodes on goals and random ones give many counts A - stayed."""
    rs = np.random.RandomState([seed, n_agents, n_envs])
    side = 20 + seed % 5
    grid = MapfGrid([''.join('@' if rs.rand() < 0.15 else '.' for _ in range(side)) for _ in range(side)])
    valid, _, nbr = grid.tables()
    V, E, A = len(valid), n_envs, n_agents
    start = np.argsort(rs.rand(E, V), axis=1)[:, :A].astype(np.uint16)
    goal = np.argsort(rs.rand(E, V), axis=1)[:, :A].astype(np.uint16)
    near = np.arange(3, E, 8)
    for e in near:
        goal[e, :A - 1] = start[e, :A - 1]
        taken = set(start[e, :A - 1].tolist())
        for g in rs.permutation(V).tolist():
            free = [int(n) for n in nbr[g, 1:5] if int(n) != g and int(n) not in taken]
            if g not in taken and free:
                goal[e, A - 1], start[e, A - 1] = g, free[0]
                break
        else:
            raise AssertionError('no room for a near env')
    rc = np.asarray([r | (c << 16) for r, c in valid], np.uint32)
    return grid, nbr, rc, start, goal, near


class Tables:
    """The two families of a case, built once and shared by its passes (never written after this)."""

    def __init__(self, case):
        self.case = case
        self.R = _random_map_tables(case.A, case.E, 500 + case.seed)
        self.G = _goal_scenario_tables(case.A, case.E, 8100 + case.A + case.seed) + (np.zeros(0, np.int64),) if case.packed else None

    def of(self, p):
        grid, nbr, rc, start, goal, near = self.R if p.family == 'R' else self.G
        if p.start_terminal:
            goal = goal.copy()
            goal[::7] = start[::7]                                    # every seventh env starts (and restarts) terminal
        return grid, nbr, rc, start, goal, near


class PassRun:
    """The C oracle's side of one pass of one case: stepped once, launch by launch, every step's result kept."""

    def __init__(self, case, p, tables):
        self.case, self.p = case, p
        self.grid, self.nbr, self.rc, self.start, self.goal, near = tables.of(p)
        A, E = case.A, case.E
        self.seed, self.offset = 31 + 10 * case.seed + p.number + (100 if p.lengths != LENGTHS else 0), 5
        self.ocrit = mo.SOC if p.soc else mo.MAKESPAN
        co = c_oracle.COracle(self.nbr, A, self.start, self.goal, p.fail_prob, *p.rewards, self.ocrit, seed=self.seed, env_id_offset=self.offset)
        co.t = FIRST_STEP
        ids = self.offset + np.arange(E)
        self.ids = ids
        # launches: (kind, n_steps); every step's actions, the oracle's cells before it and its result; cells and t after each launch
        self.launches = [('first', p.lengths[0])] + [('accumulate', n) for n in p.lengths[1:]] + [('overwrite', OVERWRITE_STEPS)] + \
            ([('record', RECORD_STEPS)] if p.record_tail else [])
        self.acts, self.prevs, self.refs, self.after = [], [], [], []
        for _, n in self.launches:
            for _ in range(n):
                if p.mode == 'random':
                    a = philox.random_actions_np(self.seed, ids, co.t, A)        # the in-kernel policy stream
                elif p.mode == 'streamed':
                    a = philox.random_actions_np(self.seed + 1000, ids, co.t, A)  # any stream will do: not the in-kernel one
                    if len(near):
                        a[near] = co.greedy_actions(self.rc)[near]
                else:
                    a = co.greedy_actions(self.rc)
                self.prevs.append(co.state.copy())
                self.acts.append(a)
                self.refs.append(co.step(a, auto_reset=p.auto_reset))
            self.after.append((co.state.copy(), co.t))
        self.n_totals_steps = sum(p.lengths)

    def steps_of(self, k):
        lo = sum(n for _, n in self.launches[:k])
        return lo, lo + self.launches[k][1]

    def actions_of(self, k):
        lo, hi = self.steps_of(k)
        return np.stack(self.acts[lo:hi]) if self.p.streamed else None

    def totals(self, lo, hi, base=None):
        """returns summed left to right from `base` (zero), episode and collision counts: what a launch over steps lo .. hi - 1 leaves"""
        E = self.case.E
        ret = np.zeros(E) if base is None else base['returns'].copy()
        epi = np.zeros(E, np.uint32) if base is None else base['episodes'].copy()
        col = np.zeros(E, np.uint32) if base is None else base['collisions'].copy()
        for ref in self.refs[lo:hi]:
            ret = ret + ref['reward']                                 # float64 adds in step order, as the kernels do
            epi = epi + ref['done'].astype(np.uint32)
            col = col + ref['collision'].astype(np.uint32)
        return dict(returns=ret, episodes=epi, collisions=col)


# ----------------------------------------------------------------------- what the oracle's output must contain
def _assert_a_wrong_rounding_would_show(refs, prevs, acts, goal, rewards, soc, fail_prob, tag):
    """On the ORACLE's output alone: this pass would not equally accept a reordered return or a fused / re-associated
    ``n * r_living + r_x``.  ``prevs[t]`` = the oracle's cells before step t, ``acts[t]`` its actions, ``refs[t]`` its results."""
    r_clash, r_goal, r_living = rewards
    T, (E, A) = len(refs), goal.shape
    rew = np.stack([ref['reward'] for ref in refs])
    ret = np.zeros(E)
    for t in range(T):
        ret = ret + rew[t]                                        # the reference's order: left to right
    reordered = sum(1 for e in range(E) if math.fsum(rew[:, e].tolist()) != ret[e])
    # waived without slip: every agent starts one move from its goal, so every episode ends at its first step and the
    # three-step pass sums three terms from {r_goal + living, r_clash + living}
    assert fail_prob == 0.0 or reordered > 0, tag
    if not soc:
        return
    counts, two_roundings = set(), 0
    for t in range(T):
        fresh = refs[t]['was_terminal'] == 0
        n = A - ((prevs[t] == goal) & (acts[t] == 0)).sum(axis=1)                 # A - stayed, from the oracle's state
        counts.update(n[fresh].tolist())
        on_goal = fresh & (refs[t]['done'] == 1) & (refs[t]['collision'] == 0)
        for base, sel in ((r_clash, fresh & (refs[t]['collision'] == 1)), (r_goal, on_goal)):
            for k in np.unique(n[sel]).tolist():
                exact = float(Fraction(k) * Fraction(r_living) + Fraction(base))   # n * r_living + r_x, rounded once
                got = refs[t]['reward'][sel & (n == k)]
                assert np.array_equal(bits(got), bits(np.full(got.shape, base + float(k) * r_living))), (tag, t, k)   # n is the oracle's n
                two_roundings += int((got != exact).sum())
    assert two_roundings > 0 and len(counts) >= 3, (tag, two_roundings, sorted(counts))       # (no waiver: see the caller)


def soc_counts(run, n_steps):
    """the counts A - stayed of the non-terminal env-steps of the first `n_steps` steps (as _assert_a_wrong_rounding_would_show counts them)"""
    counts = set()
    for t in range(n_steps):
        n = run.case.A - ((run.prevs[t] == run.goal) & (run.acts[t] == 0)).sum(axis=1)
        counts.update(n[run.refs[t]['was_terminal'] == 0].tolist())
    return counts


def slip_ties(run, thresholds16, enough):
    """agent-steps of non-terminal envs whose uniform's top 16 bits equal those of a threshold -- the kernels' 53-bit refinement
    path -- counted step by step until `enough` are found"""
    ties, t = 0, FIRST_STEP
    for ref in run.refs:
        if ties >= enough:
            break
        hi16 = np.floor(philox.slip_uniforms_np(run.seed, run.ids, t, run.case.A) * 65536.0).astype(np.int64)
        ties += int(np.isin(hi16[ref['was_terminal'] == 0], thresholds16).sum())
        t += 1
    return ties
