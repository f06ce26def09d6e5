"""The packed single step (csrc/mapf_lq_step.hip) in every instance the launcher holds, and the resident forms' chunk walk: the case
table and its oracle side, shared by tests/test_step_cases.py (no GPU: every case plans the instance it declares, the table names all
84 kernels, the oracle's output of every pass contains what makes a wrong kernel show) and tests/test_gpu_step_forms.py (every handle
of every case on the GPU against the values built here).  A plain module, not a conftest.

MAPF_LQ_STEP_INSTANCES (mapf_layout.hpp) lists 21 (Q, K, StepForm) entries; the launcher compiles each with and without the scenario
table (SCEN) and with and without is_terminal(prev) (NO_TERMINAL): 84 kernels.  An INSTANCE case is one entry at the shape and tune
of tests/golden/lq_step_kernel_names.json; a CHUNK-WALK case is a resident form at a batch of seven chunks whose grid MAPF_TUNE
step_grid=1|2|3 cuts to one, two or three blocks, which then walk 7, 4 + 3 and 3 + 2 + 2 chunks (the device's CU count would give
every chunk a block of its own).

Per case four handles -- {scenario table, scen_table=0} x the two passes below -- of twelve steps each, under an auto-reset schedule
that launches both the terminal-testing and the NO_TERMINAL instance several times, with a set_state in the middle.  The two handles
of a pass differ in how the kernel finds its start / goal rows and in nothing the oracle sees: one oracle run serves both.

A 16-bit slip tie (a uniform whose top 16 bits equal a threshold's: slip_move_exact_members, about one agent-step in 2^15) must
occur at least MIN_TIES times among the non-terminal envs of every pass.  No small batch does that by chance, so each pass's seed
is the first of SEEDS_SEARCHED that does (`python tests/step_cases.py --search` prints the table below; a case whose shape no seed
serves doubles its batch, keeping the form's divisibility rule).  Nothing is searched at test time."""
import functools
import sys
from fractions import Fraction

import numpy as np

if __name__ == '__main__':
    import conftest  # noqa: F401  (the paths of the oracle and the package)

import c_oracle
import episode_limit_cases as ec
import mapf_oracle as mo
import philox
from totals_cases import EXACT, INEXACT, SLIP

STEP_FORMS = ('Plain', 'FullRows', 'DeltaRows', 'DeltaRowsBitmap')     # StepForm's numbers (mapf_layout.hpp)
OFFSET = 5                                                             # env_id_offset of every handle
MIN_TIES = 3
SEEDS_SEARCHED = range(1, 401)
N_SCENARIOS = 5
# auto_reset of the twelve steps (the schedule of test_step_drops_is_terminal_only_when_no_env_can_be_terminal, one step longer)
SCHEDULE = (True, True, True, False, False, True, True, 'set_state', True, True, False, True, True)
N_STEPS = sum(1 for what in SCHEDULE if what != 'set_state')
WALK_CHUNKS, WALK_GRIDS = 7, (1, 2, 3)
WALK_PATTERNS = {1: (7,), 2: (4, 3), 3: (3, 2, 2)}                     # chunks per block: block b takes chunks b, b + grid, ...


class Pass:
    def __init__(self, name, soc, rewards):
        self.name, self.soc, self.rewards, self.fail_prob = name, soc, rewards, SLIP[rewards]
        self.criteria = 'SoC' if soc else 'Makespan'


PASSES = (Pass('makespan', False, EXACT), Pass('soc', True, INEXACT))


def step_plan():
    """[(auto_reset, may_be_terminal, set_state_before)] of the twelve steps: a step may meet a terminal env exactly after a step
    without auto-reset or after set_state (no scenario starts terminal, so the first step cannot)"""
    steps, may, set_before = [], False, False
    for what in SCHEDULE:
        if what == 'set_state':
            may = set_before = True
            continue
        steps.append((what, may, set_before))
        may, set_before = not what, False
    return steps


class Case:
    """One row of the table: the instance, its batch, the MAPF_TUNE keys that pin it, the two passes' seeds."""

    def __init__(self, form, K, Q, n_envs, tune, seeds, step_grid=None):
        self.form, self.K, self.Q, self.A, self.E, self.tune, self.seeds, self.step_grid = form, K, Q, K * Q, n_envs, tune, tuple(seeds), step_grid
        self.key = '%s-K%d-Q%d' % (STEP_FORMS[form], K, Q)           # its entry of lq_step_kernel_names.json
        self.walk = step_grid is not None
        self.id = self.key + ('-grid%d' % step_grid if self.walk else '')

    def tune_items(self, scen):
        """MAPF_TUNE of a handle, as keywords for conftest.set_tune"""
        items = dict(item.split('=') for item in self.tune.split(',') if item)
        if self.walk:
            items['step_grid'] = str(self.step_grid)
        if not scen:
            items['scen_table'] = '0'
        return items

    def tune_text(self, scen, grid=True):
        items = self.tune_items(scen)
        if not grid:
            items.pop('step_grid', None)
        return ','.join('%s=%s' % kv for kv in items.items())

    def seed(self, p):
        return self.seeds[PASSES.index(p)]

    def run(self, p):
        return pass_run(self.A, self.E, p.name, self.seed(p))

    @property
    def handles(self):
        return [(scen, p) for scen in (True, False) for p in PASSES]


# (form, K, Q, E, tune, (makespan seed, soc seed)): LQ_STEP_LAUNCHES of tests/plan_sweeps.py, entry by entry (held against
# it by tests/test_step_cases.py; no case had to double its batch).  Seeds: the search's output.
INSTANCE_CASES = [Case(*row) for row in (
    (0, 4, 1, 512, '', (76, 52)), (0, 4, 2, 256, '', (39, 43)), (0, 4, 4, 128, '', (14, 26)), (0, 4, 8, 64, '', (14, 31)), (0, 4, 16, 64, '', (7, 3)),
    (0, 2, 2, 256, 'k=2', (253, 52)), (0, 2, 4, 128, 'k=2', (253, 50)), (0, 2, 8, 64, 'k=2', (14, 50)), (0, 2, 16, 64, 'k=2', (14, 31)),
    (1, 4, 1, 1024, 'step_big=2,k=4', (3, 5)), (1, 4, 2, 512, 'step_big=2,k=4', (19, 1)), (1, 4, 4, 256, 'step_big=2,k=4', (13, 1)),
    (1, 4, 8, 128, 'step_big=2,k=4', (9, 3)),
    (1, 8, 1, 1024, 'step_big=2', (1, 1)), (1, 8, 2, 512, 'step_big=2', (5, 1)), (1, 8, 4, 256, 'step_big=2', (6, 1)),
    (2, 4, 1, 512, 'step_delta=2,bitmap_pairs=0', (76, 52)), (2, 4, 2, 256, 'step_delta=2,bitmap_pairs=0', (39, 43)),
    (2, 4, 4, 128, 'step_delta=2,bitmap_pairs=0', (14, 26)), (2, 4, 8, 64, 'step_delta=2,bitmap_pairs=0', (14, 31)),
    (3, 4, 8, 64, 'step_delta=2', (14, 31)),
)]
# the chunk walk: seven chunks of the form's block (1024 threads over the 16-byte rows, 512 over the delta rows) per batch
_WALKS = (
    (1, 8, 1, 7168, 'step_big=2', (1, 1)), (1, 8, 4, 1792, 'step_big=2', (1, 1)), (1, 4, 2, 3584, 'step_big=2,k=4', (1, 1)),
    (2, 4, 2, 1792, 'step_delta=2,bitmap_pairs=0', (1, 1)), (3, 4, 8, 448, 'step_delta=2', (1, 1)),
)
WALK_CASES = [Case(*row, step_grid=grid) for row in _WALKS for grid in WALK_GRIDS]
CASES = INSTANCE_CASES + WALK_CASES
GRAPH_CASE = WALK_CASES[1]                   # FullRows K = 8, Q = 1 under step_grid=2
GRAPH_NODES, GRAPH_REPLAYS, GRAPH_PLAIN = 6, 2, 2
assert (GRAPH_CASE.key, GRAPH_CASE.step_grid) == ('FullRows-K8-Q1', 2)


# ----------------------------------------------------------------------- the map and the five scenarios
@functools.lru_cache(maxsize=None)
def the_map():
    """(grid, nbr, cell_rc): the 20 x 20 random map of the limit cases and the name fixtures, V = 341 (delta rows apply)"""
    grid = ec.random_map(3)
    valid, _, nbr = grid.tables()
    nbr = np.ascontiguousarray(nbr, np.uint16)
    nbr.setflags(write=False)
    return grid, nbr, np.asarray([r | (c << 16) for r, c in valid], np.uint32)


def _one_move_rows(nbr, A, rs, shared_goal):
    """A start row and a goal row, every agent one move from its goal, all cells distinct (shared_goal: agent 1's goal is agent 0's,
    its start the opposite neighbour).  An agent that slips leaves its start sideways: the pairs are taken so that, while there is
    room, nobody starts or ends where another agent may slip to -- a large team would otherwise never reach its goals together."""
    V = nbr.shape[0]
    nb = nbr.astype(np.int64)
    start, goal, occupied, slips = [], [], set(), set()
    if shared_goal:
        for g in rs.permutation(V).tolist():
            for d in (1, 2):
                a, b = int(nb[g, d]), int(nb[g, d + 2])
                if a != g and b != g and a != b:
                    start, goal, occupied = [a, b], [g, g], {a, b, g}
                    break
            if start:
                break
        assert start, 'no cell with two opposite free neighbours'
    pairs = [(g, d) for g in range(V) for d in (1, 2, 3, 4) if int(nb[g, d]) != g]
    order = rs.permutation(len(pairs)).tolist()
    for strict in (True, False):
        for i in order:
            if len(start) == A:
                break
            g, d = pairs[i]
            s = int(nb[g, d])
            move = (d + 1) % 4 + 1                                   # the action that takes s to g: the opposite of d
            assert int(nb[s, move]) == g
            side = {int(nb[s, move % 4 + 1]), int(nb[s, (move + 2) % 4 + 1])} - {s}
            if s in occupied or g in occupied:
                continue
            if strict and (s in slips or g in slips or side & occupied):
                continue
            start.append(s); goal.append(g)
            occupied |= {s, g}
            slips |= side
    assert len(start) == A, 'no room for %d agents one move from their goals' % A
    return start, goal


@functools.lru_cache(maxsize=None)
def scenarios(A):
    """(start u16[5, A], goal u16[5, A]): scenarios 0 .. 2 one move from every goal, scenario 2 with a shared goal cell (as
    oracle/goal_scenarios.py has it), scenarios 3 and 4 random distinct starts and random distinct goals.  None starts terminal."""
    nbr = the_map()[1]
    V = nbr.shape[0]
    rs = np.random.RandomState([4100, A])
    start, goal = np.zeros((N_SCENARIOS, A), np.uint16), np.zeros((N_SCENARIOS, A), np.uint16)
    for s in range(3):
        start[s], goal[s] = _one_move_rows(nbr, A, rs, shared_goal=(s == 2))
    for s in (3, 4):
        start[s], goal[s] = rs.permutation(V)[:A], rs.permutation(V)[:A]
    for s in range(N_SCENARIOS):
        assert len(set(start[s].tolist())) == A and (start[s] != goal[s]).any()          # not terminal
    start.setflags(write=False); goal.setflags(write=False)
    return start, goal


def scenario_of(E):
    return (np.arange(E) * 7 + 3) % N_SCENARIOS


def rows_of(A, E):
    """(start u16[E, A], goal u16[E, A]): the five scenarios dealt to the envs, as launch_lq_step deals its rows"""
    start, goal = scenarios(A)
    which = scenario_of(E)
    return np.ascontiguousarray(start[which]), np.ascontiguousarray(goal[which])


# ----------------------------------------------------------------------- the oracle's side
class PassRun:
    """The C oracle's side of one pass at one shape: stepped once through the schedule, every step's actions, the cells before it,
    its result and the state and step index after it kept."""

    def __init__(self, A, E, p, seed):
        grid, nbr, cell_rc = the_map()
        self.A, self.E, self.p, self.seed = A, E, p, seed
        self.start, self.goal = rows_of(A, E)
        self.ids = OFFSET + np.arange(E, dtype=np.uint64)
        co = c_oracle.COracle(nbr, A, self.start, self.goal, p.fail_prob, *p.rewards, mo.SOC if p.soc else mo.MAKESPAN, seed=seed, env_id_offset=OFFSET)
        self.acts, self.prevs, self.refs, self.after, self.set_states = [], [], [], [], {}
        for s, (auto_reset, _, set_before) in enumerate(step_plan()):
            if set_before:                                           # every fourth env onto its goal cells: terminal
                state = co.state.copy()
                state[::4] = self.goal[::4]
                co.state[:] = state
                self.set_states[s] = state
            a = philox.random_actions_np(seed, self.ids, co.t, A)
            a[::3] = co.greedy_actions(cell_rc)[::3]
            self.prevs.append(co.state.copy())
            self.acts.append(a)
            self.refs.append(co.step(a, auto_reset=auto_reset))
            self.after.append((co.state.copy(), co.t))


@functools.lru_cache(maxsize=4)
def pass_run(A, E, pass_name, seed):
    """the run of a pass, shared by the handles and cases of one process that need it (never written after this)"""
    return PassRun(A, E, {p.name: p for p in PASSES}[pass_name], seed)


class GraphRun:
    """GRAPH_CASE's makespan handle in device mode: GRAPH_NODES recorded steps (fixed action arrays, auto-reset) replayed
    GRAPH_REPLAYS times, then GRAPH_PLAIN plain steps -- 14 oracle steps"""

    def __init__(self):
        case, p = GRAPH_CASE, PASSES[0]
        grid, nbr, cell_rc = the_map()
        self.case, self.p, self.seed = case, p, case.seed(p)
        self.start, self.goal = rows_of(case.A, case.E)
        ids = OFFSET + np.arange(case.E, dtype=np.uint64)
        co = c_oracle.COracle(nbr, case.A, self.start, self.goal, p.fail_prob, *p.rewards, mo.MAKESPAN, seed=self.seed, env_id_offset=OFFSET)
        self.node_acts = [philox.random_actions_np(self.seed, ids, k, case.A) for k in range(GRAPH_NODES)]
        self.refs, self.after = [], []
        for s in range(GRAPH_NODES * GRAPH_REPLAYS + GRAPH_PLAIN):
            self.refs.append(co.step(self.node_acts[s % GRAPH_NODES], auto_reset=True))
            self.after.append((co.state.copy(), co.t))


# ----------------------------------------------------------------------- what the oracle's output must contain
def outcomes(run):
    """counts over the run's steps: goal ends, collision ends, vertex collisions of agents 0 and 1 on the goal cell they share
    (scenario 2), and per step the number of terminal envs"""
    shared = run.goal[:, 0] == run.goal[:, 1]
    goals = colls = on_shared_goal = 0
    terminal = []
    for ref in run.refs:
        fresh = ref['was_terminal'] == 0
        goals += int((fresh & (ref['done'] == 1) & (ref['collision'] == 0)).sum())
        colls += int((fresh & (ref['collision'] == 1)).sum())
        on_shared_goal += int((fresh & (ref['collision'] == 1) & shared & (ref['local'][:, :2] == run.goal[:, :2]).all(axis=1)).sum())
        terminal.append(int(ref['was_terminal'].sum()))
    return dict(goals=goals, collisions=colls, on_shared_goal=on_shared_goal, terminal=terminal)


def soc_counts(run):
    """the counts A - stayed of the run's non-terminal env-steps (totals_cases.soc_counts)"""
    counts = set()
    for prev, a, ref in zip(run.prevs, run.acts, run.refs):
        n = run.A - ((prev == run.goal) & (a == 0)).sum(axis=1)
        counts.update(n[ref['was_terminal'] == 0].tolist())
    return counts


def mantissas(run, s):
    """the 53-bit uniforms of step s as integers, u64[E, A] (slip_uniforms_np is exact: mantissa / 2^53)"""
    return (philox.slip_uniforms_np(run.seed, run.ids, s, run.A) * 9007199254740992.0).astype(np.uint64)


def slip_ties(run, thresholds16):
    """agent-steps of non-terminal envs whose uniform's top 16 bits equal those of a threshold (totals_cases.slip_ties)"""
    ties = 0
    for s, ref in enumerate(run.refs):
        hi16 = (mantissas(run, s) >> np.uint64(37)).astype(np.int64)
        ties += int(np.isin(hi16[ref['was_terminal'] == 0], thresholds16).sum())
    return ties


def exact_thresholds(cums):
    """ceil(cum * 2^53) of every cumulative probability a slip row compares against"""
    found = set()
    for cum in cums:
        x = Fraction(float(cum)) * (1 << 53)
        found.add(-((-x.numerator) // x.denominator))
    return sorted(found)


def tie_outcomes(run, thresholds53):
    """(ties the 53-bit compare resolves as 'threshold not passed', ... as 'passed') among the non-terminal envs"""
    below = passed = 0
    for s, ref in enumerate(run.refs):
        m = mantissas(run, s)[ref['was_terminal'] == 0]
        for thr in thresholds53:
            tied = m[(m >> np.uint64(37)) == np.uint64(thr >> 37)]
            passed += int((tied >= np.uint64(thr)).sum())
            below += int((tied < np.uint64(thr)).sum())
    return below, passed


def _search():
    """prints, per distinct (shape, pass), the first seed of SEEDS_SEARCHED with MIN_TIES ties (the tables above hold the output)"""
    import tempfile
    from host_shim import build_shim, load_shim, slip_rows
    with tempfile.TemporaryDirectory() as tmp:
        shim = load_shim(build_shim(tmp))
        th16 = {}
        for p in PASSES:
            rows = slip_rows(shim, p.fail_prob)[0]
            th16[p.name] = sorted({int(row['th'][k]) for row in rows for k in range(int(row['n']) - 1)})
    seen = set()
    for case in CASES:
        if (case.key, case.E) in seen:
            continue
        seen.add((case.key, case.E))
        found = []
        for p in PASSES:
            for seed in SEEDS_SEARCHED:
                # (an upper bound first: the ties of all envs, terminal or not, need no oracle run)
                most = sum(int(np.isin((philox.slip_uniforms_np(seed, OFFSET + np.arange(case.E, dtype=np.uint64), s, case.A) * 65536.0).astype(np.int64),
                                       th16[p.name]).sum()) for s in range(N_STEPS))
                if most >= MIN_TIES and slip_ties(PassRun(case.A, case.E, p, seed), th16[p.name]) >= MIN_TIES:
                    found.append(seed)
                    break
            else:
                found.append(None)
        print('%-24s E=%-5d seeds=%r' % (case.key, case.E, tuple(found)), flush=True)


if __name__ == '__main__' and sys.argv[1:] == ['--search']:
    _search()
