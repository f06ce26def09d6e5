"""GPU parity of the packed table-policy rollout under the episode step limit (MAPF_TUNE limit_packed=1; csrc/mapf_lq_limit.hip,
lq_rollout_kernel_table_limit): every packed table instance against the composition of the unchanged C oracle in
tests/episode_limit_cases.py -- cells, flags, the float64 bit patterns of reward / prob / returns, ages and truncation counts, bit
for bit -- and every launch the packed limit launcher must NOT take.  The cases are tests/limit_packed_cases.py's.  Every bad input
here is one the host rejects: nothing provokes a device fault."""
import numpy as np
import pytest

import episode_limit_cases as ec
import limit_packed_cases as lp
from conftest import set_tune
from parity_checks import RECORDED, TOTALS, check_handle, check_record, check_totals, make, raw_bytes

pytestmark = pytest.mark.gpu
LG_LIMIT = ('lg_rollout_kernel', '_limit_guarded<', ',LIMIT>')      # what a lane-group limit instance's name holds


def _tune(monkeypatch, case, table_lds=None, limit_packed=True):
    items = case.tune_items(table_lds)
    if not limit_packed:
        items['limit_packed'] = None
    set_tune(monkeypatch, **items)


def _launch(env, ref, w, n, source='table', auto_reset=True, **kw):
    """one launch of n steps and the reference's n steps (streamed: the reference runs first, its actions are what is streamed)"""
    refs = ref.run(w, source, n, auto_reset=auto_reset) if source == 'stream' else None
    actions = np.stack([r['actions'] for r in refs]).astype(np.uint8) if source == 'stream' else None
    res = env.rollout(n, actions=actions, auto_reset=auto_reset, **kw)
    env.sync()
    return res, (refs if refs is not None else ref.run(w, source, n, auto_reset=auto_reset)), env.last_kernel('rollout')


def _run_pass(w, N, slip, criteria, expect, source='table', auto_reset=True, ages=None, absent=(), **kw):
    """The launch pattern of tests/test_gpu_episode_limit.py's _run_pass: the 36 steps as launches of 5 (recording), 1 (totals only), 18
    (accumulated into the 1's totals) and 12 (recording), then the 12 twice more into the same arrays (out=); everything compared
    after every launch, every kernel name holding all of `expect` and none of `absent`.  Returns the reference steps of the first 36."""
    env, ref = make(w, N, slip, criteria, source, **kw)
    if ages is not None:
        env.episode_steps(set=ages)
        ref.age = ages.copy()
    tag = (w.A, w.E, N, slip, criteria, source, auto_reset)

    def named(got, kind):
        assert kind in got and all(e in got for e in expect) and not any(e in got for e in absent), (tag, got, expect, absent)

    res, refs5, got = _launch(env, ref, w, 5, source, auto_reset, record=True)
    named(got, 'RECORD')
    assert sorted(res) == sorted(RECORDED + TOTALS)
    check_record(res, refs5, tag)
    check_totals(res, ec.totals_of(refs5), tag)
    check_handle(env, ref, tag)
    res, refs1, got = _launch(env, ref, w, 1, source, auto_reset)
    named(got, 'TOTALS')
    assert sorted(res) == sorted(TOTALS)
    base = ec.totals_of(refs1)
    check_totals(res, base, tag)
    check_handle(env, ref, tag)
    res, refs18, got = _launch(env, ref, w, 18, source, auto_reset, accumulate_into=res)
    named(got, 'TOTALS')
    check_totals(res, ec.totals_of(refs18, base), tag)
    check_handle(env, ref, tag)
    out, refs12, got = _launch(env, ref, w, 12, source, auto_reset, record=True)
    named(got, 'RECORD')
    check_record(out, refs12, tag)
    check_totals(out, ec.totals_of(refs12), tag)
    check_handle(env, ref, tag)
    for again in range(2):
        res, more, got = _launch(env, ref, w, 12, source, auto_reset, record=True, out=out)
        assert res is out
        named(got, 'RECORD')
        check_record(out, more, (tag, 'out=', again))
        check_totals(out, ec.totals_of(more), (tag, 'out=', again))
        check_handle(env, ref, (tag, 'out=', again))
    env.close()
    return refs5 + refs1 + refs18 + refs12


PARITY = [(c, lds, 'Makespan') for c in lp.CASES for lds in lp.TABLE_LDS] + [(c, lds, 'SoC') for c in lp.CASES if c.soc for lds in lp.TABLE_LDS]


@pytest.mark.parametrize('case,table_lds,criteria', PARITY, ids=lambda v: getattr(v, 'id', str(v)))
def test_parity_over_every_instance(monkeypatch, case, table_lds, criteria):
    """every row of the case table x both table forms x every (N, slip): the launches cross ages over launch boundaries and every
    phase of the four-step Philox block, and are shorter and longer than the eight-step probability chain of the SYS instance"""
    _tune(monkeypatch, case, table_lds)
    for N, slip in ec.LIMITS:
        w = lp.workload(case.A, case.E, N)
        # (Makespan runs its instance without terminal handling unless some env starts on its goals: a team of four whose random
        # walks all came back, in these workloads)
        starts_terminal = bool((w.start == w.goal).all(axis=1).any())
        assert not starts_terminal or case.A == 4
        no_terminal = ('NO_TERMINAL',) if criteria == 'Makespan' and not starts_terminal else ()
        expect = case.name_parts(table_lds) + ('SOC' if criteria == 'SoC' else 'MAKESPAN',) + no_terminal
        goals, colls, truncs, _ = ec.outcome_counts(_run_pass(w, N, slip, criteria, expect, absent=() if no_terminal else ('NO_TERMINAL',)))
        assert truncs > 0 and goals > 0 and (colls > 0 or (case.A == 32 and N == 1)), (case.id, N, slip, goals, colls, truncs)


@pytest.mark.parametrize('case', lp.TERMINAL_CASES, ids=lambda c: c.id)
def test_terminal_handling(monkeypatch, case):
    _tune(monkeypatch, case)
    N, slip = 4, 0.2
    # every seventh env starts on its goals, auto-reset on: the Makespan TERM instance; those envs only take no-op steps
    w = lp.workload(case.A, case.E, N, True)
    refs = _run_pass(w, N, slip, 'Makespan', case.name_parts(None)[:1] + ('MAKESPAN', ',LIMIT>'), absent=('NO_TERMINAL',))
    assert all(r['was_terminal'][::7].all() and not r['truncated'][::7].any() for r in refs) and ec.outcome_counts(refs)[2] > 0
    # the plain workload without auto-reset: a truncated env lives on and says so on every later live step; a done env stays
    # terminal and keeps its age
    w = lp.workload(case.A, case.E, N)
    refs = _run_pass(w, N, slip, 'Makespan', case.name_parts(None)[:1] + ('MAKESPAN', ',LIMIT>'), auto_reset=False)
    seen, repeats, noops = np.zeros(case.E, bool), 0, 0
    for r in refs:
        later = seen & (r['was_terminal'] == 0) & (r['done'] == 0)
        assert (r['truncated'][later] == 1).all()
        repeats += int(later.sum())
        noops += int(r['was_terminal'].sum())
        seen |= r['truncated'] != 0
    assert repeats > 0 and noops > 0


@pytest.mark.parametrize('case', (lp.BY_ID['k2-8x256'], lp.SYS_CASE, lp.BY_ID['mv_lds_max_bytes1024-32x128']), ids=lambda c: c.id)
def test_a_limit_never_reached_changes_nothing(monkeypatch, case):
    """N = 2^31 with the key set against a handle without a limit: the same outputs and state from packed table kernels whose names
    differ by the limit parts only"""
    _tune(monkeypatch, case)
    w = lp.workload(case.A, case.E, 4)
    for criteria in ('Makespan', 'SoC'):
        limited, _ = make(w, 1 << 31, 0.2, criteria)
        plain, _ = make(w, None, 0.2, criteria)
        for record in (True, False):
            a = limited.rollout(ec.T_TOTAL, record=record)
            b = plain.rollout(ec.T_TOTAL, record=record)
            name, base = limited.last_kernel('rollout'), plain.last_kernel('rollout')
            assert base.startswith('lq_rollout_kernel_table<Q=%d,K=%d,' % (case.Q, case.K)) and 'LIMIT' not in base and 'limit' not in base, base
            # (a kept name is cut at 159 characters: the instance and the block in full, the note as far as both go)
            head, note = name.split(' (', 1)
            assert head.replace('lq_rollout_kernel_table_limit<', 'lq_rollout_kernel_table<').replace(',LIMIT>', '>') == base.split(' (', 1)[0], (name, base)
            assert ('; episode step limit' in note or len(name) == 159) and base.split(' (', 1)[1].startswith(note.split('; episode step limit')[0][:40]), (name, base)
            assert name != base and sorted(b) == sorted(k for k in (RECORDED if record else ()) + TOTALS if not k.startswith('trunc'))
            for key in b:
                assert np.array_equal(raw_bytes(a[key]), raw_bytes(b[key])), (case.id, criteria, record, key)
            assert not a['truncations'].any() and not (record and a['truncated'].any())
            assert np.array_equal(limited.get_state()[0], plain.get_state()[0]) and limited.t == plain.t
        assert not plain.episode_steps().any()
        limited.close()
        plain.close()


def test_ages_saturate(monkeypatch):
    """N = 2^32 - 1, ages set to 2^32 - 3 + e % 3, no auto-reset: an age stops at 2^32 - 1 and truncates from there on"""
    case = lp.BY_ID['k2-16x128']
    _tune(monkeypatch, case)
    N = ec.AGE_MAX
    w = lp.workload(case.A, case.E, 4)
    ages = (N - 2 + np.arange(case.E, dtype=np.uint64) % 3).astype(np.uint32)
    refs = _run_pass(w, N, 0.2, 'Makespan', case.name_parts(None)[:1], auto_reset=False, ages=ages)
    first = refs[0]
    running = (first['was_terminal'] == 0) & (first['done'] == 0)
    # (the first step: the ages that began at 2^32 - 2 reach the limit, those at 2^32 - 1 stay there; those at 2^32 - 3 are one short)
    assert np.array_equal(first['truncated'][running] != 0, (np.arange(case.E) % 3 != 0)[running]) and running.sum() > case.E // 2
    final = w.oracle(N, 0.2)
    final.age = ages.copy()
    final.run(w, 'table', 2, auto_reset=False)
    assert (final.age == N).any() and (final.age <= N).all()


FALLBACKS = ('stream', 'policy', 'greedy', 'ragged', 'lane_group', 'no_key')


@pytest.mark.parametrize('what', FALLBACKS)
def test_fallbacks_stay_with_the_lane_group_limit_instance(monkeypatch, what):
    """with the key set, streamed, random-policy and greedy launches, a ragged batch and a handle created with kernel='lane_group' --
    and a table launch without the key -- run the lane-group limit instance, bit-exact against the reference"""
    case = lp.BY_ID['k2-8x256']
    _tune(monkeypatch, case, limit_packed=what != 'no_key')
    source = what if what in ec.SOURCES else 'table'
    w = lp.workload(case.A, case.E + (1 if what == 'ragged' else 0), 4)
    kw = dict(kernel='lane_group') if what == 'lane_group' else {}
    refs = _run_pass(w, 4, 0.2, 'Makespan', LG_LIMIT + ('_table' if source == 'table' else 'lg_rollout_kernel_limit_guarded<',), source=source, **kw)
    assert ec.outcome_counts(refs)[2] > 0


def test_device_arrays_with_env_ids_beyond_32_bits(monkeypatch):
    case = lp.BY_ID['k4-8x512']
    _tune(monkeypatch, case)
    w = lp.workload(case.A, case.E, 4)
    refs = _run_pass(w, 4, 0.2, 'Makespan', case.name_parts(None)[:1], device_arrays=True, env_id_offset=(1 << 32) + 5)
    assert ec.outcome_counts(refs)[2] > 0


def test_without_a_limit_the_key_changes_no_launch(monkeypatch):
    """a handle is created under limit_packed=0 and =1 alike, and without a limit both run the same packed table kernel"""
    case = lp.BY_ID['k2-8x256']
    w = lp.workload(case.A, case.E, 4)
    names = []
    for value in (0, 1):
        set_tune(monkeypatch, k=2, limit_packed=value)
        env, _ = make(w, None, 0.2)
        env.rollout(4)
        names.append(env.last_kernel('rollout'))
        env.close()
    assert names[0] == names[1] and names[0].startswith('lq_rollout_kernel_table<Q=4,K=2,')
