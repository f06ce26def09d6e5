"""The totals-only fused rollout (``rollout(record=False)``: returns, episodes, collisions and the final state) in every kernel form
it has, against the C oracle stepped with the same actions.  The case table, the passes and the oracle's side are
tests/totals_cases.py; tests/test_totals_cases.py proves without a GPU that every case reaches its kernel and that its inputs
would show a wrong one.  All comparisons are exact: integers and float64 bit patterns.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import totals_cases as tc
from conftest import set_tune
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from parity_checks import bits

pytestmark = pytest.mark.gpu


def _check(res, want, env, run, k, tag):
    assert np.array_equal(bits(res['returns']), bits(want['returns'])), tag
    assert np.array_equal(res['episodes'], want['episodes']) and np.array_equal(res['collisions'], want['collisions']), tag
    cells, t = env.get_state()
    assert t == run.after[k][1] and np.array_equal(cells, run.after[k][0]), tag


@pytest.mark.parametrize('case', tc.CASES, ids=lambda c: c.id)
def test_totals_only_rollout_against_c_oracle(case, monkeypatch):
    """Per pass (tests/totals_cases.py PASSES: streamed actions or an in-kernel policy, both criteria, auto-reset on and off, envs
    that start terminal, constants that round, both map families): from step index 3, a plain launch and two that accumulate into
    its totals, compared after each launch -- returns as float64 bit patterns (one left-to-right chain across the launches),
    episode and collision counts, cells and step index; then a plain launch with out= the accumulated totals, which it must
    overwrite; pass 1 ends with a recorded launch (the handle moves between the TOTALS and the RECORD object).  After every launch
    the library must name the instance the case and the pass declare: the packed cases name all 120 TOTALS instances."""
    set_tune(monkeypatch, **case.tune)
    tables = tc.Tables(case)
    seen = set()
    for p in tc.passes_of(case):
        run = tc.PassRun(case, p, tables)
        env = VecMapfEnv(run.grid, case.A, None, None, p.fail_prob, *p.rewards, OptimizationCriteria.SoC if p.soc else OptimizationCriteria.Makespan,
                         seed=run.seed, env_id_offset=run.offset, start_local=run.start, goal_local=run.goal, kernel=case.kernel)
        if p.policy:
            env.set_policy(p.policy)
        env.set_state(None, t=tc.FIRST_STEP)
        acc = want = None
        for k, (kind, n) in enumerate(run.launches):
            tag = (case.id, p.tag, k, kind, n)
            lo, hi = run.steps_of(k)
            actions = run.actions_of(k)
            if kind == 'first':
                acc = env.rollout(n, actions=actions, auto_reset=p.auto_reset)
                want = run.totals(lo, hi)
            elif kind == 'accumulate':
                res = env.rollout(n, actions=actions, auto_reset=p.auto_reset, accumulate_into=acc)
                assert res is acc
                want = run.totals(lo, hi, base=want)              # the chain goes on: not (old total) + (this launch from zero)
            elif kind == 'overwrite':
                res = env.rollout(n, actions=actions, auto_reset=p.auto_reset, out=acc)
                assert res is acc and set(res) == {'returns', 'episodes', 'collisions'}
                want = run.totals(lo, hi)
            else:
                rec = env.rollout(n, actions=actions, auto_reset=p.auto_reset, record=True)
                assert 'RECORD' in env.last_kernel('rollout') or case.kernel == 'thread_per_env', env.last_kernel('rollout')
                for j, ref in enumerate(run.refs[lo:hi]):
                    assert np.array_equal(rec['local'][j], ref['local']), tag + (j,)
                    assert np.array_equal(bits(rec['reward'][j]), bits(ref['reward'])), tag + (j,)
                    assert np.array_equal(bits(rec['prob'][j]), bits(ref['prob'])), tag + (j,)
                    assert np.array_equal(rec['done'][j], ref['done']) and np.array_equal(rec['collision'][j], ref['collision']), tag + (j,)
                _check(rec, run.totals(lo, hi), env, run, k, tag)
                continue
            name = env.last_kernel('rollout')
            assert name.startswith(case.kernel_name(p)), (tag, name, case.kernel_name(p))
            seen.add(name)
            _check(acc, want, env, run, k, tag)
        env.close()
    for name in sorted(seen):
        print('totals kernel: %s' % name)
    assert len({name.split(' block=')[0] for name in seen}) == len({case.kernel_name(p) for p in tc.passes_of(case)}), sorted(seen)
