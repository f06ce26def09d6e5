"""GPU parity where the step index, the seed and the env id need all 64 bits (tests/wide_counter_cases.py: the windows, the seeds,
the case tables; tests/test_wide_counter_cases.py proves on the oracle's side that every 32-bit narrowing of them shows): every
fused rollout form, every single-step form, a recorded graph and fill_random_actions, stepped ACROSS t = 2^32, 2^33, 2^34 and 2^49
with seeds whose halves are all ones and env ids that carry into their high word inside the batch -- every recorded array of every
step against the C oracle, bit for bit."""
import numpy as np
import pytest

import philox
import wide_counter_cases as wc
from conftest import set_tune
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from parity_checks import bits, to_np

pytestmark = pytest.mark.gpu


def _exp(X):
    return '2^%d' % (X.bit_length() - 1)


def _env(case, X, tables):
    grid, nbr, start, goal, policy = tables
    env = VecMapfEnv(grid, case.A, None, None, wc.SLIP, *wc.REWARDS, OptimizationCriteria.Makespan, seed=case.seed(X), env_id_offset=wc.OFFSET,
                     start_local=start, goal_local=goal, kernel=case.kernel, device_arrays=case.device)
    if policy is not None:
        env.set_policy('table', table=policy[0], rows=policy[1])
    return env


def _check_step(got, ref, tag):
    """got: (local, reward, prob, done, collision) of one step"""
    local, reward, prob, done, collision = (to_np(x) for x in got)
    assert np.array_equal(local, ref['local']), tag
    assert np.array_equal(bits(reward), bits(ref['reward'])) and np.array_equal(bits(prob), bits(ref['prob'])), tag
    assert np.array_equal(done, ref['done']) and np.array_equal(collision, ref['collision']), tag


@pytest.mark.parametrize('case', wc.ROLLOUT_CASES, ids=lambda c: c.id)
def test_recorded_rollouts_across_every_crossing_point(case, monkeypatch):
    """Pass A (streamed actions, or the table policy): launches of 5 and 7 steps from X - 5, the second one's first step is X.
    Pass B (the in-kernel random policy): 12 steps from X - 6, X inside the unrolled part.  One handle per crossing point (its seed),
    repositioned with set_state between the passes."""
    set_tune(monkeypatch, **case.tune)
    tables = wc.tables_of(case)
    start = tables[2]
    for X in wc.CROSSINGS:
        env = _env(case, X, tables)
        for window in wc.rollout_windows(X, case.table):
            run = wc.window_run(case, X, window.name)
            env.set_state(np.ascontiguousarray(start), t=window.t0)
            lo = 0
            for n in window.lengths:
                acts = np.stack(run.acts[lo:lo + n]) if window.mode == 'streamed' else None
                res = env.rollout(n, actions=acts, auto_reset=True, record=True)
                seen = env.last_kernel('rollout')
                if window.mode == 'policy':
                    assert case.layout.split(',RECORD')[0] in seen and (',POLICY' in seen or case.kernel == 'thread_per_env'), seen
                    assert ('BITMAP' in seen) == ('BITMAP' in case.layout), seen
                else:
                    assert case.layout in seen and (',STREAM' in seen or case.table or case.kernel == 'thread_per_env'), seen
                for k in range(n):
                    _check_step((res['local'][k], res['reward'][k], res['prob'][k], res['done'][k], res['collision'][k]), run.refs[lo + k],
                                (case.id, _exp(X), window.name, 'step X%+d' % (window.t0 + lo + k - X)))
                total = run.totals(lo, lo + n)
                assert np.array_equal(bits(res['returns']), bits(total['returns'])), (case.id, _exp(X), window.name, lo)
                assert np.array_equal(res['episodes'], total['episodes']) and np.array_equal(res['collisions'], total['collisions'])
                lo += n
            local, t = env.get_state()
            assert np.array_equal(local, run.state) and t == run.t_end == window.t0 + window.n_steps, (case.id, _exp(X), window.name, t)
        env.close()


@pytest.mark.parametrize('case', wc.STEP_CASES, ids=lambda c: c.id)
def test_single_steps_across_every_crossing_point(case, monkeypatch):
    """Eight plain step() calls from X - 4 with auto-reset (the device's own uniforms): the fifth call is step X.  The first call
    follows set_state (an env may be terminal), the others an auto-reset step: the packed step's NO_TERMINAL instance."""
    set_tune(monkeypatch, **case.tune)
    tables = wc.tables_of(case)
    for X in wc.CROSSINGS:
        env = _env(case, X, tables)
        run = wc.window_run(case, X, 'S')
        env.set_state(np.ascontiguousarray(tables[2]), t=run.t0)
        for k, ref in enumerate(run.refs):
            local, reward, done, info = env.step(run.acts[k], auto_reset=True)
            seen = env.last_kernel('step')
            assert seen.startswith(wc.step_name(case, k)), (seen, wc.step_name(case, k))
            _check_step((local, reward, info['prob'], done, info['collision']), ref, (case.id, _exp(X), 'step X%+d' % (run.t0 + k - X)))
            assert not info['was_terminal'].any()
        local, t = env.get_state()
        assert np.array_equal(local, run.state) and t == run.t_end == X + 4, (case.id, _exp(X), t)
        env.close()


@pytest.mark.parametrize('case', wc.GRAPH_CASES, ids=lambda c: c.id)
def test_graph_replays_carry_the_device_side_step_index(case):
    """Eight recorded steps, t set to X - 12, three replays: the second runs X - 4 .. X + 3 -- the device-side base plus the recorded
    offset carries inside a replay.  Two plain steps follow: the host's index continues the device's."""
    import torch
    tables = wc.tables_of(case)
    for X in wc.GRAPH_CROSSINGS:
        env = _env(case, X, tables)
        run = wc.window_run(case, X, 'G')
        actions = [torch.as_tensor(a).cuda() for a in run.acts[:8]]       # (one allocation each: the library wants them 16-byte aligned)
        env.graph_begin()
        outs = []
        for k in range(8):
            call, out = env.prepare_step(actions[k], auto_reset=True)
            call()
            outs.append(out)
        assert case.layout in env.last_kernel('step'), env.last_kernel('step')
        graph = env.graph_end()
        assert graph.steps == 8 and env.t == 0
        env.set_state(None, t=run.t0)
        for rep in range(3):
            graph.launch(1)
            env.sync()
            for k in range(8):
                out, s = outs[k], 8 * rep + k
                assert np.array_equal(run.acts[s], run.acts[k])
                _check_step((out['local'], out['reward'], out['prob'], out['done'], out['collision']), run.refs[s],
                            (case.id, _exp(X), 'replay %d' % rep, 'step X%+d' % (run.t0 + s - X)))
            assert env.t == run.t0 + 8 * (rep + 1)
        for s in (24, 25):
            local, reward, done, info = env.step(actions[s % 8], auto_reset=True)
            env.sync()
            _check_step((local, reward, info['prob'], done, info['collision']), run.refs[s], (case.id, _exp(X), 'plain step X%+d' % (run.t0 + s - X)))
        local, t = env.get_state()
        env.sync()
        assert np.array_equal(to_np(local), run.state) and t == run.t_end == X + 14
        graph.close()
        env.close()


@pytest.mark.parametrize('X', wc.FILL_CROSSINGS, ids=_exp)
def test_fill_random_actions_across_the_policy_counters_carry(X):
    """fill_random_actions(X - 3, 9) at 8 agents and at 5 (a ragged quad) against philox.random_actions_np"""
    from gym_mapf_amd.envs.grid import MapfGrid
    grid = MapfGrid(['.....'] * 5)
    for k, (A, E) in enumerate(wc.FILL_SHAPES):
        seed = wc.seed_of(k, X)
        cells = np.zeros((E, A), np.uint16) + np.arange(A, dtype=np.uint16)
        env = VecMapfEnv(grid, A, None, None, 0.0, -1.0, 1.0, -1.0, OptimizationCriteria.Makespan, seed=seed, env_id_offset=wc.OFFSET,
                         start_local=cells, goal_local=cells[:, ::-1].copy())
        got = env.fill_random_actions(X - 3, 9)
        ids = wc.OFFSET + np.arange(E, dtype=np.uint64)
        for s in range(9):
            assert np.array_equal(got[s], philox.random_actions_np(seed, ids, X - 3 + s, A)), (_exp(X), A, 'step X%+d' % (s - 3))
        env.close()
