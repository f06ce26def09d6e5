"""The packed single step in every instance the launcher holds and the resident forms' chunk walk, on the GPU, against the C oracle
bit for bit.  tests/step_cases.py has the case table and the oracle's side; tests/test_step_cases.py (no GPU) holds the table against
the planner -- every case plans its instance, the names below are the planned ones, the chunk-walk cases walk 7, 4 + 3 and 3 + 2 + 2
chunks per block -- and shows that the inputs contain slip ties, terminal envs, goal and collision ends."""
import numpy as np
import pytest

import step_cases as sc
from conftest import load_json, set_tune
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from parity_checks import bits

pytestmark = pytest.mark.gpu
NAMES = load_json('lq_step_kernel_names.json')['launches']


def _name(case, scen, may_be_terminal):
    """the full name of that step: the recorded one, which tests/test_step_cases.py proves to be the planned one"""
    return NAMES[case.key]['names']['%s %s' % ('SCEN' if scen else 'ROWS', 'TERMINAL' if may_be_terminal else 'NO_TERMINAL')]


def _tune(monkeypatch, case, scen, grid=True):
    items = case.tune_items(scen)
    if not grid:
        items.pop('step_grid', None)
    set_tune(monkeypatch, scen_table=None, step_grid=None)
    set_tune(monkeypatch, **items)


def _env(case, p, run, **kw):
    return VecMapfEnv(sc.the_map()[0], case.A, None, None, p.fail_prob, *p.rewards, OptimizationCriteria[p.criteria], seed=run.seed,
                      env_id_offset=sc.OFFSET, start_local=run.start, goal_local=run.goal, **kw)


def _same(got, ref, tag):
    local, reward, done, info = got
    assert np.array_equal(np.asarray(local), ref['local']), tag
    assert np.array_equal(np.asarray(done), ref['done']) and np.array_equal(np.asarray(info['collision']), ref['collision']), tag
    assert np.array_equal(np.asarray(info['was_terminal']), ref['was_terminal']), tag
    assert np.array_equal(bits(reward), bits(ref['reward'])) and np.array_equal(bits(info['prob']), bits(ref['prob'])), tag


def _run_handle(case, scen, p):
    """the twelve steps of one handle: every output of every step, the state and the step index after it, the kernel's name"""
    run = case.run(p)
    env = _env(case, p, run)
    try:
        for s, (auto_reset, may_be_terminal, set_before) in enumerate(sc.step_plan()):
            tag = (case.id, 'SCEN' if scen else 'ROWS', p.name, s)
            if set_before:
                env.set_state(run.set_states[s])
            got = env.step(run.acts[s], auto_reset=auto_reset)
            assert env.last_kernel('step') == _name(case, scen, may_be_terminal), (tag, env.last_kernel('step'))
            _same(got, run.refs[s], tag)
            state, t = env.get_state()
            assert np.array_equal(state, run.after[s][0]) and t == run.after[s][1] == env.t, tag
    finally:
        env.close()


@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.id)
def test_every_handle_of_the_case_against_the_oracle(monkeypatch, case):
    """{scenario table, scen_table=0} x {Makespan with the exact constants, SoC with the inexact ones}: four of the 84 kernels per
    instance case; a chunk-walk case runs them with its blocks walking WALK_PATTERNS[step_grid] chunks each"""
    for scen, p in case.handles:
        _tune(monkeypatch, case, scen)
        _run_handle(case, scen, p)


def test_graph_replay_in_a_chunk_walk_case(monkeypatch):
    """FullRows K = 8, Q = 1 under step_grid=2 in device mode: six recorded steps replayed twice, then two plain steps.  A block's
    later chunks re-read the argument block and load the device-side step index again: 14 steps against the oracle."""
    import torch
    case, run = sc.GRAPH_CASE, sc.GraphRun()
    _tune(monkeypatch, case, True)
    env = _env(case, run.p, run, device_arrays=True)
    try:
        actions = [torch.as_tensor(a, device='cuda') for a in run.node_acts]
        env.graph_begin()
        outs = []
        for k in range(sc.GRAPH_NODES):
            call, out = env.prepare_step(actions[k], auto_reset=True)
            call()
            outs.append(out)
            assert env.last_kernel('step') == _name(case, True, k == 0), (k, env.last_kernel('step'))   # (the first recorded step tests is_terminal)
        graph = env.graph_end()
        assert graph.steps == sc.GRAPH_NODES and env.t == 0
        s = 0
        for rep in range(sc.GRAPH_REPLAYS):
            graph.launch(1)
            env.sync()
            for k in range(sc.GRAPH_NODES):
                out = {name: arr.cpu().numpy() for name, arr in outs[k].items()}
                _same((out['local'], out['reward'], out['done'], out), run.refs[s], ('replay', rep, k))
                s += 1
            state, t = env.get_state()
            assert np.array_equal(state.cpu().numpy(), run.after[s - 1][0]) and t == run.after[s - 1][1] == env.t, rep
        for k in range(sc.GRAPH_PLAIN):
            local, reward, done, info = env.step(actions[k], auto_reset=True)
            env.sync()
            assert env.last_kernel('step') == _name(case, True, False), env.last_kernel('step')
            _same((local.cpu().numpy(), reward.cpu().numpy(), done.cpu().numpy(), {name: arr.cpu().numpy() for name, arr in info.items()}),
                  run.refs[s], ('plain', k))
            state, t = env.get_state()
            assert np.array_equal(state.cpu().numpy(), run.after[s][0]) and t == run.after[s][1], k
            s += 1
        assert s == len(run.refs) == 14
        graph.close()
    finally:
        env.close()


def test_default_dispatch_is_unchanged_by_the_key(monkeypatch):
    """without step_grid the chunk-walk batch runs as it always did (seven blocks of one chunk: the same names, the same results); under
    step_grid alone a small batch still takes the plain step, which ignores the key"""
    case = sc.WALK_CASES[0]
    assert case.key == 'FullRows-K8-Q1'
    _tune(monkeypatch, case, True, grid=False)
    _run_handle(case, True, sc.PASSES[0])
    plain = sc.INSTANCE_CASES[1]
    assert plain.key == 'Plain-K4-Q2'
    set_tune(monkeypatch, step_big=None, scen_table=None, step_grid='2')
    _run_handle(plain, True, sc.PASSES[1])
