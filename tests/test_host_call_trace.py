"""The host-mode Python layer (VecMapfEnv, MultiMapVecEnv, UnionMapVecEnv) against a recorded call trace: which C entry
points a script of Python calls reaches, with which integers, flags and struct fields, which pointers are null, and -- where
a pointer lands in an array the caller can see -- at which byte offset.  No GPU and no library: ``_native.load`` is replaced
by an object whose every ``mapf_*`` attribute records its arguments and returns 0.

tests/golden/host_call_trace.json was recorded from the tree BEFORE the call arrays of each method were named once
(``python tests/test_host_call_trace.py --record`` rewrites it; do that only when the C calls are meant to change)."""
import json
import os
import sys

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gym-mapf_amd'))

from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import multi_map, vec_env
from gym_mapf_amd.envs.grid import MapfGrid
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv
from native_recorder import Recorder

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'host_call_trace.json')


def _run_script(monkeypatch_setattr):
    rec = Recorder()
    monkeypatch_setattr(nat, 'load', lambda: rec)
    SoC, Makespan = OptimizationCriteria.SoC, OptimizationCriteria.Makespan
    grid = MapfGrid(['....', '.@..', '....'])
    valid = grid.tables()[0]
    rs = np.random.RandomState(5)

    def step(name, fn, watch=None, returned=True):
        """one step of the script: run it, watch what it was given and what it returned, resolve the pointers"""
        rec.step = name
        if watch:
            for label, arrays in watch.items():
                rec.watch(label, arrays)
        res = fn()
        if returned and res is not None:
            if isinstance(res, tuple) and len(res) == 4 and isinstance(res[3], dict):      # (local, reward, done, info)
                rec.watch('ret', dict(local=res[0], reward=res[1], done=res[2], **res[3]))
            elif isinstance(res, tuple):
                rec.watch('ret', {str(i): r for i, r in enumerate(res)})
            else:
                rec.watch('ret', res)
        rec.resolve()
        return res

    # ---- construction
    E, A = 6, 2
    step('create: locations', lambda: VecMapfEnv(grid, A, ((0, 0), (2, 3)), ((2, 0), (0, 3)), 0.2, -1000.0, 100.0, -1.0, Makespan,
                                                 n_envs=3, seed=7, env_id_offset=11).close(), returned=False)
    starts = np.asarray([[valid[i] for i in rs.choice(len(valid), A, replace=False)] for _ in range(E)])
    goals = np.asarray([[valid[i] for i in rs.choice(len(valid), A, replace=False)] for _ in range(E)])
    step('create: [E, A, 2] arrays', lambda: VecMapfEnv(grid, A, starts, goals, 0.1, -0.3, 0.7, -0.1, SoC, seed=2 ** 40 + 3,
                                                        kernel='thread_per_env').close(), returned=False)
    step('create: start_local 1-D, goal_local 1-D', lambda: VecMapfEnv(grid, A, None, None, 0.2, -1.0, 1.0, -1.0, SoC, n_envs=4,
                                                                      start_local=[0, 5], goal_local=np.array([7, 2]), kernel='lane_group').close(),
         returned=False)
    sl = rs.randint(0, len(valid), (E, A))
    env = step('create: start_local 2-D, goal_local 1-D',
               lambda: VecMapfEnv(grid, A, None, None, 0.2, -1.0, 1.0, -1.0, SoC, start_local=sl, goal_local=[7, 2], seed=3), returned=False)

    # ---- step / prepare_step
    acts = rs.randint(0, 5, (E, A)).astype(np.uint8)
    uni = rs.rand(E, A)
    step('step', lambda: env.step(acts), {'actions': acts})
    step('step: nested lists, auto_reset', lambda: env.step(acts.tolist(), auto_reset=True))
    step('step: uniforms', lambda: env.step(acts, uniforms=uni, auto_reset=True), {'actions': acts, 'uniforms': uni})
    partial = {'reward': np.empty(E, np.float64), 'was_terminal': np.empty(E, np.uint8)}
    step('step: partial out', lambda: env.step(acts, out=partial), {'actions': acts, 'out': partial})
    for write_local in (True, False):
        name = 'prepare_step: write_local=%s' % write_local
        call, out = step(name, lambda: env.prepare_step(acts, uniforms=uni, auto_reset=True, out=partial, write_local=write_local),
                         {'actions': acts, 'uniforms': uni, 'out': partial}, returned=False)
        assert ('local' in out) == write_local
        for k in range(2):
            kept = step('%s: call %d' % (name, k), call, {'actions': acts, 'uniforms': uni, 'out': out}, returned=False)
            assert kept[0] is acts and kept[1] is uni and kept[2] is out

    # ---- rollout
    T = 4
    streamed = rs.randint(0, 5, (T, E, A)).astype(np.uint8)
    for record in (False, True):
        for a in (None, streamed):
            tag = 'rollout: record=%s, %s' % (record, 'no actions' if a is None else 'actions')
            first = step(tag, lambda: env.rollout(T, actions=a, record=record, auto_reset=False), {'actions': streamed})
            step(tag + ', accumulate_into', lambda: env.rollout(T, actions=a, record=record, accumulate_into=first), {'actions': streamed, 'into': first})
            step(tag + ', out', lambda: env.rollout(T, actions=a, record=record, out=first), {'actions': streamed, 'out': first})
            step(tag + ', out again', lambda: env.rollout(T, actions=a, record=record, out=first), {'actions': streamed, 'out': first})
            assert env._rollout_io is None                   # (the cached argument block is device-mode only)
    step('rollout: empty out dict', lambda: env.rollout(3, out={}))
    step('rollout: T = 0', lambda: env.rollout(0))
    long_actions = rs.randint(0, 5, (12, E, A)).astype(np.uint8)
    real_limit, VecMapfEnv._MAX_LAUNCH_STEPS = VecMapfEnv._MAX_LAUNCH_STEPS, 5
    try:
        step('rollout: 12 steps in slices of 5', lambda: env.rollout(12, actions=long_actions, record=True), {'actions': long_actions})
        tot = step('rollout: 12 steps in slices of 5, totals only', lambda: env.rollout(12))
        step('rollout: 12 steps in slices of 5, accumulate_into', lambda: env.rollout(12, accumulate_into=tot), {'into': tot})
    finally:
        VecMapfEnv._MAX_LAUNCH_STEPS = real_limit

    # ---- transitions
    N = 5
    q_local = rs.randint(0, len(valid), (N, A)).astype(np.uint16)
    q_next = rs.randint(0, len(valid), (N, A)).astype(np.uint16)
    q_acts = rs.randint(0, 5, (N, A)).astype(np.uint8)
    q_env = rs.randint(0, E, N).astype(np.uint32)
    watch = {'local': q_local, 'actions': q_acts, 'env_index': q_env, 'next_local': q_next}
    tr = step('transitions', lambda: env.transitions(q_local, q_acts), watch)
    step('transitions: window, env_index, out', lambda: env.transitions(q_local.tolist(), q_acts, max_branches=9, env_index=q_env, first_branch=2, out=tr),
         dict(watch, out=tr))
    step('transitions: max_branches=4', lambda: env.transitions(q_local, q_acts, max_branches=4), watch)
    tc = step('transitions_compact', lambda: env.transitions_compact(q_local, q_acts), watch)
    step('transitions_compact: capacity', lambda: env.transitions_compact(q_local, q_acts, env_index=q_env, first_branch=1, max_branches=5, capacity=17), watch)
    step('transitions_compact: out', lambda: env.transitions_compact(q_local, q_acts.tolist(), max_branches=100, out=tc), dict(watch, out=tc))
    step('transitions_compact: max_branches=0', lambda: env.transitions_compact(q_local, q_acts, max_branches=0), watch)
    for want_done in (True, False):
        for want_collision in (True, False):
            step('transition_rewards: want_done=%s, want_collision=%s' % (want_done, want_collision),
                 lambda: env.transition_rewards(q_local, q_acts, q_next, env_index=q_env if want_done else None, want_done=want_done,
                                                want_collision=want_collision), watch)

    # ---- the rest of the API
    step('fill_random_actions', lambda: env.fill_random_actions(3, 4))
    fill = np.empty((2, E, A), np.uint8)
    step('fill_random_actions: out', lambda: env.fill_random_actions(9, 2, out=fill), {'out': fill})
    step('set_policy: greedy', lambda: env.set_policy('greedy'))
    table = rs.randint(0, 5, (3, len(valid)))
    step('set_policy: table, rows [E, A]', lambda: env.set_policy('table', table=table, rows=rs.randint(0, 3, (E, A))))
    step('set_policy: table, rows [A]', lambda: env.set_policy('table', table=table.tolist(), rows=[2, 0]))
    step('set_policy: random', lambda: env.set_policy('random'))
    step('get_state', lambda: env.get_state())
    state = np.empty((E, A), np.uint16)
    step('get_state: out', lambda: env.get_state(out=state), {'out': state})
    step('set_state', lambda: env.set_state(q_local[:1].repeat(E, 0), t=5))
    step('set_state: t only', lambda: env.set_state(t=9))
    step('set_state: cells only', lambda: env.set_state(np.zeros((E, A), np.int64)))
    step('reset', lambda: env.reset())
    mask = np.array([1, 0, 0, 1, 1, 0], np.uint8)
    step('reset: mask', lambda: env.reset(mask), {'mask': mask})
    step('reset: mask as list', lambda: env.reset([0, 1, 0, 0, 0, 1]))
    step('query_terminal', lambda: env.query_terminal())
    term = np.empty(E, np.uint8)
    step('query_terminal: out', lambda: env.query_terminal(out=term), {'out': term})
    assert step('t', lambda: env.t, returned=False) == 0
    assert step('last_kernel', lambda: [env.last_kernel(w) for w in ('step', 'rollout', 'transitions')], returned=False) == ['', '', '']
    step('stream, sync, timer', lambda: (env.stream, env.sync(), env.timer_begin(), env.timer_end()), returned=False)
    step('close', env.close, returned=False)

    # ---- MultiMapVecEnv: four envs over two maps in three runs
    maps = [MapfGrid(['....', '.@..', '....']), MapfGrid(['...', '...', '...'])]
    pick = [0, 1, 1, 0]
    A = 3
    starts = [[maps[k].tables()[0][i] for i in rs.choice(9, A, replace=False)] for k in pick]
    goals = [[maps[k].tables()[0][i] for i in rs.choice(9, A, replace=False)] for k in pick]
    kw = dict(seed=8, env_id_offset=1000)
    multi = step('multi: create', lambda: multi_map.MultiMapVecEnv([maps[k] for k in pick], A, starts, goals, 0.3, -10.0, 5.0, -1.0, SoC, **kw),
                 returned=False)
    assert multi.n_handles == 3 and len(multi.grids) == 2
    m_acts = rs.randint(0, 5, (4, A)).astype(np.uint8)
    m_uni = rs.rand(4, A)
    m_streamed = rs.randint(0, 5, (3, 4, A)).astype(np.uint8)
    step('multi: step', lambda: multi.step(m_acts, auto_reset=True), {'actions': m_acts})
    step('multi: step, uniforms', lambda: multi.step(m_acts.tolist(), uniforms=m_uni), {'uniforms': m_uni})
    step('multi: rollout', lambda: multi.rollout(6, auto_reset=False))
    step('multi: rollout, streamed actions', lambda: multi.rollout(3, actions=m_streamed), {'actions': m_streamed})
    step('multi: reset', lambda: multi.reset())
    step('multi: reset(mask)', lambda: multi.reset(np.array([0, 1, 1, 0], np.uint8)))
    step('multi: get_state', lambda: multi.get_state())
    step('multi: sync, close', lambda: (multi.sync(), multi.close()), returned=False)

    # ---- UnionMapVecEnv
    union = step('union: create', lambda: multi_map.UnionMapVecEnv([maps[k] for k in pick], A, starts, goals, 0.3, -10.0, 5.0, -1.0, SoC, **kw),
                 returned=False)
    step('union: step', lambda: union.step(m_acts, uniforms=m_uni, auto_reset=True), {'actions': m_acts, 'uniforms': m_uni})
    step('union: rollout(record=True)', lambda: union.rollout(3, actions=m_streamed, record=True), {'actions': m_streamed})
    step('union: rollout', lambda: union.rollout(2))
    step('union: set_policy, get_state, query_terminal, last_kernel',
         lambda: (union.set_policy('greedy'), union.get_state(), union.query_terminal(), union.last_kernel()), returned=False)
    step('union: set_state', lambda: union.set_state(np.zeros((4, A), np.uint16), t=3))
    step('union: reset(mask), close', lambda: (union.reset(np.array([1, 1, 0, 0], np.uint8)), union.sync(), union.close()), returned=False)
    return json.loads(json.dumps(rec.trace))                     # (tuples -> lists, as the fixture holds them)


def test_host_mode_python_layer_makes_the_recorded_calls(monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = _run_script(monkeypatch.setattr)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, 'call %d (%s -> %s)' % (k, w['step'], w['fn'])
    assert len(got) == len(want)
    # the script covers what the fixture is meant to pin
    assert {e['fn'] for e in want} >= {'mapf_create', 'mapf_step', 'mapf_rollout', 'mapf_transitions_window', 'mapf_transitions_compact',
                                       'mapf_transition_rewards', 'mapf_fill_random_actions', 'mapf_set_policy', 'mapf_set_policy_table',
                                       'mapf_get_state', 'mapf_set_state', 'mapf_reset', 'mapf_query_terminal', 'mapf_last_kernel', 'mapf_destroy'}
    sliced = [e['args'][1] for e in want if e['step'] == 'rollout: 12 steps in slices of 5']
    assert [(io['n_steps'], io['accumulate'], io['actions']) for io in sliced] == \
        [(5, 0, ['actions', 0]), (5, 1, ['actions', 5 * 6 * 2]), (2, 1, ['actions', 10 * 6 * 2])]


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], 'usage: python tests/test_host_call_trace.py --record'
    trace = _run_script(setattr)
    with open(FIXTURE, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(e, sort_keys=True) for e in trace) + '\n]\n')
    print('recorded %d calls into %s' % (len(trace), FIXTURE))
