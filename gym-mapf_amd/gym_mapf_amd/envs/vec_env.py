"""VecMapfEnv -- E concurrent MAPF environments stepped by one HIP kernel launch.

This is the batched form of the reference's ``MapfEnv`` (gym_mapf/envs/mapf_env.py:115-266):
same constructor arguments, same transition semantics per env, but state, actions and
results are env-major arrays (``x[e, i]`` = agent i of env e) and the work happens in
``libmapf_hip.so``.  Two memory modes:

* host mode (default): numpy arrays in, numpy arrays out, each call synchronises;
* device mode (``device_arrays=True``): torch CUDA tensors in/out, calls only enqueue on the
  env's HIP stream -- call ``sync()`` before reading results on another stream.

There is no CPU implementation behind this class: without the library or a GPU the
constructor raises ``MapfNativeError``.
"""
import collections
import ctypes
import enum

import numpy as np

from gym_mapf_amd import _native as nat


class OptimizationCriteria(enum.Enum):
    """Reference mapf_env.py:31-33."""
    SoC = 'SoC'
    Makespan = 'Makespan'


_CRITERIA_CODE = {OptimizationCriteria.Makespan: nat.MAPF_MAKESPAN, OptimizationCriteria.SoC: nat.MAPF_SOC}


# One step's outputs, in the argument order of mapf_step: (name, dtype, one value per agent -- else one per env).  The first
# five are also what a recording rollout keeps per step (mapf_rollout_io's rec_<name>); ROLLOUT_TOTALS are its out_<name>.
STEP_OUTPUTS = (('local', np.uint16, True), ('reward', np.float64, False), ('done', np.uint8, False),
                ('collision', np.uint8, False), ('prob', np.float64, False), ('was_terminal', np.uint8, False))
ROLLOUT_TOTALS = (('returns', np.float64), ('episodes', np.uint32), ('collisions', np.uint32))
# ... and what an env with an episode limit (set_episode_limit) reports on top: mapf_step_limited's out_truncated, a recording
# rollout's rec_truncated, the rollout's out_truncations
STEP_TRUNCATED = ('truncated', np.uint8, False)
ROLLOUT_TRUNCATIONS = ('truncations', np.uint32)
# ... and an env with an episode budget (set_episode_budget): the rollout's out_live_steps
ROLLOUT_LIVE_STEPS = ('live_steps', np.uint32)
_TORCH_DTYPE = {np.uint8: 'uint8', np.uint16: 'uint16', np.uint32: 'uint32', np.uint64: 'uint64', np.float64: 'float64'}
# rollout(out=...): the argument block of the last such call, with what it was made from
_RolloutIO = collections.namedtuple('_RolloutIO', 'out call arrays actions io call_args')


def checked_ptr(torch, arr, dtype, shape, name):
    """Raw pointer of a caller-supplied array after checking dtype/shape/contiguity: a CUDA tensor of the ``torch`` module
    (device mode), a numpy array when ``torch`` is None (host mode)."""
    if torch is not None:
        want = getattr(torch, _TORCH_DTYPE[dtype])
        if not (isinstance(arr, torch.Tensor) and arr.is_cuda and arr.dtype == want and arr.is_contiguous()
                and tuple(arr.shape) == tuple(shape)):
            raise ValueError('%s must be a contiguous CUDA %s tensor of shape %r' % (name, want, tuple(shape)))
        return arr.data_ptr()
    if not (isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.flags.c_contiguous
            and tuple(arr.shape) == tuple(shape)):
        raise ValueError('%s must be a C-contiguous %s array of shape %r' % (name, np.dtype(dtype), tuple(shape)))
    return arr.ctypes.data


def array_ptr(torch, arr, dtype, shape, name):
    """``checked_ptr`` of an optional array: None stays None (the C ABI's NULL)."""
    return None if arr is None else checked_ptr(torch, arr, dtype, shape, name)


def coerce_array(torch, arr, dtype, shape, name):
    """Inputs: accept anything array-like in host mode (``torch`` None), strict tensors in device mode."""
    if arr is None or torch is not None:
        return arr
    out = np.ascontiguousarray(arr, dtype=dtype)
    if tuple(out.shape) != tuple(shape):
        raise ValueError('%s must have shape %r, got %r' % (name, tuple(shape), tuple(out.shape)))
    return out


def _locs_to_local(loc_to_int, locs):
    """(row, col) sequence -> local ids; KeyError for obstacles / out-of-map cells (reference :143, :369)."""
    return [loc_to_int[(int(l[0]), int(l[1]))] for l in locs]


class _DeviceView:
    """``__cuda_array_interface__`` carrier: lets torch wrap a device pointer the library owns without copying."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}
        self._owner = owner   # the view must not outlive the env


class StepGraph:
    """A recorded sequence of ``step`` / ``rollout`` calls (``VecMapfEnv.graph_begin`` .. ``graph_end``): ``launch(n)``
    replays it n times.  The step index lives in device memory for recorded launches, so every replay draws fresh
    random numbers -- n replays of an N-step recording equal n * N ``step`` calls with the same arrays."""

    def __init__(self, env, handle, steps):
        self._env, self._g, self.steps = env, handle, steps

    def launch(self, n_replays=1):
        rc = self._env._lib.mapf_graph_launch(self._env._h, self._g, int(n_replays))
        if rc:
            nat.check(rc)

    def close(self):
        g, self._g = self._g, None
        if g and self._env._h:
            nat.check(self._env._lib.mapf_graph_destroy(self._env._h, g))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VecMapfEnv:
    def __init__(self, grid, n_agents, start_locations, goal_locations, fail_prob,
                 reward_of_collision, reward_of_goal, reward_of_living, optimization_criteria,
                 *, n_envs=None, seed=42, env_id_offset=0, device=0, device_arrays=False, stream=None,
                 start_local=None, goal_local=None, kernel='auto'):
        self.grid = grid
        self.n_agents = int(n_agents)
        self.fail_prob = fail_prob
        self.reward_of_clash = reward_of_collision
        self.reward_of_goal = reward_of_goal
        self.reward_of_living = reward_of_living
        self.optimization_criteria = optimization_criteria
        self.seed = int(seed)
        self.env_id_offset = int(env_id_offset)
        self.device = int(device)
        self.device_arrays = bool(device_arrays)
        self.valid_locations, self.loc_to_int, self._nbr = grid.tables()
        self.n_cells = len(self.valid_locations)

        start, start_bcast = self._as_local(start_locations, start_local, 'start')
        goal, goal_bcast = self._as_local(goal_locations, goal_local, 'goal')
        if n_envs is None:
            n_envs = 1
            for arr, bc in ((start, start_bcast), (goal, goal_bcast)):
                if not bc:
                    n_envs = arr.shape[0]
        self.n_envs = int(n_envs)
        for arr, bc, what in ((start, start_bcast, 'start'), (goal, goal_bcast, 'goal')):
            if not bc and arr.shape[0] != self.n_envs:
                raise ValueError('%s_locations has %d envs, expected %d' % (what, arr.shape[0], self.n_envs))
        self.start_local, self.goal_local = start, goal
        self._start_bcast, self._goal_bcast = start_bcast, goal_bcast

        flags = 0
        flags |= nat.MAPF_FLAG_START_BROADCAST if start_bcast else 0
        flags |= nat.MAPF_FLAG_GOAL_BROADCAST if goal_bcast else 0
        flags |= nat.MAPF_FLAG_DEVICE_PTRS if self.device_arrays else 0
        # kernel family: both give identical results; 'auto' lets the library choose
        flags |= {'auto': 0, 'thread_per_env': nat.MAPF_FLAG_THREAD_PER_ENV,
                  'lane_group': nat.MAPF_FLAG_LANE_GROUP}[kernel]
        self.kernel = kernel
        nbr = np.ascontiguousarray(self._nbr, dtype=np.uint16)
        desc = nat.MapfDesc(
            struct_size=ctypes.sizeof(nat.MapfDesc), n_cells=self.n_cells, n_agents=self.n_agents,
            criteria=_CRITERIA_CODE[optimization_criteria], n_envs=self.n_envs,
            env_id_offset=self.env_id_offset, seed=self.seed & 0xFFFFFFFFFFFFFFFF,
            nbr=nbr.ctypes.data, start=start.ctypes.data, goal=goal.ctypes.data,
            fail_prob=float(fail_prob), r_clash=float(reward_of_collision), r_goal=float(reward_of_goal),
            r_living=float(reward_of_living), device=self.device, flags=flags,
            stream=(int(stream) if stream else None))
        self._torch = None
        if self.device_arrays:
            # torch wheels bundle their own HIP runtime: it must be initialised BEFORE libmapf_hip pulls in the
            # system one, otherwise torch later reports "No HIP GPUs are available".
            import torch
            torch.cuda.init()
            self._torch = torch
            self._tdev = torch.device('cuda', self.device)
        self._lib = nat.load()
        handle = ctypes.c_void_p()
        nat.check(self._lib.mapf_create(ctypes.byref(desc), ctypes.byref(handle)))
        self._h = handle
        self.policy = 'random'         # on-device policy of rollout(actions=None): see set_policy
        self._rollout_io = None        # rollout(out=...): the _RolloutIO of the last such call
        self.episode_limit = 0         # set_episode_limit: steps per episode, 0 = no limit
        self.episode_budget = 0        # set_episode_budget: episodes per env, 0 = no budget
        self.conflict_slots = 0        # set_conflict_pairs: slots of the conflict matrix, 0 = the mode is off
        self.episode_log_capacity = 0  # set_episode_log: records per env, 0 = the mode is off

    # ------------------------------------------------------------------ construction
    def _as_local(self, locations, local_ids, what):
        """``locations``: A (row, col) pairs shared by every env, or an [E, A, 2] array of
        per-env locations.  ``local_ids`` (keyword form): integer [A] or [E, A] local ids."""
        A = self.n_agents
        if local_ids is not None:
            ids = np.asarray(local_ids)
            broadcast = ids.ndim == 1
            if broadcast:
                ids = ids.reshape(1, -1)
            if ids.ndim != 2 or ids.shape[1] != A or not np.issubdtype(ids.dtype, np.integer):
                raise ValueError('%s_local must be an integer array of shape [A] or [E, A]' % what)
            if ids.size and (ids.min() < 0 or ids.max() >= self.n_cells):
                raise KeyError('%s_local: local id out of range' % what)
            return np.ascontiguousarray(ids, dtype=np.uint16), broadcast
        if len(locations) != A and not (np.asarray(locations).ndim == 3):
            raise AssertionError('%r locations number is different than the number of agents %d' % (locations, A))
        arr = np.asarray(locations)
        if arr.ndim == 2 and arr.shape == (A, 2):
            return np.asarray(_locs_to_local(self.loc_to_int, arr), dtype=np.uint16).reshape(1, A), True
        if arr.ndim == 3 and arr.shape[1:] == (A, 2):
            flat = _locs_to_local(self.loc_to_int, arr.reshape(-1, 2))
            return np.ascontiguousarray(np.asarray(flat, dtype=np.uint16).reshape(arr.shape[0], A)), False
        raise ValueError('cannot interpret %s_locations of shape %r' % (what, arr.shape))

    # --------------------------------------------------------------------- plumbing
    def _ptr(self, arr, dtype, shape, name):
        return array_ptr(self._torch, arr, dtype, shape, name)

    def _empty(self, shape, dtype):
        if self.device_arrays:
            return self._torch.empty(shape, dtype=getattr(self._torch, _TORCH_DTYPE[dtype]), device=self._tdev)
        return np.empty(shape, dtype=dtype)

    def _coerce(self, arr, dtype, shape, name):
        return coerce_array(self._torch, arr, dtype, shape, name)

    def _inputs(self, *spec):
        """The input arrays of a call, each named once as (name, dtype, shape, array): the arrays as the library reads them (the
        caller keeps them alive across the call) and their pointers."""
        arrays = [self._coerce(arr, dt, shape, name) for name, dt, shape, arr in spec]
        return arrays, [self._ptr(arr, dt, shape, name) for arr, (name, dt, shape, _) in zip(arrays, spec)]

    def _outputs(self, spec, given=None, skip=(), fill=False):
        """The output arrays of a call, each named once as (name, dtype, shape): the dict ``given`` (with ``fill``, completed by new
        arrays), or a dict of new arrays -- and their pointers in the spec's order, None for the names in ``skip``."""
        res, ptrs = ({} if given is None else given), []
        for name, dt, shape in spec:
            if name in skip:
                ptrs.append(None)
                continue
            if name not in res and (fill or given is None):
                res[name] = self._empty(shape, dt)
            ptrs.append(self._ptr(res[name], dt, shape, name))
        return res, ptrs

    # -------------------------------------------------------------------------- API
    def reset(self, mask=None):
        """``MapfEnv.reset()`` for all envs, or those with a non-zero mask byte.  No reseed."""
        mask = self._coerce(mask, np.uint8, (self.n_envs,), 'mask')
        nat.check(self._lib.mapf_reset(self._h, self._ptr(mask, np.uint8, (self.n_envs,), 'mask')))

    def step(self, actions, uniforms=None, auto_reset=False, out=None):
        """One ``MapfEnv.step()`` per env.

        actions: uint8 [E, A] (0 STAY, 1 UP, 2 RIGHT, 3 DOWN, 4 LEFT).  uniforms: float64 [E, A]
        values the reference would draw from ``np_random.rand()`` in agent order, or None for the
        device Philox stream.  Returns ``(local, reward, done, info)`` with ``local`` uint16
        [E, A], ``reward`` float64 [E], ``done`` uint8 [E] and ``info`` holding ``prob``,
        ``collision`` and ``was_terminal`` arrays.  ``out`` may carry preallocated arrays under
        those names (plus ``local``, ``reward``, ``done``).  With an episode limit (``set_episode_limit``) ``info`` also
        holds ``truncated`` uint8 [E].
        """
        args, (_, _, out) = self._step_args(actions, uniforms, auto_reset, out)
        nat.check(self._step_fn()(*args))
        info = {'prob': out['prob'], 'collision': out['collision'], 'was_terminal': out['was_terminal']}
        if self.episode_limit:
            info['truncated'] = out['truncated']
        return out['local'], out['reward'], out['done'], info

    def _step_fn(self):
        """``mapf_step``, or ``mapf_step_limited`` (one more output, ``truncated``) for an env with an episode limit."""
        return self._lib.mapf_step_limited if self.episode_limit else self._lib.mapf_step

    def _step_args(self, actions, uniforms, auto_reset, out, write_local=True):
        """The argument tuple of one ``mapf_step`` and what it points into: (actions, uniforms, out), ``out`` completed."""
        E, A = self.n_envs, self.n_agents
        keep, inputs = self._inputs(('actions', np.uint8, (E, A), actions), ('uniforms', np.float64, (E, A), uniforms))
        spec = STEP_OUTPUTS + ((STEP_TRUNCATED,) if self.episode_limit else ())
        out, outputs = self._outputs([(name, dt, (E, A) if per_agent else (E,)) for name, dt, per_agent in spec],
                                     dict(out) if out else {}, skip=() if write_local else ('local',), fill=True)
        return (self._h, *inputs, *outputs, nat.MAPF_STEP_AUTO_RESET if auto_reset else 0), (*keep, out)

    def prepare_step(self, actions, uniforms=None, auto_reset=False, out=None, write_local=True):
        """Validate once, call many times: returns ``(call, out)`` where ``call()`` performs
        ``mapf_step`` on exactly these arrays (the per-call Python cost is one ctypes call).  Meant
        for device mode, where a training loop refills ``actions`` in place every iteration.
        ``write_local=False`` leaves ``out_local`` out of the call: the next observation is then read from
        ``state_view()`` (the handle's own state buffer, after auto-reset) and the step writes the cells once."""
        args, keep = self._step_args(actions, uniforms, auto_reset, out, write_local)
        fn, check, out = self._step_fn(), nat.check, keep[2]

        def call():
            rc = fn(*args)
            if rc:
                check(rc)
            return keep

        return call, out

    def state_view(self):
        """The handle's own state buffer as a uint16 [E, A] CUDA tensor (device mode only; no copy): ``env.s`` of every
        env as per-agent cells -- after an auto-reset step the state the NEXT step starts from (a finished episode
        shows its start cells).  Its contents change with every step / rollout / reset enqueued on the env's stream.
        READ-ONLY by contract (the C API returns a const pointer; torch cannot import a read-only CUDA array, so the
        tensor itself is writable): change the state through ``set_state``, or call ``invalidate_state()`` after writing
        the tensor -- the library otherwise assumes that no env is terminal after an auto-reset step and skips
        ``is_terminal(prev)`` (reference mapf_env.py:238-240) in the next one."""
        if not self.device_arrays:
            raise ValueError('state_view() needs device_arrays=True (use get_state() in host mode)')
        ptr = ctypes.c_void_p()
        nat.check(self._lib.mapf_state_view(self._h, ctypes.byref(ptr)))
        return self._torch.as_tensor(_DeviceView(ptr.value, (self.n_envs, self.n_agents), '<u2', self), device=self._tdev)

    def invalidate_state(self):
        """Tell the library that the state buffer was written behind its back (see ``state_view``)."""
        nat.check(self._lib.mapf_invalidate_state(self._h))

    def graph_begin(self):
        """Start recording ``step`` / ``prepare_step`` calls / ``rollout`` / ``reset`` into a hipGraph (device mode only)."""
        nat.check(self._lib.mapf_graph_begin(self._h))

    def graph_end(self):
        """Finish the recording: returns a ``StepGraph``."""
        g = ctypes.c_void_p()
        nat.check(self._lib.mapf_graph_end(self._h, ctypes.byref(g)))
        steps = ctypes.c_uint64(0)
        nat.check(self._lib.mapf_graph_steps(g, ctypes.byref(steps)))
        return StepGraph(self, g, steps.value)

    # one launch addresses every array with 32-bit byte offsets and counts per-launch events in 16 bits (include/mapf_hip.h)
    _MAX_ARRAY_BYTES = (1 << 32) - 1
    _MAX_LAUNCH_STEPS = 65535

    def rollout(self, n_steps, actions=None, auto_reset=True, record=False, accumulate_into=None, out=None):
        """``n_steps`` fused steps.  ``actions`` uint8 [T, E, A] or None for the on-device policy.  Returns a dict with
        ``returns`` f64 [E], ``episodes`` u32 [E], ``collisions`` u32 [E] and, when ``record``, the per-step
        ``local``/``reward``/``done``/``collision``/``prob`` trajectories (step-major).  One launch when every array
        of the call stays below 4 GiB and T <= 65535 (the C ABI's limits); otherwise the steps are issued as a few
        launches over consecutive slices of the same arrays (totals accumulate, the trajectory is identical).
        ``out``: the dict an earlier call of the same shape returned -- its arrays are written again instead of allocating
        eight new ones per call (totals overwritten, unlike ``accumulate_into``); a training loop that calls
        ``rollout(T=16..64)`` thousands of times wants this (profiles/r05_rollout_T_sweep.txt).
        With an episode limit (``set_episode_limit``) the dict also has ``truncations`` u32 [E] and, when ``record``,
        ``truncated`` u8 [T, E]; ``out`` and ``accumulate_into`` cover them.  With an episode budget (``set_episode_budget``) it
        has ``live_steps`` u32 [E] as well (covered likewise), and ``auto_reset=False`` raises ``ValueError``."""
        E, A, T = self.n_envs, self.n_agents, int(n_steps)
        if out is not None and accumulate_into is None:
            # the repeat call of a training loop: the same dict of arrays, the same shape.  The argument block of the earlier call
            # is reused once every array of the dict is still the OBJECT it was made from (an array swapped in the dict, another T
            # or another actions buffer take the full path below) -- slicing, checking and packing nine arrays is ~6 us of host
            # time per call, which is what a T <= 16 launch is bound by (profiles/r05_rollout_T_sweep.txt, column b)
            cached = self._rollout_io
            if cached is not None and cached.out is out and cached.call == (T, bool(auto_reset), bool(record)):
                act_ref = cached.actions
                same = all(out.get(k) is v for k, v in cached.arrays)
                if actions is None:
                    same = same and act_ref is None
                elif act_ref is not None and self.device_arrays:
                    same = same and isinstance(actions, self._torch.Tensor) and actions.data_ptr() == act_ref[0] and \
                        tuple(actions.shape) == act_ref[1] and actions.dtype == self._torch.uint8 and actions.is_contiguous() and actions.is_cuda
                else:
                    same = False
                if same:
                    nat.check(cached.call_args[0](*cached.call_args[1:]))
                    return out
        actions = self._coerce(actions, np.uint8, (T, E, A), 'actions')
        if out is not None and accumulate_into is not None:
            raise ValueError('pass either out= (overwrite) or accumulate_into= (add), not both')
        res = accumulate_into if accumulate_into is not None else (out if out is not None else {})
        limited, budgeted = bool(self.episode_limit), bool(self.episode_budget)
        if budgeted and not auto_reset:
            raise ValueError('an env with an episode budget rolls out with auto_reset=True only (set_episode_budget(None) switches it off)')
        trajectory = (STEP_OUTPUTS[:5] + ((STEP_TRUNCATED,) if limited else ())) if record else ()
        total_spec = ROLLOUT_TOTALS + ((ROLLOUT_TRUNCATIONS,) if limited else ()) + ((ROLLOUT_LIVE_STEPS,) if budgeted else ())
        for name, on in (('truncations', limited), ('live_steps', budgeted)):
            if on and accumulate_into is not None and name not in res:   # (totals of a call without the limit / budget: count from 0)
                res[name] = self._torch.zeros((E,), dtype=self._torch.uint32, device=self._tdev) if self.device_arrays else np.zeros((E,), np.uint32)
        res, totals = self._outputs([(name, dt, (E,)) for name, dt in total_spec], res, fill=True)
        for name, dt, per_agent in trajectory:
            shape = (T, E, A) if per_agent else (T, E)
            if out is None or name not in res or tuple(res[name].shape) != shape:
                res[name] = self._empty(shape, dt)
        per_step = max(E * A * 2, E * 8) if (record or actions is not None) else 0    # bytes of the widest per-step row
        t_max = min(self._MAX_LAUNCH_STEPS, self._MAX_ARRAY_BYTES // per_step if per_step else self._MAX_LAUNCH_STEPS)
        if T > 0 and t_max < 1:
            raise ValueError('one env-step of this batch exceeds 4 GiB: use fewer envs per handle')
        first, accumulate = 0, accumulate_into is not None
        while True:
            n = min(T - first, t_max) if T else 0
            sl = slice(first, first + n)
            fields = {'actions': self._ptr(actions[sl] if actions is not None else None, np.uint8, (n, E, A), 'actions')}
            fields.update(zip(('out_' + name for name, _ in total_spec), totals))
            for name, dt, per_agent in trajectory:
                fields['rec_' + name] = self._ptr(res[name][sl], dt, (n, E, A) if per_agent else (n, E), name)
            # (the truncation outputs are mapf_rollout_limited's two arguments behind the block, which stays mapf_rollout's)
            # (... and the live steps mapf_rollout_budgeted's third; without a limit its truncation arguments are NULL)
            beside = (fields.pop('out_truncations', None), fields.pop('rec_truncated', None)) if (limited or budgeted) else ()
            entry = self._lib.mapf_rollout_limited if limited else self._lib.mapf_rollout
            if budgeted:
                beside, entry = beside + (fields.pop('out_live_steps'),), self._lib.mapf_rollout_budgeted
            io = nat.MapfRolloutIO(struct_size=ctypes.sizeof(nat.MapfRolloutIO), n_steps=n, step_flags=nat.MAPF_STEP_AUTO_RESET if auto_reset else 0,
                                   accumulate=1 if accumulate else 0, **fields)
            call_args = (entry, self._h, ctypes.byref(io)) + beside
            nat.check(call_args[0](*call_args[1:]))
            first += n
            if first >= T:
                if out is not None and accumulate_into is None and n == T and self.device_arrays:
                    # (one launch covered the call: its argument block serves the next call with the same arrays; the arrays are
                    # referenced here, so their memory cannot be handed to anyone else while the block is kept)
                    keys = [name for name, _ in total_spec] + [name for name, _, _ in trajectory]
                    self._rollout_io = _RolloutIO(out, (T, bool(auto_reset), bool(record)), tuple((k, res[k]) for k in keys),
                                                  None if actions is None else (actions.data_ptr(), tuple(actions.shape), actions), io, call_args)
                return res
            accumulate = True

    def transitions(self, local, actions, max_branches=None, env_index=None, first_branch=0, out=None):
        """``env.P[s][a]`` for N (state, joint action) queries (reference mapf_env.py:448-478): every branch of the
        joint slip distribution in the reference's order.  ``local`` uint16 [N, A], ``actions`` uint8 [N, A],
        ``env_index`` uint32 [N] picks whose goals apply (default env 0).  Returns a dict: ``count`` uint32 [N] (always
        the full number of branches) and, for the window of ``max_branches`` branches (default 3**A) that starts at
        ``first_branch``, ``next`` uint16 [N, M, A], ``prob`` / ``reward`` float64 [N, M], ``done`` / ``collision``
        uint8 [N, M].  Rows whose branch index is >= count[q] are unspecified.  Up to 16 agents."""
        A = self.n_agents
        N, alive, queries = self._queries(local, actions, env_index)    # (alive: the coerced arrays, held across the call)
        M = int(max_branches) if max_branches is not None else 3 ** A
        res, outputs = self._outputs((('count', np.uint32, (N,)), ('next', np.uint16, (N, M, A)), ('prob', np.float64, (N, M)),
                                      ('reward', np.float64, (N, M)), ('done', np.uint8, (N, M)), ('collision', np.uint8, (N, M))), out)
        nat.check(self._lib.mapf_transitions_window(self._h, N, *queries, int(first_branch), M, *outputs))
        return res

    def _queries(self, local, actions, env_index):
        """The query arrays of both transitions calls: (N, the arrays to keep alive across the call, their pointers)."""
        A, local = self.n_agents, (local if self.device_arrays else np.asarray(local))
        N = int(local.shape[0])
        return (N,) + self._inputs(('local', np.uint16, (N, A), local), ('actions', np.uint8, (N, A), actions),
                                   ('env_index', np.uint32, (N,), env_index))

    def transitions_compact(self, local, actions, env_index=None, first_branch=0, max_branches=None, capacity=None, out=None):
        """``env.P[s][a]`` for N queries with COMPACTED rows (``mapf_transitions_compact``): the branches of query q are
        rows ``offset[q] .. offset[q + 1] - 1`` of ``next`` uint16 [R, A], ``prob`` / ``reward`` float64 [R], ``done`` /
        ``collision`` uint8 [R], in the reference's order (mapf_env.py:448-478); ``offset`` uint64 [N + 1], ``count``
        uint32 [N] (full branch counts).  ``capacity`` = R, the rows the arrays hold (default: N * min(3**A, max_branches),
        which always suffices); rows beyond it are not written -- check ``offset[N] <= R`` (after ``sync()`` in device
        mode).  ``out`` reuses the arrays of an earlier call."""
        A = self.n_agents
        N, alive, queries = self._queries(local, actions, env_index)    # (alive: the coerced arrays, held across the call)
        M = min(int(max_branches), 3 ** A) if max_branches is not None else 3 ** A
        R = int(out['prob'].shape[0]) if out is not None else int(capacity) if capacity is not None else N * M
        res, outputs = self._outputs((('offset', np.uint64, (N + 1,)), ('count', np.uint32, (N,)), ('next', np.uint16, (R, A)), ('prob', np.float64, (R,)),
                                      ('reward', np.float64, (R,)), ('done', np.uint8, (R,)), ('collision', np.uint8, (R,))), out)
        nat.check(self._lib.mapf_transitions_compact(self._h, N, *queries, int(first_branch), max(1, M), R, *outputs))
        return res

    def transition_rewards(self, prev_local, actions, next_local, env_index=None, want_done=True, want_collision=True):
        """``calc_transition_reward_from_local_states`` (reference mapf_env.py:225-235) for N given transitions:
        ``prev_local`` / ``next_local`` uint16 [N, A], ``actions`` uint8 [N, A].  Returns ``(reward f64 [N],
        done u8 [N], collision u8 [N])``; with ``want_done`` / ``want_collision`` False that output is not computed
        (the C ABI gets NULL for it) and None is returned in its place."""
        A, prev_local = self.n_agents, (prev_local if self.device_arrays else np.asarray(prev_local))
        N = int(prev_local.shape[0])
        alive, queries = self._inputs(('prev_local', np.uint16, (N, A), prev_local), ('actions', np.uint8, (N, A), actions),
                                     ('next_local', np.uint16, (N, A), next_local), ('env_index', np.uint32, (N,), env_index))    # (alive: as above)
        skip = [name for name, wanted in (('done', want_done), ('collision', want_collision)) if not wanted]
        res, outputs = self._outputs((('reward', np.float64, (N,)), ('done', np.uint8, (N,)), ('collision', np.uint8, (N,))), skip=skip)
        nat.check(self._lib.mapf_transition_rewards(self._h, N, *queries, *outputs))
        return res['reward'], res.get('done'), res.get('collision')

    def fill_random_actions(self, t0, n_steps, out=None):
        """Synthetic policy stream: uint8 [n_steps, E, A] uniform over the 5 actions."""
        shape = (int(n_steps), self.n_envs, self.n_agents)
        if out is None:
            out = self._empty(shape, np.uint8)
        nat.check(self._lib.mapf_fill_random_actions(self._h, self._ptr(out, np.uint8, shape, 'out'),
                                                     int(t0), int(n_steps)))
        return out

    def set_policy(self, policy='random', table=None, rows=None, offsets=None, partners=None, members=None, book=None, entry_cells=None,
                   entry_actions=None, book_begin=None):
        """On-device policy of ``rollout(actions=None)``: ``'random'`` (default; the uniform-random action stream),
        ``'greedy'`` -- every agent takes the first action in ACTIONS order whose intended target is closest
        (Manhattan distance) to its goal, i.e. the first unblocked move one step closer, else STAY -- or ``'table'``:
        the caller's plan.  ``table`` array-like uint8 [R, V] of action codes 0..4 (``table[r, cell]`` = what an agent
        that follows row ``r`` does on ``cell``), ``rows`` [E, A] or [A] = the row every agent follows; both HOST arrays
        (numpy or CPU torch) in either handle mode, copied.  ``envs/policies.py`` builds such tables (shortest paths,
        or the row of a single-agent policy planned on a ``get_local_view``).  The reference has no policy; this
        stands in for the caller-side ``a = policy(s)`` of the loop around ``step`` (mapf_env.py:237-266).

        ``'joint'``: a plan in which some agent PAIRS were merged and replanned jointly (include/mapf_hip.h MAPF_POLICY_JOINT).
        ``table`` uint8 [N] of action codes, ``offsets`` [E, A] or [A] = where every agent's segment begins, ``partners`` [E, A]
        or [A] = the agent it is merged with, or itself; HOST arrays, copied.  A solo agent on cell ``c`` takes
        ``table[offsets[e, i] + c]``, an agent merged with ``j`` takes ``table[offsets[e, i] + c_i * V + c_j]``.
        ``envs/policies.py`` builds the three (``pair_shortest_path_rows``, ``pair_rows_from_policy``, ``join_plan``).  Joint
        launches always run a lane-group kernel (``last_kernel`` says JOINT); ``graph_begin`` is refused in this mode.

        ``'group'``: a plan in which GROUPS of two to four agents were merged and replanned on the joint cells the planner visited
        (include/mapf_hip.h MAPF_POLICY_GROUP).  ``table`` [R, V] and ``rows`` [E, A] or [A] are the solo rows of ``'table'``;
        ``members`` [E, A, 4] or [A, 4] lists every agent's group in ascending order, padded with 0xFFFF; ``book`` [E, A] or [A] names
        the group's book; ``entry_cells`` uint16 [N, 4] and ``entry_actions`` uint8 [N, 4] are the entries of all books (padded
        positions: 0xFFFF and 0), ``book_begin`` [n_books + 1] where each book begins; HOST arrays, copied.  An agent of a group takes
        its byte of the entry whose cells equal the members' cells if the group's book has one, else ``table[rows[e, i], c]``.
        ``envs/policies.py`` builds them (``group_shortest_path_entries``, ``group_entries_from_policy``, ``join_group_plan``).  Group
        launches always run a lane-group kernel (``last_kernel`` says GROUP); ``graph_begin`` is refused in this mode."""
        if policy == 'group':
            if offsets is not None or partners is not None:
                raise ValueError("offsets= and partners= belong to policy='joint'")
            V = len(self.grid.tables()[0])
            args = self._group_arguments(V, self.n_envs, self.n_agents, table, rows, members, book, entry_cells, entry_actions, book_begin)
            table8, rows16, members16, book32, entries, begin32 = args
            # (entries and book_begin may be null only without books: books that are all empty still name an array)
            no_books = begin32.size == 1
            held = entries if entries.size else np.zeros(1, entries.dtype)
            nat.check(self._lib.mapf_set_policy_group(self._h, table8.ctypes.data, table8.shape[0], rows16.ctypes.data, members16.ctypes.data, book32.ctypes.data,
                                                      None if no_books else held.ctypes.data, entries.size,
                                                      None if no_books else begin32.ctypes.data, begin32.size - 1,
                                                      nat.MAPF_POLICY_ROWS_BROADCAST if rows16.ndim == 1 else 0))
            self._rollout_io = None
            self.policy = policy
            return
        if any(a is not None for a in (members, book, entry_cells, entry_actions, book_begin)):
            raise ValueError("members=, book=, entry_cells=, entry_actions= and book_begin= belong to policy='group'")
        if (policy not in ('table', 'joint') and table is not None) or (policy != 'table' and rows is not None):
            raise ValueError("table= and rows= belong to policy='table'" + (" (policy='joint' takes table=, offsets= and partners=)" if policy == 'joint' else ''))
        if policy != 'joint' and (offsets is not None or partners is not None):
            raise ValueError("offsets= and partners= belong to policy='joint'")
        if policy == 'random':
            nat.check(self._lib.mapf_set_policy(self._h, nat.MAPF_POLICY_RANDOM, None))
        elif policy == 'greedy':
            valid, _, _ = self.grid.tables()
            rc = np.ascontiguousarray([r | (c << 16) for r, c in valid], dtype=np.uint32)
            nat.check(self._lib.mapf_set_policy(self._h, nat.MAPF_POLICY_GREEDY, rc.ctypes.data))
        elif policy == 'table':
            if table is None or rows is None:
                raise ValueError("policy='table' needs table= [R, V] and rows= [E, A] or [A]")
            V = len(self.grid.tables()[0])
            table, rows = self._host_ints(table, 'table'), self._host_ints(rows, 'rows')
            if table.ndim != 2 or table.shape[1] != V or not 1 <= table.shape[0] <= 65536:
                raise ValueError('table must be [R, V] with V = %d free cells and 1 <= R <= 65536, got %r' % (V, tuple(table.shape)))
            if tuple(rows.shape) not in ((self.n_envs, self.n_agents), (self.n_agents,)):
                raise ValueError('rows must be [E, A] = %r or [A], got %r' % ((self.n_envs, self.n_agents), tuple(rows.shape)))
            if table.size and (table.min() < 0 or table.max() > 4):
                raise ValueError('table holds action codes 0..4 (STAY, UP, RIGHT, DOWN, LEFT), found %d' % (table.max() if table.max() > 4 else table.min()))
            if rows.min() < 0 or rows.max() >= table.shape[0]:
                raise ValueError('rows must name table rows 0..%d, found %d' % (table.shape[0] - 1, rows.max() if rows.max() >= table.shape[0] else rows.min()))
            table8, rows16 = np.ascontiguousarray(table, dtype=np.uint8), np.ascontiguousarray(rows, dtype=np.uint16)
            nat.check(self._lib.mapf_set_policy_table(self._h, table8.ctypes.data, table8.shape[0], rows16.ctypes.data,
                                                      nat.MAPF_POLICY_ROWS_BROADCAST if rows16.ndim == 1 else 0))
        elif policy == 'joint':
            V = len(self.grid.tables()[0])
            table8, offsets32, partners16 = self._joint_arguments(V, self.n_envs, self.n_agents, table, offsets, partners)
            nat.check(self._lib.mapf_set_policy_joint(self._h, table8.ctypes.data, table8.size, offsets32.ctypes.data, partners16.ctypes.data,
                                                      nat.MAPF_POLICY_ROWS_BROADCAST if offsets32.ndim == 1 else 0))
        else:
            raise ValueError("policy must be 'random', 'greedy', 'table', 'joint' or 'group'")
        self._rollout_io = None            # (a cached argument block must not outlive a policy change)
        self.policy = policy

    @staticmethod
    def _joint_arguments(V, n_envs, n_agents, table, offsets, partners):
        """The three arrays of ``set_policy('joint')`` as the library takes them -- (uint8 [N], uint32, uint16) -- after the checks
        the library repeats (include/mapf_hip.h MAPF_POLICY_JOINT); a ``ValueError`` names the offending entry.  Needs no handle."""
        if table is None or offsets is None or partners is None:
            raise ValueError("policy='joint' needs table= [N], offsets= and partners= [E, A] or [A]")
        table, offsets, partners = (VecMapfEnv._host_ints(a, name) for a, name in ((table, 'table'), (offsets, 'offsets'), (partners, 'partners')))
        if table.ndim != 1 or not 1 <= table.size <= 0x7FFFFFFF:
            raise ValueError('table must be [N] with 1 <= N <= 2**31 - 1, got %r' % (tuple(table.shape),))
        shapes = ((n_envs, n_agents), (n_agents,))
        if tuple(offsets.shape) not in shapes or tuple(partners.shape) != tuple(offsets.shape):
            raise ValueError('offsets and partners must both be [E, A] = %r or both [A], got %r and %r' % (shapes[0], tuple(offsets.shape), tuple(partners.shape)))
        bad = np.flatnonzero((table < 0) | (table > 4))
        if bad.size:
            raise ValueError('table holds action codes 0..4 (STAY, UP, RIGHT, DOWN, LEFT), found table[%d] = %d' % (bad[0], table[bad[0]]))
        part = partners.reshape(-1, n_agents).astype(np.int64)
        off = offsets.reshape(-1, n_agents).astype(np.int64)
        where = lambda k: '[%d, %d]' % (k[0], k[1]) if offsets.ndim == 2 else '[%d]' % k[1]   # (the entry's name: [e, i], or [i] of shared arrays)
        bad = np.argwhere((part < 0) | (part >= n_agents))
        if bad.size:
            raise ValueError('partners%s = %d is not an agent 0..%d' % (where(bad[0]), part[tuple(bad[0])], n_agents - 1))
        me = np.arange(n_agents, dtype=np.int64)[None, :]
        bad = np.argwhere(np.take_along_axis(part, part, axis=1) != me)
        if bad.size:
            e, i = bad[0]
            raise ValueError('partners%s = %d, but agent %d is merged with %d: the merge is not mutual' % (where(bad[0]), part[e, i], part[e, i], part[e, part[e, i]]))
        if off.min() < 0 or off.max() > 0xFFFFFFFF:
            raise ValueError('offsets must be 0 .. 2**32 - 1')
        bad = np.argwhere(off + np.where(part == me, V, V * V) > table.size)
        if bad.size:
            raise ValueError('offsets%s = %d: the segment of %d bytes ends past the table of %d' % (where(bad[0]), off[tuple(bad[0])],
                                                                                               V if part[tuple(bad[0])] == bad[0][1] else V * V, table.size))
        return (np.ascontiguousarray(table, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.uint32), np.ascontiguousarray(partners, dtype=np.uint16))

    def policy_group_stats(self):
        """(slots, longest probe chain) of the device table of a handle under ``set_policy('group')``"""
        slots, chain = ctypes.c_uint64(0), ctypes.c_uint32(0)
        nat.check(self._lib.mapf_policy_group_stats(self._h, ctypes.byref(slots), ctypes.byref(chain)))
        return slots.value, chain.value

    @staticmethod
    def _group_arguments(V, n_envs, n_agents, table, rows, members, book, entry_cells, entry_actions, book_begin):
        """The arrays of ``set_policy('group')`` as the library takes them -- (uint8 [R, V], uint16 rows, uint16 members, uint32 book,
        entries as ``_native.GROUP_ENTRY_DTYPE`` [N], uint32 book_begin [n_books + 1]) -- after the checks the library repeats
        (include/mapf_hip.h MAPF_POLICY_GROUP); a ``ValueError`` names the offending entry.  ``entry_cells``, ``entry_actions`` and
        ``book_begin`` may all be None: no books.  Needs no handle."""
        if table is None or rows is None or members is None or book is None:
            raise ValueError("policy='group' needs table= [R, V], rows= and book= [E, A] or [A], members= [E, A, 4] or [A, 4]")
        if (entry_cells is None) != (entry_actions is None) or (entry_cells is None) != (book_begin is None):
            raise ValueError("entry_cells=, entry_actions= and book_begin= come together (or none of them: no books)")
        if V > 65535:
            raise ValueError("policy='group' needs a map of at most 65535 free cells (cell 0xFFFF is the padding of keys), got %d" % V)
        ints = VecMapfEnv._host_ints
        table, rows, members, book = ints(table, 'table'), ints(rows, 'rows'), ints(members, 'members'), ints(book, 'book')
        if table.ndim != 2 or table.shape[1] != V or not 1 <= table.shape[0] <= 65536:
            raise ValueError('table must be [R, V] with V = %d free cells and 1 <= R <= 65536, got %r' % (V, tuple(table.shape)))
        shapes = ((n_envs, n_agents), (n_agents,))
        if tuple(rows.shape) not in shapes or tuple(book.shape) != tuple(rows.shape) or tuple(members.shape) != tuple(rows.shape) + (4,):
            raise ValueError('rows and book must both be [E, A] = %r or both [A], and members that shape + [4]; got %r, %r and %r'
                             % (shapes[0], tuple(rows.shape), tuple(book.shape), tuple(members.shape)))
        bad = np.argwhere((table < 0) | (table > 4))
        if bad.size:
            raise ValueError('table holds action codes 0..4 (STAY, UP, RIGHT, DOWN, LEFT), found table[%d, %d] = %d' % (bad[0][0], bad[0][1], table[tuple(bad[0])]))
        if rows.min() < 0 or rows.max() >= table.shape[0]:
            raise ValueError('rows must name table rows 0..%d, found %d' % (table.shape[0] - 1, rows.max() if rows.max() >= table.shape[0] else rows.min()))
        if entry_cells is None:
            cells, actions, begin = np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int64), np.zeros(1, np.int64)
        else:
            cells, actions, begin = ints(entry_cells, 'entry_cells'), ints(entry_actions, 'entry_actions'), ints(book_begin, 'book_begin')
            begin = begin.astype(np.int64)
        if cells.ndim != 2 or cells.shape[1] != 4 or tuple(actions.shape) != tuple(cells.shape) or cells.shape[0] > 1 << 24:
            raise ValueError('entry_cells and entry_actions must both be [N, 4] with N <= 2**24, got %r and %r' % (tuple(cells.shape), tuple(actions.shape)))
        if begin.ndim != 1 or begin.size < 1 or begin[0] != 0 or begin[-1] != cells.shape[0] or (np.diff(begin) < 0).any():
            raise ValueError('book_begin must be [n_books + 1], non-decreasing from 0 to N = %d, got %r' % (cells.shape[0], begin.tolist()[:8]))
        n_books = begin.size - 1
        PAD = nat.MAPF_GROUP_PAD
        where = lambda k: '[%d, %d]' % (k[0], k[1]) if rows.ndim == 2 else '[%d]' % k[1]   # (the entry's name: [e, i], or [i] of shared arrays)
        mem = members.reshape(-1, n_agents, 4).astype(np.int64)
        bk = book.reshape(-1, n_agents).astype(np.int64)
        pad = mem == PAD
        bad = np.argwhere(~pad & ((mem < 0) | (mem >= n_agents)))
        if bad.size:
            raise ValueError('members%s[%d] = %d is not an agent 0..%d and not padding (0xFFFF)' % (where(bad[0]), bad[0][2], mem[tuple(bad[0])], n_agents - 1))
        bad = np.argwhere(pad[:, :, :-1] & ~pad[:, :, 1:])
        if bad.size:
            raise ValueError('members%s[%d] follows padding: padding must be trailing' % (where(bad[0]), bad[0][2] + 1))
        bad = np.argwhere(~pad[:, :, 1:] & (mem[:, :, 1:] <= mem[:, :, :-1]))
        if bad.size:
            raise ValueError('members%s is not ascending at position %d' % (where(bad[0]), bad[0][2] + 1))
        me = np.arange(n_agents, dtype=np.int64)[None, :, None]
        bad = np.argwhere(~(mem == me).any(axis=2))
        if bad.size:
            raise ValueError('members%s does not contain agent %d itself' % (where(bad[0]), bad[0][1]))
        size = (~pad).sum(axis=2)
        other = np.where(pad, me, mem)                                     # (a padded position: the agent itself)
        rows_of = np.arange(mem.shape[0])[:, None, None]
        bad = np.argwhere((mem[rows_of, other] != mem[:, :, None, :]).any(axis=3))
        if bad.size:
            e, i, k = bad[0]
            raise ValueError('members%s names agent %d, whose list differs' % (where(bad[0]), other[e, i, k]))
        booked = (size >= 2) & (n_books != 0)                              # (without books every group falls back to its rows: book is not read)
        bad = np.argwhere(booked & ((bk < 0) | (bk >= n_books)))
        if bad.size:
            raise ValueError('book%s = %d is not a book 0..%d' % (where(bad[0]), bk[tuple(bad[0])], n_books - 1))
        bad = np.argwhere(booked[:, :, None] & (bk[rows_of, other] != bk[:, :, None]))
        if bad.size:
            e, i, k = bad[0]
            raise ValueError('book%s = %d, but agent %d of the same group has book %d' % (where(bad[0]), bk[e, i], other[e, i, k], bk[e, other[e, i, k]]))
        if (bk < 0).any() or (bk > 0xFFFFFFFF).any():
            raise ValueError('book must be 0 .. 2**32 - 1')
        cpad = cells == PAD
        bad = np.argwhere(~cpad & ((cells < 0) | (cells >= V)))
        if bad.size:
            raise ValueError('entry_cells[%d, %d] = %d is not a cell 0..%d and not padding (0xFFFF)' % (bad[0][0], bad[0][1], cells[tuple(bad[0])], V - 1))
        bad = np.argwhere(cpad[:, :-1] & ~cpad[:, 1:])
        if bad.size:
            raise ValueError('entry_cells[%d, %d] follows padding: padding must be trailing' % (bad[0][0], bad[0][1] + 1))
        bad = np.argwhere((actions < 0) | (actions > 4))
        if bad.size:
            raise ValueError('entry_actions[%d, %d] = %d is not an action code 0..4' % (bad[0][0], bad[0][1], actions[tuple(bad[0])]))
        bad = np.argwhere(cpad & (actions != 0))
        if bad.size:
            raise ValueError('entry_actions[%d, %d] = %d at a padded position must be 0' % (bad[0][0], bad[0][1], actions[tuple(bad[0])]))
        if cells.shape[0]:
            keyed = np.concatenate([np.repeat(np.arange(n_books), np.diff(begin))[:, None], cells], axis=1)
            order = np.lexsort(keyed.T[::-1])
            same = np.flatnonzero((keyed[order][1:] == keyed[order][:-1]).all(axis=1))
            if same.size:
                a, b = sorted((int(order[same[0]]), int(order[same[0] + 1])))
                raise ValueError('entry_cells[%d] has the same four cells as entry_cells[%d] of the same book' % (b, a))
        entries = np.zeros(cells.shape[0], nat.GROUP_ENTRY_DTYPE)
        entries['cell'], entries['action'] = cells, actions
        return (np.ascontiguousarray(table, dtype=np.uint8), np.ascontiguousarray(rows, dtype=np.uint16), np.ascontiguousarray(members, dtype=np.uint16),
                np.ascontiguousarray(book, dtype=np.uint32), entries, np.ascontiguousarray(begin, dtype=np.uint32))

    def set_episode_limit(self, n):
        """Episode step limit: an episode that has taken ``n`` steps without ending is TRUNCATED -- with ``auto_reset`` the env goes
        back to its start cells as after ``done``, without it the env lives on and reports ``truncated`` on every later step.
        ``None`` or 0 switches the limit off (the default).  Truncation changes no reward, no ``done`` and no random number; every
        call zeroes the per-env step counts (``episode_steps``).  With a limit ``rollout`` also returns ``truncations`` (and
        ``truncated`` when recording), ``step``'s ``info`` gains ``truncated``, and the launches run the lane-group kernels' limit
        instances (``last_kernel`` says LIMIT).  The reference has no limit: this is the caller-side ``TimeLimit`` / "n episodes of
        at most max_steps" loop around ``MapfEnv.step`` (mapf_env.py:237-266), done inside the launch."""
        n = 0 if n is None else n
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= 0xFFFFFFFF:
            raise ValueError('the episode limit must be None or an integer 0 .. 2**32 - 1, got %r' % (n,))
        nat.check(self._lib.mapf_set_episode_limit(self._h, int(n)))
        self._rollout_io = None            # (a cached argument block names the arrays of the other mode)
        self.episode_limit = int(n)

    def set_episode_budget(self, n):
        """Episode budget: every env stops after ``n`` episodes.  An episode ends with ``done`` or ``truncated`` (``set_episode_limit``);
        an env that has ended ``n`` of them is PARKED on its start cells and later steps of a ``rollout`` do nothing for it -- no
        move, no random number, no total; a recording rollout writes the env's cells and zeros (``done == 0`` and ``prob == 0``).  So
        totals-only rollouts give unbiased per-env episode statistics: exactly ``n`` episodes each and no cut-off episode in
        ``returns`` once every env is parked (``episodes_left().max() == 0``).  ``None`` or 0 switches the budget off (the default);
        every call re-arms every env and touches neither state nor ages.  With a budget ``rollout`` also returns ``live_steps``, needs
        ``auto_reset=True``, and runs the lane-group kernels' budget instances (``last_kernel`` says BUDGET); ``step`` and
        ``graph_begin`` are refused.  Not covered: the multi-map and union-map wrappers and the scalar ``MapfEnv``."""
        n = 0 if n is None else n
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= 0xFFFFFFFF:
            raise ValueError('the episode budget must be None or an integer 0 .. 2**32 - 1, got %r' % (n,))
        nat.check(self._lib.mapf_set_episode_budget(self._h, int(n)))
        self._rollout_io = None            # (a cached argument block names the arrays of the other mode)
        self.episode_budget = int(n)

    def episodes_left(self, out=None, set=None):
        """The episodes every env may still end, uint32 [E] (all zero without a budget; 0 = parked); ``set`` uint32 [E] replaces them
        afterwards -- per-env budgets, or re-arming single envs (needs a budget).  Host arrays, or CUDA tensors in device mode (then
        only enqueued).  Not covered: the multi-map and union-map wrappers and the scalar ``MapfEnv``."""
        shape = (self.n_envs,)
        set = self._coerce(set, np.uint32, shape, 'set')
        if out is None:
            out = self._empty(shape, np.uint32)
        nat.check(self._lib.mapf_episodes_left(self._h, self._ptr(out, np.uint32, shape, 'out'), self._ptr(set, np.uint32, shape, 'set')))
        return out

    def set_conflict_pairs(self, n_slots=1, slots=None):
        """Conflict matrix: from now on every ``rollout`` counts, per agent pair, the vertex conflicts and the swaps of its live steps
        into ``M`` uint64 [n_slots, A, A] on the device (``conflict_pairs`` reads it): ``M[slot, i, j]``, i < j, counts the steps on
        which agents i and j moved onto one cell, ``M[slot, j, i]`` the steps on which they traded cells; all conflicting pairs of a
        step count.  ``slots`` uint32 [E] (a HOST array in both modes; copied) names every env's slot, ``None`` puts all envs in slot
        0.  ``n_slots`` ``None`` or 0 switches the mode off (the default); every call zeroes ``M``.  Nothing else of a rollout
        changes; it runs the lane-group kernels' instances that count (``last_kernel`` says PAIRS), ``step`` counts nothing and
        ``graph_begin`` is refused.  Not covered: the multi-map and union-map wrappers and the scalar ``MapfEnv``."""
        n_slots = 0 if n_slots is None else n_slots
        if isinstance(n_slots, bool) or not isinstance(n_slots, (int, np.integer)) or not 0 <= int(n_slots) <= 0xFFFFFFFF:
            raise ValueError('n_slots must be None or an integer 0 .. 2**32 - 1, got %r' % (n_slots,))
        ptr = None
        if slots is not None:
            slots = self._host_ints(slots, 'slots')
            if slots.shape != (self.n_envs,) or (slots.size and (slots.min() < 0 or slots.max() > 0xFFFFFFFF)):
                raise ValueError('slots must be %d non-negative integers below n_slots' % self.n_envs)
            slots = np.ascontiguousarray(slots, dtype=np.uint32)
            ptr = slots.ctypes.data
        nat.check(self._lib.mapf_set_conflict_pairs(self._h, int(n_slots), ptr))
        self._rollout_io = None
        self.conflict_slots = int(n_slots)

    def conflict_pairs(self, out=None, zero=False):
        """The conflict matrix, uint64 [n_slots, A, A] (``set_conflict_pairs``): the upper triangle counts vertex conflicts, the lower
        one swaps, the diagonal is zero.  ``zero=True`` clears the device's counts after the read.  A host array, or a CUDA tensor in
        device mode (then only enqueued).  ``policies.conflicts`` and ``policies.conflicting_pairs`` read it."""
        if not self.conflict_slots:
            raise ValueError('the env has no conflict matrix (set_conflict_pairs)')
        shape = (self.conflict_slots, self.n_agents, self.n_agents)
        if out is None:
            out = self._empty(shape, np.uint64)
        nat.check(self._lib.mapf_conflict_pairs(self._h, self._ptr(out, np.uint64, shape, 'out'), 1 if zero else 0))
        return out

    def set_episode_log(self, capacity):
        """Episode log: from now on every ``rollout`` under the episode budget (``set_episode_budget`` first) records each finished
        episode per env -- its return, its live steps and how it ended -- for the first ``capacity`` episodes an env ends after a
        clear; later ones are counted only (``count > capacity``).  ``None`` or 0 switches the mode off (the default); every call
        empties the log and drops the running episodes' partial sums.  Nothing else of a rollout changes; it runs the lane-group
        kernels' log instances (``last_kernel`` says LOG next to BUDGET) and ``graph_begin`` is refused.  ``reset`` and ``set_state``
        with cells drop the running partial sums of the envs they touch; a clear and a re-armed budget do not, so an episode that
        spans them is logged whole.  Not covered: the multi-map and union-map wrappers and the scalar ``MapfEnv``."""
        capacity = 0 if capacity is None else capacity
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 0 <= int(capacity) <= 0xFFFFFFFF:
            raise ValueError('the capacity of the episode log must be None or an integer 0 .. 2**32 - 1, got %r' % (capacity,))
        nat.check(self._lib.mapf_set_episode_log(self._h, int(capacity)))
        self._rollout_io = None
        self.episode_log_capacity = int(capacity)

    def episode_log(self, out=None, clear=False):
        """The episode log (``set_episode_log``) as a dict: ``returns`` float64 [E, C], ``steps`` uint32 [E, C], ``outcome`` uint8
        [E, C] (bit 0 done, bit 1 collision, bit 2 truncated: 1 = on the goals, 3 = by a collision, 4 = cut by the step limit) and
        ``count`` uint32 [E], the episodes each env has ended since the last clear -- columns from ``min(count, C)`` on are zero.
        ``clear=True`` empties the log after the read (the running episodes' partial sums stay).  ``out`` may hold ``records``
        (the raw 16-byte records: a numpy array of ``_native.EPISODE_RECORD_DTYPE`` [E, C], in device mode a uint8 CUDA tensor
        [E, C, 16]) and ``count`` to read into.  Host arrays, or CUDA tensors in device mode (the call then waits for the env's stream
        before it cuts the records into columns)."""
        C = self.episode_log_capacity
        if not C:
            raise ValueError('the env has no episode log (set_episode_log)')
        E, out = self.n_envs, ({} if out is None else out)
        count = out.get('count')
        if count is None:
            count = self._empty((E,), np.uint32)
        records = out.get('records')
        if self.device_arrays:
            if records is None:
                records = self._empty((E, C, 16), np.uint8)
            rec_ptr = self._ptr(records, np.uint8, (E, C, 16), 'records')
        else:
            if records is None:
                records = np.empty((E, C), dtype=nat.EPISODE_RECORD_DTYPE)
            if not isinstance(records, np.ndarray) or records.dtype != np.dtype(nat.EPISODE_RECORD_DTYPE) or records.shape != (E, C) \
                    or not records.flags['C_CONTIGUOUS']:
                raise ValueError('records must be a C-contiguous numpy array of _native.EPISODE_RECORD_DTYPE with shape %r' % ((E, C),))
            rec_ptr = records.ctypes.data
        nat.check(self._lib.mapf_episode_log(self._h, rec_ptr, self._ptr(count, np.uint32, (E,), 'count'), 1 if clear else 0))
        if self.device_arrays:
            torch = self._torch
            self.sync()                                            # (the columns are cut on torch's stream: the raw records must have landed)
            words = records.view(torch.int32)                     # [E, C, 4]: ret lo, ret hi, steps, outcome
            res = {'returns': records[:, :, :8].contiguous().view(torch.float64).reshape(E, C),
                   'steps': words[:, :, 2].contiguous().view(torch.uint32), 'outcome': records[:, :, 12].contiguous()}
        else:
            res = {'returns': np.ascontiguousarray(records['ret']), 'steps': np.ascontiguousarray(records['steps']),
                   'outcome': records['outcome'].astype(np.uint8)}
        res['count'] = count
        res['records'] = records
        return res

    def episode_steps(self, out=None, set=None):
        """The steps every env's current episode has taken since it began, uint32 [E] (all zero without a limit); ``set`` uint32 [E]
        replaces them afterwards (needs a limit).  Host arrays, or CUDA tensors in device mode (then only enqueued)."""
        shape = (self.n_envs,)
        set = self._coerce(set, np.uint32, shape, 'set')
        if out is None:
            out = self._empty(shape, np.uint32)
        nat.check(self._lib.mapf_episode_steps(self._h, self._ptr(out, np.uint32, shape, 'out'), self._ptr(set, np.uint32, shape, 'set')))
        return out

    @staticmethod
    def _host_ints(a, name):
        """A host integer array from numpy / CPU torch / nested lists (the table policy's arguments are host data in both modes)."""
        if hasattr(a, 'is_cuda'):
            if a.is_cuda:
                raise ValueError('%s must be a host array (numpy or CPU torch): it is copied by the library' % name)
            a = a.numpy()
        a = np.asarray(a)
        if a.dtype.kind not in 'iu':
            raise ValueError('%s must be an integer array, got %s' % (name, a.dtype))
        return a.astype(np.int64, copy=False) if a.dtype.kind == 'i' else a

    def query_terminal(self, out=None):
        """``MapfEnv.is_terminal`` of every env's current state: uint8 [E]."""
        if out is None:
            out = self._empty((self.n_envs,), np.uint8)
        nat.check(self._lib.mapf_query_terminal(self._h, self._ptr(out, np.uint8, (self.n_envs,), 'out')))
        return out

    def get_state(self, out=None):
        """(local uint16 [E, A], step index t)."""
        shape = (self.n_envs, self.n_agents)
        if out is None:
            out = self._empty(shape, np.uint16)
        t = ctypes.c_uint64(0)
        nat.check(self._lib.mapf_get_state(self._h, self._ptr(out, np.uint16, shape, 'out'), ctypes.byref(t)))
        return out, t.value

    def set_state(self, local=None, t=None):
        shape = (self.n_envs, self.n_agents)
        local = self._coerce(local, np.uint16, shape, 'local')
        if t is None:
            t = self.t
        nat.check(self._lib.mapf_set_state(self._h, self._ptr(local, np.uint16, shape, 'local'), int(t)))

    @property
    def t(self):
        t = ctypes.c_uint64(0)
        nat.check(self._lib.mapf_get_state(self._h, None, ctypes.byref(t)))
        return t.value

    def sync(self):
        nat.check(self._lib.mapf_sync(self._h))

    def timer_begin(self):
        nat.check(self._lib.mapf_timer_begin(self._h))

    def timer_end(self):
        ms = ctypes.c_double(0.0)
        nat.check(self._lib.mapf_timer_end(self._h, ctypes.byref(ms)))
        return ms.value

    def last_kernel(self, which='rollout'):
        """Name of the kernel instance that took this env's last ``step`` / ``rollout`` launch (the library picks
        the lane layout from A, E and the table size); '' before the first launch."""
        code = {'step': nat.MAPF_KERNEL_STEP, 'rollout': nat.MAPF_KERNEL_ROLLOUT, 'transitions': nat.MAPF_KERNEL_TRANSITIONS}[which]
        return self._lib.mapf_last_kernel(self._h, code).decode()

    @property
    def stream(self):
        s = ctypes.c_void_p()
        nat.check(self._lib.mapf_get_stream(self._h, ctypes.byref(s)))
        return s.value

    def close(self):
        h, self._h = getattr(self, '_h', None), None
        self._rollout_io = None
        if h:
            self._lib.mapf_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
