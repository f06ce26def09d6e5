"""The stand-in for libmapf_hip.so that the host-mode tests of the Python layer record C calls with (tests/test_host_call_trace.py,
tests/test_vec_env_arguments.py).  A plain module, no test in it."""
import ctypes
import hashlib

import numpy as np

from gym_mapf_amd import _native as nat

_INTS = (ctypes.c_int, ctypes.c_int32, ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64)


class Recorder:
    """Stands in for libmapf_hip.so.  Arguments are read by the C signature (_native.SIGNATURES): integers and floats by value,
    ``void *`` as null / non-null (resolved to an offset into a watched array by ``resolve``), structs field by field."""

    def __init__(self):
        self.trace, self.step, self._handles, self._watched, self._pending = [], '', {}, [], []

    def __getattr__(self, name):
        if not name.startswith('mapf_'):
            raise AttributeError(name)
        restype, argtypes = nat.SIGNATURES[name]

        def fn(*args):
            assert len(args) == len(argtypes), name
            entry = {'step': self.step, 'fn': name, 'args': [self._arg(name, i, a, ty) for i, (a, ty) in enumerate(zip(args, argtypes))]}
            self.trace.append(entry)
            return b'' if restype is ctypes.c_char_p else 0
        return fn

    def _pointer(self, value):
        value = getattr(value, 'value', value)
        if not value:
            return None
        slot = ['ptr', int(value)]
        self._pending.append(slot)
        return slot

    def _arg(self, fn, i, a, ty):
        if i == 0 and fn != 'mapf_create' and ty is ctypes.c_void_p and getattr(a, 'value', a) in self._handles:
            return 'handle %d' % self._handles[getattr(a, 'value', a)]
        if ty is ctypes.c_void_p:
            return self._pointer(a)
        if ty in _INTS:
            return int(a)
        if ty is ctypes.c_double:
            return float(a)
        obj = a._obj                                            # ctypes.byref(...)
        if isinstance(obj, nat.MapfDesc):
            return self._desc(obj)
        if isinstance(obj, nat.MapfRolloutIO):
            return {name: (self._pointer(getattr(obj, name)) if fty is ctypes.c_void_p else getattr(obj, name)) for name, fty in obj._fields_}
        if fn == 'mapf_create':                                 # the new handle
            obj.value = 0x1000 * (len(self._handles) + 1)
            self._handles[obj.value] = len(self._handles)
            return 'handle %d' % self._handles[obj.value]
        return 'out'                                            # a c_uint64 / c_void_p / c_double the library would fill

    @staticmethod
    def _desc(d):
        out = {}
        for name, fty in d._fields_:
            v = getattr(d, name)
            out[name] = (None if not v else 'ptr') if fty is ctypes.c_void_p else v
        n_start = (1 if d.flags & nat.MAPF_FLAG_START_BROADCAST else d.n_envs) * d.n_agents
        n_goal = (1 if d.flags & nat.MAPF_FLAG_GOAL_BROADCAST else d.n_envs) * d.n_agents
        for name, count in (('nbr', d.n_cells * 5), ('start', n_start), ('goal', n_goal)):
            out[name] = hashlib.sha1(ctypes.string_at(getattr(d, name), count * 2)).hexdigest()
        return out

    def watch(self, label, arrays):
        """Arrays the caller can see (name -> array, or one array): pointers into them are reported as (label, byte offset)."""
        if isinstance(arrays, np.ndarray):
            arrays = {'': arrays}
        for key, arr in arrays.items():
            if isinstance(arr, np.ndarray):
                while arr.base is not None and isinstance(arr.base, np.ndarray):
                    arr = arr.base
                self._watched.append(('%s.%s' % (label, key) if key else label, arr))

    def resolve(self):
        """After a step of the script: pointers become 'label+offset' or 'ptr'; the watch list starts over."""
        for slot in self._pending:
            p = slot[1]
            slot[:] = ['ptr']
            for label, arr in self._watched:
                base = arr.ctypes.data
                if base <= p < base + max(arr.nbytes, 1):
                    slot[:] = [label, p - base]
                    break
        self._pending, self._watched = [], []
