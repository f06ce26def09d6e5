"""The argument checks of the Python layer (vec_env.checked_ptr / array_ptr / coerce_array, and the VecMapfEnv methods that
delegate to them), on the CPU: what is refused, with which words -- the texts are the ones callers have always seen."""
import numpy as np
import pytest

from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs.grid import MapfGrid
from gym_mapf_amd.envs.vec_env import OptimizationCriteria, VecMapfEnv, array_ptr, checked_ptr, coerce_array
from native_recorder import Recorder


def test_host_mode_output_arrays_are_checked_not_converted():
    good = np.zeros((2, 3), np.uint8)
    assert array_ptr(None, good, np.uint8, (2, 3), 'done') == good.ctypes.data == checked_ptr(None, good, np.uint8, (2, 3), 'done')
    assert array_ptr(None, None, np.uint8, (2, 3), 'done') is None
    for bad in (np.zeros((2, 3), np.uint16),                       # wrong dtype
                np.zeros((3, 2), np.uint8),                        # wrong shape
                np.zeros((2, 6), np.uint8)[:, ::2],                # a non-contiguous view of the right shape
                np.zeros((3, 2), np.uint8).T,                      # (Fortran order)
                [[0, 0, 0], [0, 0, 0]]):                           # a list cannot receive results
        with pytest.raises(ValueError) as err:
            array_ptr(None, bad, np.uint8, (2, 3), 'done')
        assert str(err.value) == 'done must be a C-contiguous uint8 array of shape (2, 3)'
    with pytest.raises(ValueError) as err:
        checked_ptr(None, np.zeros(4, np.float32), np.float64, [4], 'reward')
    assert str(err.value) == 'reward must be a C-contiguous float64 array of shape (4,)'
    with pytest.raises(ValueError) as err:
        checked_ptr(None, None, np.uint64, (5,), 'offset')
    assert str(err.value) == 'offset must be a C-contiguous uint64 array of shape (5,)'


def test_host_mode_inputs_are_converted_and_their_shape_checked():
    got = coerce_array(None, [[1, 2, 3], [4, 0, 1]], np.uint8, (2, 3), 'actions')
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.flags.c_contiguous and got.tolist() == [[1, 2, 3], [4, 0, 1]]
    wide = np.arange(12, dtype=np.int64).reshape(2, 6)[:, ::2]
    got = coerce_array(None, wide, np.uint16, (2, 3), 'local')
    assert got.dtype == np.uint16 and got.flags.c_contiguous and np.array_equal(got, wide)
    same = np.zeros((2, 3), np.float64)
    assert coerce_array(None, same, np.float64, (2, 3), 'uniforms') is same          # nothing to do: no copy
    assert coerce_array(None, None, np.float64, (2, 3), 'uniforms') is None
    with pytest.raises(ValueError) as err:
        coerce_array(None, np.zeros((3, 2)), np.float64, (2, 3), 'uniforms')
    assert str(err.value) == 'uniforms must have shape (2, 3), got (3, 2)'
    with pytest.raises(ValueError) as err:
        coerce_array(None, [1, 2, 3], np.uint8, (1, 3), 'actions')
    assert str(err.value) == 'actions must have shape (1, 3), got (3,)'


def test_device_mode_takes_contiguous_cuda_tensors_only():
    torch = pytest.importorskip('torch')
    cpu = torch.zeros((2, 3), dtype=torch.uint8)
    for bad in (cpu, cpu.t(), torch.zeros((2, 6), dtype=torch.uint8)[:, ::2], np.zeros((2, 3), np.uint8)):
        with pytest.raises(ValueError) as err:
            array_ptr(torch, bad, np.uint8, (2, 3), 'actions')
        assert str(err.value) == 'actions must be a contiguous CUDA torch.uint8 tensor of shape (2, 3)'
    with pytest.raises(ValueError) as err:
        checked_ptr(torch, torch.zeros(4, dtype=torch.float32), np.float64, (4,), 'prob')
    assert str(err.value) == 'prob must be a contiguous CUDA torch.float64 tensor of shape (4,)'
    assert array_ptr(torch, None, np.uint32, (4,), 'env_index') is None
    assert coerce_array(torch, cpu, np.uint8, (9, 9), 'actions') is cpu             # device mode converts nothing: array_ptr refuses it


def test_the_env_methods_delegate_with_their_old_signatures(monkeypatch):
    monkeypatch.setattr(nat, 'load', lambda: Recorder())
    env = VecMapfEnv(MapfGrid(['....', '....']), 2, ((0, 0), (1, 3)), ((1, 0), (0, 3)), 0.2, -1.0, 1.0, -1.0, OptimizationCriteria.SoC, n_envs=3)
    arr = env._empty((3, 2), np.uint16)
    assert isinstance(arr, np.ndarray) and arr.shape == (3, 2) and arr.dtype == np.uint16
    assert env._ptr(arr, np.uint16, (3, 2), 'local') == arr.ctypes.data and env._ptr(None, np.uint16, (3, 2), 'local') is None
    assert env._coerce([[0, 1], [2, 3], [4, 0]], np.uint8, (3, 2), 'actions').dtype == np.uint8
    with pytest.raises(ValueError) as err:
        env.step(np.zeros((3, 2), np.uint8), out={'reward': np.zeros(3, np.float32)})
    assert str(err.value) == 'reward must be a C-contiguous float64 array of shape (3,)'
    with pytest.raises(ValueError) as err:
        env.step(np.zeros((2, 3), np.uint8))
    assert str(err.value) == 'actions must have shape (3, 2), got (2, 3)'
    with pytest.raises(ValueError) as err:
        env.rollout(4, actions=np.zeros((4, 3, 2), np.uint8), out={}, accumulate_into={})
    assert str(err.value) == 'pass either out= (overwrite) or accumulate_into= (add), not both'
    with pytest.raises(KeyError):
        env.transitions(np.zeros((1, 2), np.uint16), np.zeros((1, 2), np.uint8), out={'count': np.zeros(1, np.uint32)})   # (an out dict is complete)
    env.close()
