"""CPU tests of the terminal observation stacks (include/lcr.h: lcr_enable_obs_stack_terminal, lcr_get_obs_stack_terminal, lcr_obs_stack_terminal): the additions to the C ABI
(declared, bound, exported; the ABI version and every existing struct stay as they are), the order of the checks that need no device -- spec, then keep_terminal, then the
handle --, VecSim's ValueErrors for `terminal` before any device call, what the vector adapters accept, and the routing of ShardedVecSim's terminal calls by env id."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_enable_obs_stack_terminal", "lcr_get_obs_stack_terminal", "lcr_obs_stack_terminal"]


def _spec(frames=4, cameras=0, dtype=0, reset_fill=0):
    return _capi.ObsStackSpec(frames=frames, cameras=cameras, dtype=dtype, reset_fill=reset_fill)


def test_the_new_functions_are_declared_bound_and_exported(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    # the header says what the stack now keeps on request, and what it still does not
    assert "Terminal observation stacks" in hdr and "ONLY step refills save" in hdr and "terminal history of the depth and segmentation planes" in hdr
    assert "so there is no stacked terminal observation" not in hdr


def test_the_existing_structs_are_unchanged(hip_lib):
    cfg = _capi.LcrConfig()
    assert hip_lib.lcr_config_default(ctypes.byref(cfg), 0) == 0
    assert cfg.struct_size == ctypes.sizeof(_capi.LcrConfig) == 200
    assert ctypes.sizeof(_capi.LcrObsView) == 64 and ctypes.sizeof(_capi.LcrPlanesView) == 48
    assert ctypes.sizeof(_capi.LookVariant) == 136 and ctypes.sizeof(_capi.LookSampler) == 80
    assert ctypes.sizeof(_capi.WristCamera) == 44 and ctypes.sizeof(_capi.LcrWristView) == 88
    assert ctypes.sizeof(_capi.ObsStackSpec) == 16 and ctypes.sizeof(_capi.LcrObsStackView) == 48
    assert ctypes.sizeof(_capi.PointCloudSpec) == 16 and ctypes.sizeof(_capi.LcrPointCloudView) == 80
    assert ctypes.sizeof(_capi.PointCloudSampling) == 8 and ctypes.sizeof(_capi.PointCloudCrop) == 24


BAD_SPEC = [("frames", dict(frames=0)), ("cameras", dict(cameras=8)), ("dtype", dict(dtype=3)), ("reset_fill", dict(reset_fill=2))]


@pytest.mark.parametrize("field,over", BAD_SPEC, ids=[f for f, _ in BAD_SPEC])
@pytest.mark.parametrize("keep", [0, 1, 7])
def test_the_spec_is_checked_first(hip_lib, field, over, keep):
    """a bad spec is refused under its field's name whatever keep_terminal and the handle are"""
    assert hip_lib.lcr_enable_obs_stack_terminal(None, ctypes.byref(_spec(**over)), keep) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert msg.startswith(field.encode()) and b"keep_terminal" not in msg and b"sim is NULL" not in msg, msg
    assert hip_lib.lcr_enable_obs_stack_terminal(None, None, keep) == _capi.LCR_ERR_INVALID and b"spec is NULL" in hip_lib.lcr_last_error()


@pytest.mark.parametrize("keep", [2, -1, 255, 1 << 30])
def test_keep_terminal_is_checked_before_the_handle(hip_lib, keep):
    assert hip_lib.lcr_enable_obs_stack_terminal(None, ctypes.byref(_spec()), keep) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert msg.startswith(b"keep_terminal") and str(keep).encode() in msg and b"sim is NULL" not in msg, msg


def test_valid_arguments_reach_the_handle_check_and_null_handles_are_refused(hip_lib):
    for sp in (_spec(), _spec(1, 1, 2, 1), _spec(8, 7, 1, 0)):
        for keep in (0, 1):
            assert hip_lib.lcr_enable_obs_stack_terminal(None, ctypes.byref(sp), keep) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()
    keep, hist, nbytes = ctypes.c_int32(5), ctypes.c_void_p(1), ctypes.c_uint64(9)
    assert hip_lib.lcr_get_obs_stack_terminal(None, ctypes.byref(keep), ctypes.byref(hist), ctypes.byref(nbytes)) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_get_obs_stack_terminal(None, None, None, None) == _capi.LCR_ERR_INVALID
    ids, out = np.zeros(1, np.int32), np.zeros(16, np.uint8)
    assert hip_lib.lcr_obs_stack_terminal(None, ids.ctypes.data_as(ctypes.c_void_p), 1, out.ctypes.data_as(ctypes.c_void_p)) == _capi.LCR_ERR_INVALID
    assert b"sim is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_obs_stack_terminal(None, None, 0, None) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()


def _guarded(hip_lib, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())


def test_vecsim_checks_terminal_before_device_use(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import VecSim

    _guarded(hip_lib, monkeypatch)
    for bad in (1, 0, "yes", None, 1.0, [True]):
        with pytest.raises(ValueError, match="obs_stack: terminal must be a bool"):
            VecSim("reach", 4, observation_mode="both", obs_stack={"frames": 2, "terminal": bad})
    # the other fields are checked as before, with or without terminal; unknown fields stay refused
    for bad, what in (({"frames": 9, "terminal": True}, "frames"), ({"dtype": "float64", "terminal": False}, "dtype"), ({"frames": 2, "terminal": True, "depth": 3}, "unknown obs_stack fields"),
                      ({"frames": 2, "keep_terminal": True}, "unknown obs_stack fields"), ({"terminal": True, "cameras": ("front", "wrist")}, "wrist")):
        with pytest.raises(ValueError, match=what):
            VecSim("reach", 4, observation_mode="both", obs_stack=bad)
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, obs_stack={"frames": 2, "terminal": True})
    for good in ({"frames": 4, "terminal": True}, {"terminal": np.bool_(True)}, {"frames": 1, "terminal": True, "dtype": "float16"}, {"frames": 3, "terminal": False}):
        with pytest.raises(AssertionError, match="lcr_create was reached"):
            VecSim("reach", 4, observation_mode="both", obs_stack=good)
    assert _capi.take_terminal({"frames": 4, "terminal": True}, "obs_stack") == ({"frames": 4}, True)
    assert _capi.take_terminal({"frames": 4}, "obs_stack") == ({"frames": 4}, False) and _capi.take_terminal(4, "obs_stack") == (4, False)


def test_the_adapters_accept_a_terminal_stack(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, LowCostRobotVectorEnv

    _guarded(hip_lib, monkeypatch)
    for cls in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        for stack in ({"frames": 4, "terminal": True}, 4, {"frames": 2}):   # (without terminal a stack is accepted too, and not exposed)
            with pytest.raises(AssertionError, match="lcr_create was reached"):
                cls("reach", 4, observation_mode="both", obs_stack=stack)
        with pytest.raises(ValueError, match="obs_stack: terminal must be a bool"):
            cls("reach", 4, observation_mode="both", obs_stack={"frames": 4, "terminal": 1})


def test_sharded_terminal_calls_are_routed_by_env_id():
    """ShardedVecSim hands every shard its own envs' local ids and puts the answers back in the order of env_ids"""
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    class Arr:
        def __init__(self, shape, dtype=np.float32):
            self.shape, self.dtype = shape, np.dtype(dtype)

    class Shard:
        def __init__(self, g):
            self.g, self.calls = g, []
            self.obs_stack = Arr((64, 2, 3, 1, 1), np.uint8)
            self.point_cloud, self.point_cloud_source, self.point_cloud_pose = Arr((64, 4, 3)), Arr((64, 4), np.int32), Arr((2, 13, 64))

        def obs_stack_terminal(self, local):
            self.calls.append(local.copy())
            return np.broadcast_to((100 * self.g + local).astype(np.uint8)[:, None, None, None, None], (local.size, 2, 3, 1, 1))

        def point_cloud_terminal(self, local):
            v = (1000 * self.g + local).astype(np.float32)
            return {"point_cloud": np.broadcast_to(v[:, None, None], (local.size, 4, 3)), "count": v.astype(np.int32), "source": np.broadcast_to(v.astype(np.int32)[:, None], (local.size, 4)),
                    "pose": np.broadcast_to(v[None, None, :], (2, 13, local.size))}

    sh = object.__new__(ShardedVecSim)
    sh.per, sh.n, sh.shards = 64, 128, [Shard(0), Shard(1)]
    ids = np.array([70, 3, 127, 64, 0, 63])
    want = np.array([106, 3, 163, 100, 0, 63])
    got = sh.obs_stack_terminal(ids)
    assert got.shape == (6, 2, 3, 1, 1) and got.dtype == np.uint8
    np.testing.assert_array_equal(got[:, 0, 0, 0, 0], want)
    np.testing.assert_array_equal(sh.shards[0].calls[0], [3, 0, 63]); np.testing.assert_array_equal(sh.shards[1].calls[0], [6, 63, 0])
    assert sh.shards[1].calls[0].dtype == np.int32
    want = np.array([1006, 3, 1063, 1000, 0, 63])
    pc = sh.point_cloud_terminal(ids)
    np.testing.assert_array_equal(pc["point_cloud"][:, 1, 2], want); np.testing.assert_array_equal(pc["count"], want)
    np.testing.assert_array_equal(pc["source"][:, 3], want); np.testing.assert_array_equal(pc["pose"][1, 12], want)
    assert pc["pose"].shape == (2, 13, 6) and sh.obs_stack_terminal(np.zeros(0, np.int32)).shape == (0, 2, 3, 1, 1)
