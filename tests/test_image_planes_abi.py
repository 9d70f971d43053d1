"""CPU tests of the depth / segmentation planes of the image observations: the five additions to the C ABI (declared, bound, exported; the ABI version and the
existing structs stay as they are), the refusals of lcr_enable_image_planes and of VecSim that need no device, and the reference of the planes itself
(tests/planes_ref.py) -- tied to the committed colour oracle by its visibility classes, and run in fp32 against fp64.

The figures of the reference checks (8 seed-17 states of test_gpu_image_size._random_poses, four tasks, two cameras): the visibility class of the reference's id equals
the class implied by the oracle's colour at every pixel without the marker bit; the fp32 twin has no segmentation mismatch in any frame and a worst relative depth
deviation of 1.3e-6 (asserted below: <= 1e-5, a hundred fp32 roundings of a chain of about ten operations -- the 1e-4 the GPU test allows is 10x that)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import planes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_enable_image_planes", "lcr_get_image_planes", "lcr_render_planes", "lcr_render_state_planes", "lcr_render_terminal_planes"]
TASKS = ["push", "stack", "pick_place", "reach"]
CAMS = ("camera_front", "camera_top")


def _states(task, n=8):
    """the states of test_sized_frames_vs_cpu_raycaster (seed 17); the poses overwrite every row of qpos, so zeros stand in for the sim's state"""
    from tests.test_gpu_image_size import _random_poses

    nq = 20 if task == "stack" else 13
    return _random_poses(task, n, np.random.default_rng(17), {"qpos": np.zeros((nq, n))})


def test_the_five_functions_are_declared_bound_and_exported(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"LCR_PLANE_DEPTH\s*=\s*1\b", hdr) and re.search(r"LCR_PLANE_SEGMENTATION\s*=\s*2\b", hdr)
    assert (_capi.PLANE_DEPTH, _capi.PLANE_SEGMENTATION) == (1, 2)


def test_planes_view_binding_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    body = hdr[hdr.index("typedef struct lcr_planes_view {"):hdr.index("} lcr_planes_view;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(uint32_t|int32_t|float|uint8_t)\s+(.*)$", decl, flags=re.S)
        assert m, decl
        for nm in m.group(3).split(","):
            nm = nm.strip()
            ctype = ctypes.c_void_p if nm.startswith("*") else {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}[m.group(2)]
            fields.append((nm.lstrip("* "), ctype))
    assert [n for n, _ in fields] == ["planes", "image_width", "image_height", "depth_far", "depth_front", "depth_top", "seg_front", "seg_top"]
    Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(Parsed) == ctypes.sizeof(_capi.LcrPlanesView) == 48
    assert [n for n, _ in _capi.LcrPlanesView._fields_] == [n for n, _ in fields]
    for n, _ in fields:
        assert getattr(Parsed, n).offset == getattr(_capi.LcrPlanesView, n).offset, n


def test_enable_refuses_bad_arguments_before_it_looks_at_the_handle(hip_lib):
    f = hip_lib.lcr_enable_image_planes
    for planes in (0, 4, 7):
        assert f(None, planes, 10.0) == _capi.LCR_ERR_INVALID
        assert b"planes" in hip_lib.lcr_last_error() and b"sim is NULL" not in hip_lib.lcr_last_error(), hip_lib.lcr_last_error()
    for far in (0.0, -1.0, math.nan, math.inf, 2000.0):
        assert f(None, 3, far) == _capi.LCR_ERR_INVALID
        assert b"depth_far" in hip_lib.lcr_last_error() and b"sim is NULL" not in hip_lib.lcr_last_error(), hip_lib.lcr_last_error()
    for planes in (1, 2, 3):
        assert f(None, planes, 10.0) == _capi.LCR_ERR_INVALID
        assert b"sim is NULL" in hip_lib.lcr_last_error()
    pv = _capi.LcrPlanesView()
    assert hip_lib.lcr_get_image_planes(None, ctypes.byref(pv)) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_render_planes(None, 0, 0, 64, 64, None, None) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_render_state_planes(None, 0, 64, 64, None, None, None, None) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_render_terminal_planes(None, None, 0, None, None, None, None) == _capi.LCR_ERR_INVALID


def test_vecsim_refuses_bad_planes_before_device_use(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import VecSim

    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:   # the loaded library with lcr_create replaced: the refusals below must come before it is asked for a device
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())
    with pytest.raises(ValueError, match="image_planes"):
        VecSim("reach", 4, observation_mode="both", image_planes=("depth", "normals"))
    with pytest.raises(ValueError, match="image_planes"):
        VecSim("reach", 4, observation_mode="both", image_planes="depth")          # a tuple of names, not a name
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, observation_mode="state", image_planes=("depth",))
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, image_planes=("segmentation",))                         # (VecSim's default mode is "state")
    for far in (0.0, -1.0, math.nan, math.inf, 2000.0, "far"):
        with pytest.raises(ValueError, match="depth_far"):
            VecSim("reach", 4, observation_mode="both", image_planes=("depth",), depth_far=far)
    with pytest.raises(ValueError, match="depth_far"):
        VecSim("reach", 4, observation_mode="both", depth_far=-1.0)                # checked with no plane asked for as well


@pytest.mark.parametrize("size", [(84, 84), (240, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", TASKS)
def test_reference_visibility_classes_equal_the_colour_oracle(task, size):
    """the id class of the reference (floor / sky, arm, red cube, blue cube) equals the class implied by the colours of oracle.render_oracle.render at every pixel
    without the marker bit"""
    from oracle import render_oracle

    H, W = size
    qpos, target = _states(task)
    seen = np.zeros(4, int)
    for e in range(qpos.shape[1]):
        for cam in CAMS:
            depth, seg = planes_ref.planes(task, qpos[:, e], target[:, e], cam, W, H)
            rgb = render_oracle.render(task, qpos[:, e], target[:, e], cam, W, H)
            plain = (seg & planes_ref.MARKER_BIT) == 0
            a, b = planes_ref.id_class(seg), planes_ref.rgb_class(rgb)
            assert int(((a != b) & plain).sum()) == 0, (task, size, e, cam, np.argwhere((a != b) & plain)[:5].tolist())
            seen += np.bincount(a[plain], minlength=4)
            assert depth.dtype == np.float32 and seg.dtype == np.uint8 and (depth > 0).all() and (depth <= 10.0).all()
            assert ((seg == 0) <= (depth == 10.0)).all()
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and (seen[3] > 0) == (task == "stack")


@pytest.mark.parametrize("size", [(84, 84), (240, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", TASKS)
def test_fp32_twin_of_the_reference(task, size):
    """the same ray arithmetic in fp32: no segmentation mismatch in any frame, depth within 1e-5 relative; the far clip and the marker bit are exercised"""
    H, W = size
    qpos, target = _states(task)
    worst, clipped, marked, nearest = 0.0, 0, 0, np.inf
    for e in range(qpos.shape[1]):
        for cam in CAMS:
            d64, s64 = planes_ref.planes(task, qpos[:, e], target[:, e], cam, W, H)
            d32, s32 = planes_ref.planes(task, qpos[:, e], target[:, e], cam, W, H, dtype=np.float32)
            assert int((s64 != s32).sum()) == 0, (task, size, e, cam, np.argwhere(s64 != s32)[:5].tolist())
            worst = max(worst, float((np.abs(d32.astype(float) - d64) / d64).max()))
            clipped += int((d64 == 10.0).sum()); marked += int((s64 & planes_ref.MARKER_BIT != 0).sum()); nearest = min(nearest, float(d64.min()))
    print(f"[fp32 twin] {task} {H}x{W}: worst relative depth deviation {worst:.2e}, nearest {nearest:.3f} m, {clipped} pixels at the far clip, {marked} under the marker")
    assert worst <= 1e-5
    assert clipped > 0 and 0.05 < nearest < 1.0
    assert (marked > 0) == (task in ("push", "pick_place"))
