"""CPU tests of the wrist camera (include/lcr.h: lcr_enable_wrist_camera): the four additions to the C ABI (declared, bound, exported; the ABI version and lcr_config stay
as they are), the default mount, the refusals that need no device, and the reference itself (tests/wrist_ref.py) -- tied to the committed colour oracle byte for byte
through a world-frame mount with a scene camera's pose, checked for the floor rule, and run in fp32 against fp64 for the states and mounts of the GPU tests.

The fp32 twin against fp64 (8 seed-17 states of test_gpu_image_size._random_poses; push, stack, pick_place), worst pixels beyond +-2 levels per frame:
  default mount (link 5)          84 x 84: 1 (allowed 26.9)    36 x 52: 1 (allowed 11.5)    120 x 160: 5 (allowed 38.4)
  second mount (link 4, fovy 90)  84 x 84: 3                   36 x 52: 1                   120 x 160: 6
The mounts by themselves do not use up the pixel bound of the GPU test (test_gpu_image_size._oracle_pixels, imported, not restated)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import look_ref, planes_ref, wrist_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_wrist_camera_default", "lcr_wrist_camera_check", "lcr_enable_wrist_camera", "lcr_get_wrist_camera", "lcr_render_terminal_wrist"]
CTYPES = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "lcr_wrist_camera": _capi.WristCamera, "const uint8_t *": ctypes.c_void_p, "const float *": ctypes.c_void_p}


def _states(task, n=8):
    from tests.test_gpu_image_size import _random_poses

    nq = 20 if task == "stack" else 13
    return _random_poses(task, n, np.random.default_rng(17), {"qpos": np.zeros((nq, n))})


def _parse_struct(hdr, name):
    """[(field, ctypes type)] of a struct of include/lcr.h made of int32_t, float, pointers and lcr_wrist_camera"""
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const uint8_t \*|const float \*|int32_t|float|lcr_wrist_camera)\s*(.*)$", decl, flags=re.S)
        assert m, decl
        base = CTYPES[m.group(1)]
        for nm in m.group(2).split(","):
            dims = [int(d) for d in re.findall(r"\[(\d+)\]", nm)]
            t = base
            for d in reversed(dims):
                t = t * d
            fields.append((re.match(r"\s*\*?\s*(\w+)", nm).group(1), t))
    return fields


def test_the_new_functions_are_declared_bound_and_exported(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"#define\s+LCR_WRIST_GUARD\s+4096\b", hdr) and _capi.WRIST_GUARD == 4096
    assert re.search(r"#define\s+LCR_WRIST_GUARD_BYTE\s+0xA5\b", hdr) and _capi.WRIST_GUARD_BYTE == 0xA5


def test_lcr_config_and_the_existing_views_are_unchanged(hip_lib):
    cfg = _capi.LcrConfig()
    assert hip_lib.lcr_config_default(ctypes.byref(cfg), 0) == 0
    assert cfg.struct_size == ctypes.sizeof(_capi.LcrConfig) == 200
    assert [n for n, _ in _capi.LcrConfig._fields_][-2:] == ["image_width", "image_height"]
    assert ctypes.sizeof(_capi.LcrObsView) == 64 and ctypes.sizeof(_capi.LcrPlanesView) == 48
    assert ctypes.sizeof(_capi.LookVariant) == 136 and ctypes.sizeof(_capi.LookSampler) == 80


def test_wrist_structs_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name, bound, size in (("lcr_wrist_camera", _capi.WristCamera, 44), ("lcr_wrist_view", _capi.LcrWristView, 88)):
        fields = _parse_struct(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in bound._fields_] == [n for n, _ in fields], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)


def test_default_mount_has_the_documented_values(hip_lib):
    import gym_lowcostrobot_amd

    c = _capi.WristCamera()
    ctypes.memset(ctypes.byref(c), 0xFF, ctypes.sizeof(c))
    assert hip_lib.lcr_wrist_camera_default(ctypes.byref(c)) == 0
    want = wrist_ref.default_mount()
    assert c.link == want["link"] == 5
    np.testing.assert_array_equal(np.array(c.pos, np.float32), np.array([0.03, 0.0033, 0.045], np.float32))
    np.testing.assert_array_equal(np.array(c.xyaxes, np.float32), np.array([0, 1, 0, -0.4226, 0, 0.9063], np.float32))
    np.testing.assert_array_equal(np.array(c.pos, np.float64), want["pos"]); np.testing.assert_array_equal(np.array(c.xyaxes, np.float64), want["xyaxes"])
    assert c.fovy_deg == want["fovy_deg"] == 60.0
    assert hip_lib.lcr_wrist_camera_default(None) == _capi.LCR_ERR_INVALID
    assert gym_lowcostrobot_amd.default_wrist_camera() == c.as_dict()
    # 25 degrees down along the link's -x: the optical axis -Z
    X, Y, Z = wrist_ref.axes(want)
    assert abs(np.degrees(np.arctan2(Z[2], Z[0])) - 25.0) < 0.01 and abs(Z[1]) < 1e-7


def _cam(**over):
    c = _capi.WristCamera()
    assert _capi.load().lcr_wrist_camera_default(ctypes.byref(c)) == 0
    for k, v in over.items():
        if k in ("link", "fovy_deg"):
            setattr(c, k, v)
        else:
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
    return c


BAD = [("link", dict(link=7)), ("link", dict(link=-1)),
       ("xyaxes", dict(xyaxes=(0, 0, 0, 0, 1, 0))),                    # a zero X
       ("xyaxes", dict(xyaxes=(1, 2, 3, -2, -4, -6))),                 # Y parallel to X
       ("xyaxes", dict(xyaxes=(1, 0, 0, 1, 1e-7, 0))),                 # ... to within 1e-6 after the projection
       ("fovy_deg", dict(fovy_deg=10.0)), ("fovy_deg", dict(fovy_deg=130.0)), ("fovy_deg", dict(fovy_deg=math.nan)),
       ("xyaxes", dict(xyaxes=(0, 1, 0, math.nan, 0, 1))), ("xyaxes", dict(xyaxes=(math.inf, 1, 0, 0, 0, 1))),
       ("pos", dict(pos=(0.0, math.nan, 0.0))), ("pos", dict(pos=(0.6, 0.0, 0.0))), ("pos", dict(pos=(0.0, 0.0, -0.51))),
       ("pos", dict(link=0, pos=(0.0, 2.5, 0.3))), ("pos", dict(link=0, pos=(0.1, 0.4, 0.04))), ("pos", dict(link=0, pos=(0.1, 0.4, -0.2)))]


@pytest.mark.parametrize("field,over", BAD, ids=[f"{f}-{i}" for i, (f, _) in enumerate(BAD)])
def test_enable_refuses_a_bad_mount_before_it_looks_at_the_handle(hip_lib, field, over):
    assert hip_lib.lcr_enable_wrist_camera(None, ctypes.byref(_cam(**over))) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert field.encode() in msg and b"sim is NULL" not in msg, (field, msg)
    assert hip_lib.lcr_wrist_camera_check(ctypes.byref(_cam(**over))) == _capi.LCR_ERR_INVALID and hip_lib.lcr_last_error() == msg


def test_valid_mounts_reach_the_handle_check_and_null_handles_are_refused(hip_lib):
    for c in (_cam(), _cam(link=0, pos=(1.9, -2.0, 0.05)), _cam(link=6, pos=(0.5, -0.5, 0.5), fovy_deg=120.0), _cam(link=1, fovy_deg=20.0, xyaxes=(0, 0, 5, 1e-3, 0, 7))):
        assert hip_lib.lcr_enable_wrist_camera(None, ctypes.byref(c)) == _capi.LCR_ERR_INVALID
        assert b"sim is NULL" in hip_lib.lcr_last_error()
        assert hip_lib.lcr_wrist_camera_check(ctypes.byref(c)) == 0
    assert hip_lib.lcr_wrist_camera_check(None) == _capi.LCR_ERR_INVALID and b"cam is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_enable_wrist_camera(None, None) == _capi.LCR_ERR_INVALID and b"cam is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_get_wrist_camera(None, None) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_get_wrist_camera(None, ctypes.byref(_capi.LcrWristView())) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_render_terminal_wrist(None, None, 0, None, None, None) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()


def test_vecsim_checks_the_mount_before_device_use(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import VecSim

    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, wrist_camera=True)
    with pytest.raises(ValueError, match="unknown wrist camera fields"):
        VecSim("reach", 4, observation_mode="both", wrist_camera={"fov": 30.0})
    with pytest.raises(ValueError, match="fovy_deg"):
        VecSim("reach", 4, observation_mode="both", wrist_camera={"fovy_deg": 150.0})
    with pytest.raises(ValueError, match="link"):
        VecSim("reach", 4, observation_mode="both", wrist_camera={"link": 9})
    with pytest.raises(ValueError, match="xyaxes"):
        VecSim("reach", 4, observation_mode="both", wrist_camera={"xyaxes": (1, 0, 0, 2, 0, 0)})
    with pytest.raises(ValueError, match="xyaxes takes 6"):
        VecSim("reach", 4, observation_mode="both", wrist_camera={"xyaxes": (1, 0, 0)})
    with pytest.raises(ValueError, match="wrist_camera must be"):
        VecSim("reach", 4, observation_mode="both", wrist_camera="link_5")


@pytest.mark.parametrize("size", [(84, 84), (240, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", ["push", "stack", "reach"])
def test_a_world_mount_at_a_scene_camera_is_the_colour_oracle_byte_for_byte(task, size):
    from oracle import render_oracle
    from tests.test_gpu_image_size import _oracle_pixels

    H, W = size
    qpos, target = _states(task, 4)
    for cam in ("camera_front", "camera_top"):
        m = wrist_ref.scene_camera_mount(task, cam)
        for e in range(4):
            ref = render_oracle.render(task, qpos[:, e], target[:, e], cam, W, H)
            got = wrist_ref.render(task, qpos[:, e], target[:, e], m, W, H, exact=True)
            np.testing.assert_array_equal(got, ref, err_msg=f"{task} {size} env {e} {cam}")
            d, s = wrist_ref.planes(task, qpos[:, e], target[:, e], m, W, H, exact=True)
            dr, sr = planes_ref.planes(task, qpos[:, e], target[:, e], cam, W, H)
            np.testing.assert_array_equal(d, dr); np.testing.assert_array_equal(s, sr)
            # the same mount as the library receives it (float32 numbers, float32 axes): the same picture but for pixels on an fp32 edge -- the project's bound for those
            got32 = wrist_ref.render(task, qpos[:, e], target[:, e], wrist_ref.mount(0, m["pos"], m["xyaxes"], 45.0), W, H)
            assert int((np.abs(got32.astype(int) - ref.astype(int)).max(-1) > 2).sum()) <= _oracle_pixels(H, W)



def test_a_camera_below_the_floor_draws_no_floor_and_still_the_boxes():
    """state 0 of the GPU test's poses puts the default mount at z = -0.015: the floor rule.  Without it (tests/look_ref.render's rule through the same camera) the negative
    floor parameter hides every box"""
    task = "stack"
    qpos, target = _states(task)
    m = wrist_ref.default_mount()
    ro = wrist_ref.camera(m, qpos[:, 0])[0]
    assert -0.02 < ro[2] < -0.01, ro
    H, W = 84, 84
    img = wrist_ref.render(task, qpos[:, 0], None, m, W, H)
    d, s = wrist_ref.planes(task, qpos[:, 0], None, m, W, H, depth_far=10.0)
    ids = s & 0x7F
    assert not (ids == planes_ref.ID_FLOOR).any()
    assert (ids >= planes_ref.ID_ARM0).sum() > 50 and (ids == planes_ref.ID_SKY).sum() > 50     # boxes are seen, and so is what lies behind them
    assert (d[ids == planes_ref.ID_SKY] == 10.0).all() and (d[ids >= planes_ref.ID_ARM0] < 1.0).all()
    v = look_ref.default_variant()
    sky_px = img[ids == planes_ref.ID_SKY].astype(int)
    lo, hi = np.rint(255 * v["sky_rgb"]).astype(int), np.rint(255 * (v["sky_rgb"] + v["sky_slope"])).astype(int)
    assert (sky_px >= lo).all() and (sky_px <= hi).all()
    # rays that point down from below the floor: a = 0, the plain sky colour
    pos, X, Y, Z = wrist_ref.camera(m, qpos[:, 0])
    sc = wrist_ref._scale(m, H, False)
    vv, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dz = ((u + 0.5 - 0.5 * W) * sc)[..., None] * X + (-(vv + 0.5 - 0.5 * H) * sc)[..., None] * Y - Z
    downsky = (dz[..., 2] < -1e-3) & (ids == planes_ref.ID_SKY)
    assert downsky.sum() > 20 and (img[downsky] == lo).all()
    # a state with the camera above the floor does see it
    e = next(i for i in range(8) if wrist_ref.camera(m, qpos[:, i])[0][2] > 0.05)
    assert ((wrist_ref.planes(task, qpos[:, e], None, m, W, H)[1] & 0x7F) == planes_ref.ID_FLOOR).any()


@pytest.mark.parametrize("size", [(84, 84), (36, 52), (120, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("which", ["default", "other"])
@pytest.mark.parametrize("task", ["push", "stack", "pick_place"])
def test_fp32_twin_of_the_gpu_mounts_stays_within_the_pixel_bound(task, which, size):
    """the states and mounts of the GPU test must not by themselves break its bound: the reference in fp32 against fp64"""
    from tests.test_gpu_image_size import _oracle_pixels

    H, W = size
    m = wrist_ref.default_mount() if which == "default" else wrist_ref.OTHER_MOUNT
    qpos, target = _states(task)
    worst = 0
    for e in range(8):
        a = wrist_ref.render(task, qpos[:, e], target[:, e], m, W, H).astype(int)
        b = wrist_ref.render(task, qpos[:, e], target[:, e], m, W, H, dtype=np.float32).astype(int)
        assert a.std() > 5, (task, which, e, a.std())
        bad = int((np.abs(a - b).max(-1) > 2).sum())
        worst = max(worst, bad)
        assert bad <= _oracle_pixels(H, W), (task, which, size, e, bad, np.argwhere(np.abs(a - b).max(-1) > 2)[:5].tolist())
    print(f"[wrist fp32 twin] {task} {which} {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_oracle_pixels(H, W):.1f})")
