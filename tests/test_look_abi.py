"""CPU tests of the look of the image observations (visual domain randomisation; include/lcr.h: lcr_enable_look): the four additions to the C ABI (declared, bound,
exported; the ABI version and lcr_config stay as they are), the default variant, the refusals that need no device, and the reference of the look itself
(tests/look_ref.py) -- tied to the committed colour oracle byte for byte at the default look, and run in fp32 against fp64 for the variants of the GPU tests.

The fp32 twin against fp64 for look_ref.GPU_VARIANTS (8 seed-17 states of test_gpu_image_size._random_poses, per-env colours of the GPU test; push, stack, pick_place; both
cameras): worst pixels beyond +-2 levels per frame -- 84 x 84: 2 (allowed 26.9), 120 x 160: 8 (allowed 38.4).  The variants by themselves do not use up the pixel bound
of the GPU test (test_gpu_image_size._oracle_pixels, imported, not restated)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import look_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_look_variant_default", "lcr_enable_look", "lcr_set_look", "lcr_get_look"]
CAMS = ("camera_front", "camera_top")
VARIANT_FIELDS = ["cam_dpos", "cam_drot", "fovy_deg", "floor_rgb", "sky_rgb", "sky_slope", "ambient", "diffuse", "arm_rgb", "finger_rgb"]


def _states(task, n):
    from tests.test_gpu_image_size import _random_poses

    nq = 20 if task == "stack" else 13
    return _random_poses(task, n, np.random.default_rng(17), {"qpos": np.zeros((nq, n))})


def _parse_struct(hdr, name):
    """[(field, ctypes type)] of a struct of floats / uint64_t in include/lcr.h"""
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(float|uint64_t)\s+(.*)$", decl, flags=re.S)
        assert m, decl
        base = {"float": ctypes.c_float, "uint64_t": ctypes.c_uint64}[m.group(1)]
        for nm in m.group(2).split(","):
            dims = [int(d) for d in re.findall(r"\[(\d+)\]", nm)]
            t = base
            for d in reversed(dims):
                t = t * d
            fields.append((re.match(r"\s*(\w+)", nm).group(1), t))
    return fields


def test_the_four_functions_are_declared_bound_and_exported(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"#define\s+LCR_LOOK_MAX_VARIANTS\s+64\b", hdr) and _capi.LOOK_MAX_VARIANTS == 64


def test_lcr_config_is_unchanged(hip_lib):
    cfg = _capi.LcrConfig()
    assert hip_lib.lcr_config_default(ctypes.byref(cfg), 0) == 0
    assert cfg.struct_size == ctypes.sizeof(_capi.LcrConfig) == 200
    assert [n for n, _ in _capi.LcrConfig._fields_][-2:] == ["image_width", "image_height"]


def test_look_structs_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name, bound, size in (("lcr_look_variant", _capi.LookVariant, 136), ("lcr_look_sampler", _capi.LookSampler, 80)):
        fields = _parse_struct(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in bound._fields_] == [n for n, _ in fields], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)
    assert [n for n, _ in _capi.LookVariant._fields_] == VARIANT_FIELDS


def test_default_variant_has_the_documented_values(hip_lib):
    import gym_lowcostrobot_amd

    v = _capi.LookVariant()
    ctypes.memset(ctypes.byref(v), 0xFF, ctypes.sizeof(v))
    assert hip_lib.lcr_look_variant_default(ctypes.byref(v)) == 0
    got, want = v.as_dict(), look_ref.default_variant()
    assert sorted(got) == sorted(want) == sorted(VARIANT_FIELDS)
    for k in VARIANT_FIELDS:
        np.testing.assert_array_equal(np.asarray(got[k], np.float32), np.asarray(want[k], np.float32), err_msg=k)
    assert hip_lib.lcr_look_variant_default(None) == _capi.LCR_ERR_INVALID
    assert bytes(gym_lowcostrobot_amd.default_look_variant()) == bytes(v)
    assert look_ref.TASK_RGB == _capi.LOOK_TASK_RGB


def _variants(k=1):
    arr = (_capi.LookVariant * k)()
    for i in range(k):
        assert _capi.load().lcr_look_variant_default(ctypes.byref(arr[i])) == 0
    return arr


def _set(v, field, idx, val):
    f = getattr(v, field)
    if idx == ():
        setattr(v, field, val)
    elif len(idx) == 1:
        f[idx[0]] = val
    else:
        f[idx[0]][idx[1]] = val


BAD_FIELDS = [("cam_dpos", (0, 1), [0.25, -0.3, math.nan]), ("cam_dpos", (1, 2), [math.inf]), ("cam_drot", (1, 0), [0.6, -0.51, math.nan]), ("fovy_deg", (0,), [19.0, 91.0, math.nan]),
              ("fovy_deg", (1,), [0.0]), ("floor_rgb", (1, 2), [-0.01, 1.01, math.inf]), ("sky_rgb", (0,), [1.5, math.nan]), ("sky_slope", (2,), [-1.0]),
              ("ambient", (), [-0.1, 1.6, math.nan]), ("diffuse", (), [1.51, -math.inf]), ("arm_rgb", (1,), [2.0]), ("finger_rgb", (2,), [-0.5, math.nan])]


def test_enable_refuses_bad_arguments_before_it_looks_at_the_handle(hip_lib):
    f = hip_lib.lcr_enable_look

    def refused(nv, arr, sampler, word):
        assert f(None, nv, arr, sampler) == _capi.LCR_ERR_INVALID
        msg = hip_lib.lcr_last_error()
        assert word in msg and b"sim is NULL" not in msg, (word, msg)

    for k in (0, -1, 65):
        refused(k, _variants(1), None, b"n_variants")
    refused(1, None, None, b"variants_host")
    for field, idx, values in BAD_FIELDS:
        for val in values:
            arr = _variants(3)
            _set(arr[2], field, idx, val)          # (the last of three: every variant is checked)
            refused(3, arr, None, field.encode())
    arr = _variants(1)
    arr[0].cam_drot[0][0] = arr[0].cam_drot[0][1] = arr[0].cam_drot[0][2] = 0.3   # each component is small enough, the vector is 0.52 rad long
    refused(1, arr, None, b"cam_drot")
    for grp in ("cube", "cube2", "marker"):
        for end, val in (("lo", -0.1), ("hi", 1.2), ("lo", math.nan), ("hi", math.inf)):
            sm = _capi.LookSampler.from_any({"seed": 1})
            getattr(sm, f"{grp}_{end}")[1] = val
            refused(1, _variants(1), ctypes.byref(sm), f"{grp}_{end}".encode())
        sm = _capi.LookSampler.from_any({"seed": 1, grp: ([0.5, 0.5, 0.5], [0.6, 0.4, 0.6])})   # lo > hi in one channel
        refused(1, _variants(1), ctypes.byref(sm), f"{grp}_lo".encode())
    # valid arguments: now the handle is looked at
    sm = _capi.LookSampler.from_any({"seed": 1, "cube": ([0, 0, 0], [1, 1, 1])})
    for sampler in (None, ctypes.byref(sm)):
        assert f(None, 64, _variants(64), sampler) == _capi.LCR_ERR_INVALID
        assert b"sim is NULL" in hip_lib.lcr_last_error()


def test_null_handles_are_refused_by_all_four(hip_lib):
    assert hip_lib.lcr_enable_look(None, 1, _variants(1), None) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_set_look(None, None, None, None) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_get_look(None, None, None, None) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_look_variant_default(None) == _capi.LCR_ERR_INVALID


def test_vecsim_refuses_a_look_without_frames_before_device_use(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import VecSim

    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, look_variants=[{}])
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, observation_mode="state", look_sampler={"seed": 3})
    with pytest.raises(ValueError, match="unknown look variant field"):
        VecSim("reach", 4, observation_mode="both", look_variants=[{"fov": 30.0}])
    with pytest.raises(ValueError, match="unknown look sampler"):
        VecSim("reach", 4, observation_mode="both", look_sampler={"seed": 3, "cubes": ([0] * 3, [1] * 3)})


@pytest.mark.parametrize("size", [(84, 84), (240, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", ["push", "stack", "reach"])
def test_default_look_is_the_colour_oracle_byte_for_byte(task, size):
    from oracle import render_oracle

    H, W = size
    qpos, target = _states(task, 4)
    for e in range(4):
        for cam in CAMS:
            ref = render_oracle.render(task, qpos[:, e], target[:, e], cam, W, H)
            got = look_ref.render(task, qpos[:, e], target[:, e], cam, W, H)
            np.testing.assert_array_equal(got, ref, err_msg=f"{task} {size} env {e} {cam}")
            # the planes through an unmoved camera are the planes reference's
            from tests import planes_ref

            d, s = look_ref.planes(task, qpos[:, e], target[:, e], cam, W, H)
            dr, sr = planes_ref.planes(task, qpos[:, e], target[:, e], cam, W, H)
            np.testing.assert_array_equal(d, dr); np.testing.assert_array_equal(s, sr)


def gpu_test_colours(n):
    """the explicit per-env colours of the GPU test against look_ref: (9, n) float32, seed 23"""
    return np.random.default_rng(23).uniform(0.05, 0.95, (9, n)).astype(np.float32)


@pytest.mark.parametrize("size", [(84, 84), (120, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", ["push", "stack", "pick_place"])
def test_fp32_twin_of_the_gpu_variants_stays_within_the_pixel_bound(task, size):
    """the variants of the GPU test must not by themselves break its bound: the reference in fp32 against fp64, same states, variants and colours"""
    from tests.test_gpu_image_size import _oracle_pixels

    H, W = size
    n = 8
    qpos, target = _states(task, n)
    rgb = gpu_test_colours(n)
    worst = 0
    for e in range(n):
        v = look_ref.GPU_VARIANTS[e % len(look_ref.GPU_VARIANTS)]
        for cam in CAMS:
            a = look_ref.render(task, qpos[:, e], target[:, e], cam, W, H, v=v, rgb=rgb[:, e]).astype(int)
            b = look_ref.render(task, qpos[:, e], target[:, e], cam, W, H, v=v, rgb=rgb[:, e], dtype=np.float32).astype(int)
            assert a.std() > 5
            bad = int((np.abs(a - b).max(-1) > 2).sum())
            worst = max(worst, bad)
            assert bad <= _oracle_pixels(H, W), (task, size, e, cam, bad, np.argwhere(np.abs(a - b).max(-1) > 2)[:5].tolist())
    print(f"[look fp32 twin] {task} {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_oracle_pixels(H, W):.1f})")


def test_sampler_reference_is_uniform_and_keyed():
    lo, hi = np.array([0.1] * 3 + [0.0] * 3 + [0.5, 0.5, 0.5], np.float32), np.array([0.9] * 3 + [1.0] * 3 + [0.5, 0.6, 0.5], np.float32)
    draws = [look_ref.sample(7, g, ep, 5, lo, hi) for g in range(200) for ep in range(3)]
    var = np.array([d[0] for d in draws]); rgb = np.stack([d[1] for d in draws])
    assert set(var) == set(range(5)) and (rgb >= lo).all() and (rgb <= hi).all() and rgb.dtype == np.float32
    assert (rgb[:, 6] == 0.5).all() and (rgb[:, 8] == 0.5).all() and 0.45 < rgb[:, 0].mean() < 0.55
    assert look_ref.sample(7, 11, 2, 5, lo, hi)[0] == draws[11 * 3 + 2][0] and np.array_equal(look_ref.sample(7, 11, 2, 5, lo, hi)[1], draws[11 * 3 + 2][1])
    assert not np.array_equal(look_ref.sample(8, 11, 2, 5, lo, hi)[1], draws[11 * 3 + 2][1])
