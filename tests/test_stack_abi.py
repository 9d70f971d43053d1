"""CPU tests of the observation stack (include/lcr.h: lcr_enable_obs_stack): the additions to the C ABI (declared, bound, exported; the ABI version and every existing struct
stay as they are), the refusals that need no device, VecSim's ValueErrors before any device call, the element formula for all 256 bytes, and the numpy model of the GPU tests
(tests/stack_ref.py) against two independent per-env restatements -- one in the style of gymnasium's FrameStackObservation(padding_type="reset"), one in the style of SB3's
VecFrameStack -- on synthetic frames with episode boundaries."""
import ctypes
import os
import re
from collections import deque
from fractions import Fraction

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import stack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_obs_stack_check", "lcr_enable_obs_stack", "lcr_get_obs_stack"]
CTYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "const void *": ctypes.c_void_p, "lcr_obs_stack_spec": _capi.ObsStackSpec}


def _parse_struct(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const void \*|int32_t|uint32_t|uint64_t|lcr_obs_stack_spec)\s*(.*)$", decl, flags=re.S)
        assert m, decl
        for nm in m.group(2).split(","):
            fields.append((re.match(r"\s*\*?\s*(\w+)", nm).group(1), CTYPES[m.group(1)]))
    return fields


def test_the_new_functions_are_declared_bound_and_exported(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"#define\s+LCR_STACK_MAX_FRAMES\s+8\b", hdr) and _capi.STACK_MAX_FRAMES == 8
    for name, val in (("LCR_STACK_CAM_FRONT", 1), ("LCR_STACK_CAM_TOP", 2), ("LCR_STACK_CAM_WRIST", 4), ("LCR_STACK_UINT8", 0), ("LCR_STACK_FLOAT16", 1),
                      ("LCR_STACK_FLOAT32", 2), ("LCR_STACK_FILL_REPEAT", 0), ("LCR_STACK_FILL_ZERO", 1)):
        assert re.search(name + r"\s*=\s*%d\b" % val, hdr), name
    assert _capi.STACK_CAMERAS == {"front": 1, "top": 2, "wrist": 4} and tuple(_capi.STACK_CAMERAS) == stack_ref.CAMERAS
    assert _capi.STACK_DTYPES == {"uint8": 0, "float16": 1, "float32": 2} and _capi.STACK_FILLS == {"repeat": 0, "zero": 1}


def test_the_existing_structs_are_unchanged(hip_lib):
    cfg = _capi.LcrConfig()
    assert hip_lib.lcr_config_default(ctypes.byref(cfg), 0) == 0
    assert cfg.struct_size == ctypes.sizeof(_capi.LcrConfig) == 200
    assert ctypes.sizeof(_capi.LcrObsView) == 64 and ctypes.sizeof(_capi.LcrPlanesView) == 48
    assert ctypes.sizeof(_capi.LookVariant) == 136 and ctypes.sizeof(_capi.LookSampler) == 80
    assert ctypes.sizeof(_capi.WristCamera) == 44 and ctypes.sizeof(_capi.LcrWristView) == 88


def test_stack_structs_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name, bound, size in (("lcr_obs_stack_spec", _capi.ObsStackSpec, 16), ("lcr_obs_stack_view", _capi.LcrObsStackView, 48)):
        fields = _parse_struct(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in bound._fields_] == [n for n, _ in fields], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)


def _spec(frames=4, cameras=0, dtype=0, reset_fill=0):
    return _capi.ObsStackSpec(frames=frames, cameras=cameras, dtype=dtype, reset_fill=reset_fill)


BAD = [("frames", dict(frames=0)), ("frames", dict(frames=9)), ("frames", dict(frames=-1)), ("cameras", dict(cameras=8)), ("cameras", dict(cameras=0x13)),
       ("dtype", dict(dtype=3)), ("dtype", dict(dtype=-1)), ("reset_fill", dict(reset_fill=2)), ("reset_fill", dict(reset_fill=-1))]


@pytest.mark.parametrize("field,over", BAD, ids=[f"{f}-{i}" for i, (f, _) in enumerate(BAD)])
def test_a_bad_spec_is_refused_before_the_handle_is_looked_at(hip_lib, field, over):
    assert hip_lib.lcr_obs_stack_check(ctypes.byref(_spec(**over))) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert msg.startswith(field.encode()), (field, msg)
    assert hip_lib.lcr_enable_obs_stack(None, ctypes.byref(_spec(**over))) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_last_error() == msg and b"sim is NULL" not in msg


def test_valid_specs_reach_the_handle_check_and_null_handles_are_refused(hip_lib):
    for sp in (_spec(), _spec(1, 1, 2, 1), _spec(8, 7, 1, 0), _spec(2, 4, 0, 1)):
        assert hip_lib.lcr_obs_stack_check(ctypes.byref(sp)) == 0
        assert hip_lib.lcr_enable_obs_stack(None, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_obs_stack_check(None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_enable_obs_stack(None, None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_get_obs_stack(None, None) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_get_obs_stack(None, ctypes.byref(_capi.LcrObsStackView())) == _capi.LCR_ERR_INVALID


def test_vecsim_checks_the_stack_before_device_use(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import VecSim

    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, obs_stack=4)
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, observation_mode="state", obs_stack={"frames": 2})
    for bad, what in ((0, "frames"), (9, "frames"), (True, "obs_stack must be"), ("4", "obs_stack must be"), (2.0, "obs_stack must be"), ({"frames": 2.5}, "frames"),
                      ({"frames": 2, "cameras": ("side",)}, "cameras"), ({"cameras": "front"}, "cameras"), ({"cameras": ()}, "cameras"), ({"dtype": "float64"}, "dtype"),
                      ({"dtype": "bfloat16"}, "dtype"), ({"reset_fill": "edge"}, "reset_fill"), ({"frames": 2, "depth": 3}, "unknown obs_stack fields"),
                      ({"cameras": ("front", "wrist")}, "wrist")):
        with pytest.raises(ValueError, match=what):
            VecSim("reach", 4, observation_mode="both", obs_stack=bad)
    # (valid values pass the checks: the constructor then goes on to lcr_create)
    for good in (1, 8, {"frames": 3, "cameras": ("top",), "dtype": np.float16, "reset_fill": "zero"}, {"dtype": "float32"}):
        with pytest.raises(AssertionError, match="lcr_create was reached"):
            VecSim("reach", 4, observation_mode="both", obs_stack=good)
    with pytest.raises(AssertionError, match="lcr_create was reached"):
        VecSim("reach", 4, observation_mode="image", wrist_camera=True, obs_stack={"cameras": ("wrist",)})
    sp = _capi.ObsStackSpec.from_any({"frames": 3, "cameras": ("wrist", "front"), "dtype": "float16", "reset_fill": "zero"})
    assert (sp.frames, sp.cameras, sp.dtype, sp.reset_fill) == (3, 5, 1, 1)
    assert sp.as_dict() == {"frames": 3, "cameras": ("front", "wrist"), "dtype": "float16", "reset_fill": "zero"}
    sp = _capi.ObsStackSpec.from_any(4)
    assert (sp.frames, sp.cameras, sp.dtype, sp.reset_fill) == (4, 0, 0, 0)


def test_the_float_elements_of_all_256_bytes():
    """float32: one correctly rounded fp32 multiply by the fp32 constant 1 / 255, checked against exact rational arithmetic; float16: that value rounded to nearest even.  For
    these 256 products rounding the exact product straight to float16 gives the same bits, so a fused multiply-and-convert cannot differ either"""
    x = np.arange(256, dtype=np.uint8)
    c = stack_ref.INV255
    assert c.dtype == np.float32 and c.view(np.uint32) == 0x3B808081
    f32, f16 = stack_ref.convert(x, np.float32), stack_ref.convert(x, np.float16)
    assert f32.dtype == np.float32 and f16.dtype == np.float16 and stack_ref.convert(x, np.uint8).dtype == np.uint8
    np.testing.assert_array_equal(stack_ref.convert(x, "uint8"), x)
    np.testing.assert_array_equal(f32.view(np.uint32), (np.float32(1) * x.astype(np.float32) * np.float32(1 / 255)).view(np.uint32))
    assert f32[0] == 0 and f32[255] == 1 and f16[0] == 0 and f16[255] == 1 and (np.diff(f32) > 0).all() and (np.diff(f16.astype(np.float32)) >= 0).all()
    for i in range(256):
        exact = Fraction(i) * Fraction(float(c))                       # the exact product of the two fp32 numbers
        lo, hi = np.nextafter(f32[i], np.float32(-1)), np.nextafter(f32[i], np.float32(2))
        err = abs(Fraction(float(f32[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i   # correctly rounded
        assert f16[i].view(np.uint16) == np.float16(f32[i]).view(np.uint16)
        assert f16[i].view(np.uint16) == np.float16(np.float64(i) * np.float64(c)).view(np.uint16), i   # (the fp64 product is exact: 8 + 24 bits)
    # not the division: x / 255 in fp32 differs from the multiply for some bytes, which is why the contract names the multiply
    assert (f32.view(np.uint32) != (x.astype(np.float32) / np.float32(255)).view(np.uint32)).any()


# ---- the model against two per-env restatements ----

def _episodes(rng, n, T, C, H, W, p_done=0.3):
    """synthetic rollout: frames[t] (n, C, H, W) uint8 AFTER step t (the reset-state frames where done[t]), first[.] the frames of the initial reset"""
    first = rng.integers(0, 256, (n, C, H, W), dtype=np.uint8)
    frames = rng.integers(0, 256, (T, n, C, H, W), dtype=np.uint8)
    done = rng.random((T, n)) < p_done
    done[:, 0] = False            # an env that never finishes
    done[:, 1] = True             # ... and one that finishes every step
    return first, frames, done


def _gymnasium_style(first, frames, done, K, e):
    """one env, a deque per episode as FrameStackObservation(padding_type="reset") keeps it: reset() fills all K places with the reset observation, step() appends"""
    out = []
    q = deque([first[e]] * K, maxlen=K)
    for t in range(frames.shape[0]):
        if done[t, e]:            # the vector env has auto-reset: frames[t] is the reset observation of the new episode
            q = deque([frames[t, e]] * K, maxlen=K)
        else:
            q.append(frames[t, e])
        out.append(np.stack(list(q)))
    return out


def _sb3_style(first, frames, done, K, e):
    """one env of VecFrameStack (StackedObservations, channels-first): reset() zeros the stack and writes the observation last; step_wait() rolls by one observation,
    zeros the stack of an env that is done, and writes the new observation last"""
    C = first.shape[1]
    st = np.zeros((K * C,) + first.shape[2:], np.uint8)
    st[-C:] = first[e]
    out = []
    for t in range(frames.shape[0]):
        st = np.roll(st, -C, axis=0)
        if done[t, e]:
            st[...] = 0
        st[-C:] = frames[t, e]
        out.append(st.reshape((K, C) + first.shape[2:]).copy())
    return out


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_model_against_the_gymnasium_and_sb3_restatements(K):
    rng = np.random.default_rng(K)
    n, T, H, W = 6, 14, 4, 8
    cams = 2
    first, frames, done = _episodes(rng, n, T, 3 * cams, H, W)

    def as_cameras(x):   # (n, C, H, W) -> the cameras' (n, H, W, 3) frames the model is fed
        return [np.ascontiguousarray(np.moveaxis(x[:, 3 * c:3 * c + 3], 1, -1)) for c in range(cams)]

    np.testing.assert_array_equal(stack_ref.channels_first(as_cameras(first)), first)
    m = stack_ref.StackRef(as_cameras(first), K)
    np.testing.assert_array_equal(m.expected("uint8", "repeat"), np.repeat(first[:, None], K, axis=1))
    if K > 1:
        assert not m.expected("uint8", "zero")[:, :-1].any()
    gy = [_gymnasium_style(first, frames, done, K, e) for e in range(n)]
    sb = [_sb3_style(first, frames, done, K, e) for e in range(n)]
    for t in range(T):
        m.step(as_cameras(frames[t]), done[t])
        np.testing.assert_array_equal(m.expected("uint8", "repeat"), np.stack([gy[e][t] for e in range(n)]), err_msg=f"gymnasium style, step {t}")
        np.testing.assert_array_equal(m.expected("uint8", "zero"), np.stack([sb[e][t] for e in range(n)]), err_msg=f"SB3 style, step {t}")
        for dt in ("float16", "float32"):
            got = m.expected(dt, "zero")
            assert got.dtype == np.dtype(dt) and got.shape == (n, K, 3 * cams, H, W)
            np.testing.assert_array_equal(got, stack_ref.convert(np.stack([sb[e][t] for e in range(n)]), dt))


def test_model_reset_and_set_look_rules():
    rng = np.random.default_rng(3)
    n, K = 5, 3
    f = lambda: [rng.integers(0, 256, (n, 4, 4, 3), dtype=np.uint8)]   # noqa: E731
    a, b, c, d = f(), f(), f(), f()
    m = stack_ref.StackRef(a, K)
    m.step(b, np.zeros(n, bool))
    before = {fill: m.expected("uint8", fill).copy() for fill in stack_ref.FILLS}
    mask = np.array([1, 0, 0, 1, 0], np.uint8)
    m.reset(c, mask)
    xc = stack_ref.channels_first(c)
    for fill in stack_ref.FILLS:
        s = m.expected("uint8", fill)
        np.testing.assert_array_equal(s[:, -1], xc)                                    # the invariant
        np.testing.assert_array_equal(s[mask == 0, :-1], before[fill][mask == 0, :-1])   # no time has passed for the unmasked envs
        np.testing.assert_array_equal(s[mask == 1, :-1], np.repeat(xc[mask == 1, None], K - 1, 1) if fill == "repeat" else 0)
    before = {fill: m.expected("uint8", fill).copy() for fill in stack_ref.FILLS}
    m.set_look(d)
    for fill in stack_ref.FILLS:
        s = m.expected("uint8", fill)
        np.testing.assert_array_equal(s[:, -1], stack_ref.channels_first(d)); np.testing.assert_array_equal(s[:, :-1], before[fill][:, :-1])
    m.reset(a)   # no mask: all
    np.testing.assert_array_equal(m.expected("uint8", "repeat"), np.repeat(stack_ref.channels_first(a)[:, None], K, 1))
