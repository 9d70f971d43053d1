"""CPU tests of the depth channel of the observation stack (include/lcr.h: lcr_enable_obs_stack_planes, lcr_get_obs_stack_planes): the additions to the C ABI (declared,
bound, exported; the ABI version and the stack's structs stay as they are), the order of the checks that need no device -- spec, keep_terminal, planes, then the handle --,
VecSim's and the adapters' ValueErrors for `planes` before any device call, and the numpy model of the element rule (tests/stack_depth_ref.py) against exact rational
arithmetic with one rounding per stated operation."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import stack_depth_ref as ref
from tests.cloud_fps_ref import round_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_enable_obs_stack_planes", "lcr_get_obs_stack_planes"]


def _spec(frames=4, cameras=0, dtype=0, reset_fill=0):
    return _capi.ObsStackSpec(frames=frames, cameras=cameras, dtype=dtype, reset_fill=reset_fill)


def test_the_new_functions_are_declared_bound_and_exported(hip_lib):
    """1.  (fails without the feature: neither function exists)"""
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    assert ctypes.sizeof(_capi.ObsStackSpec) == 16 and ctypes.sizeof(_capi.LcrObsStackView) == 48
    # the header defines the channel and says what is not in it
    assert "The depth channel of the observation stack" in hdr and "fmaf(d, s255, 0.5f)" in hdr and "fminf(d * inv_far, 1.0f)" in hdr
    for phrase in ("a segmentation channel", "normalisation by mean and std", "a depth-only stack without colours", "per-camera depth_far", "the recorder"):
        assert phrase in hdr, phrase


def test_null_handle_and_null_spec_are_refused(hip_lib):
    """2.  valid arguments reach the handle check; the getter refuses NULL arguments"""
    for planes in (0, 1):
        for keep in (0, 1):
            assert hip_lib.lcr_enable_obs_stack_planes(None, ctypes.byref(_spec()), keep, planes) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()
            assert hip_lib.lcr_enable_obs_stack_planes(None, None, keep, planes) == _capi.LCR_ERR_INVALID and b"spec is NULL" in hip_lib.lcr_last_error()
    p, a, b = ctypes.c_uint32(9), ctypes.c_float(1), ctypes.c_float(1)
    assert hip_lib.lcr_get_obs_stack_planes(None, ctypes.byref(p), ctypes.byref(a), ctypes.byref(b)) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_get_obs_stack_planes(None, None, None, None) == _capi.LCR_ERR_INVALID


@pytest.mark.parametrize("planes,code,word", [(2, _capi.LCR_ERR_UNSUPPORTED, b"segmentation"), (3, _capi.LCR_ERR_UNSUPPORTED, b"segmentation"), (4, _capi.LCR_ERR_INVALID, b"planes"),
                                              (8, _capi.LCR_ERR_INVALID, b"planes"), (5, _capi.LCR_ERR_INVALID, b"planes"), (1 << 31, _capi.LCR_ERR_INVALID, b"planes")])
def test_bad_planes_masks_are_refused_before_the_handle(hip_lib, planes, code, word):
    """2.  the segmentation bit is unsupported, named in the message; unknown bits are invalid; both before the handle is looked at"""
    assert hip_lib.lcr_enable_obs_stack_planes(None, ctypes.byref(_spec()), 1, planes) == code
    msg = hip_lib.lcr_last_error()
    assert word in msg and b"sim is NULL" not in msg, msg


def test_the_order_of_the_checks(hip_lib):
    """2.  spec, then keep_terminal, then planes, then the handle"""
    assert hip_lib.lcr_enable_obs_stack_planes(None, ctypes.byref(_spec(frames=0)), 7, 2) == _capi.LCR_ERR_INVALID and hip_lib.lcr_last_error().startswith(b"frames")
    assert hip_lib.lcr_enable_obs_stack_planes(None, ctypes.byref(_spec()), 7, 2) == _capi.LCR_ERR_INVALID and hip_lib.lcr_last_error().startswith(b"keep_terminal")
    assert hip_lib.lcr_enable_obs_stack_planes(None, ctypes.byref(_spec()), 0, 2) == _capi.LCR_ERR_UNSUPPORTED
    assert hip_lib.lcr_enable_obs_stack_planes(None, ctypes.byref(_spec()), 0, 16) == _capi.LCR_ERR_INVALID and b"sim is NULL" not in hip_lib.lcr_last_error()


def _guarded(hip_lib, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())


BAD_PLANES = [
    (dict(planes=("depth",)), dict(), "image_planes"),                                                   # the depth plane is not switched on silently
    (dict(planes=("depth",)), dict(image_planes=("segmentation",)), "image_planes"),
    (dict(planes=("segmentation",)), dict(image_planes=("depth", "segmentation")), "unsupported"),
    (dict(planes=("depth", "segmentation")), dict(image_planes=("depth", "segmentation")), "unsupported"),
    (dict(planes=("normals",)), dict(image_planes=("depth",)), "unknown names"),
    (dict(planes="depth"), dict(image_planes=("depth",)), "tuple or list"),
    (dict(planes=1), dict(image_planes=("depth",)), "tuple or list"),
    (dict(planes=None), dict(image_planes=("depth",)), "tuple or list"),
    (dict(planes=(1,)), dict(image_planes=("depth",)), "tuple or list"),
    (dict(planes={"depth"}), dict(image_planes=("depth",)), "tuple or list"),
]


def _classes():
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, LowCostRobotVectorEnv, VecSim

    return VecSim, LowCostRobotVecEnv, LowCostRobotVectorEnv


@pytest.mark.parametrize("which", [0, 1, 2], ids=["VecSim", "VecEnv", "VectorEnv"])
def test_planes_is_checked_before_device_use(hip_lib, monkeypatch, which):
    """3.  every bad `planes` value is a ValueError before lcr_create; `depth` as a key stays an unknown field; good values reach lcr_create"""
    cls = _classes()[which]
    _guarded(hip_lib, monkeypatch)
    for stack, more, what in BAD_PLANES:
        for terminal in (False, True):
            with pytest.raises(ValueError, match="obs_stack: planes.*" + what):
                cls("reach", 4, observation_mode="both", obs_stack=dict(frames=2, terminal=terminal, **stack), **more)
    with pytest.raises(ValueError, match="unknown obs_stack fields"):
        cls("reach", 4, observation_mode="both", image_planes=("depth",), obs_stack={"frames": 2, "depth": 3})
    with pytest.raises(ValueError, match="unknown obs_stack fields"):
        cls("reach", 4, observation_mode="both", image_planes=("depth",), obs_stack={"frames": 2, "planes": ("depth",), "depth": 3})
    with pytest.raises(ValueError, match="frames"):
        cls("reach", 4, observation_mode="both", image_planes=("depth",), obs_stack={"frames": 9, "planes": ("depth",)})
    for stack, more in ((dict(frames=4, planes=("depth",)), dict(image_planes=("depth",))), (dict(frames=4, planes=["depth"], terminal=True), dict(image_planes=("depth", "segmentation"))),
                        (dict(frames=2, planes=()), dict()), (dict(frames=2, planes=[], terminal=True), dict(image_planes=("depth",)))):
        with pytest.raises(AssertionError, match="lcr_create was reached"):
            cls("reach", 4, observation_mode="both", obs_stack=stack, **more)
    assert _capi.take_stack_planes({"frames": 4, "planes": ("depth",)}, ("depth",)) == ({"frames": 4}, _capi.PLANE_DEPTH)
    assert _capi.take_stack_planes({"frames": 4}, ()) == ({"frames": 4}, 0) and _capi.take_stack_planes(4, ()) == (4, 0)


# ---- 4.  the model of the element rule against exact rational arithmetic ----

def _round_f16(x):
    """a Fraction -> the nearest float16, ties to even"""
    if x == 0:
        return np.float16(0.0)
    r = np.float16(float(x))
    best = None
    for c in (np.nextafter(r, np.float16(-np.inf)), r, np.nextafter(r, np.float16(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - x)
        even = (int(np.asarray(c, np.float16).view(np.uint16)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, c, even)
    return np.float16(best[1])


def _exact(d, inv_far, s255):
    """the header's three elements of one depth, in Fractions with one rounding per stated operation -> (uint8, float16 bits, float32 bits)"""
    D = Fraction(float(d))
    m = round_f32(D * Fraction(float(inv_far)))                     # one rounded float32 multiply
    m = np.float32(1.0) if Fraction(float(m)) > 1 else m            # fminf(., 1.0f)
    h = _round_f16(Fraction(float(m)))                              # that float32 value rounded to nearest even
    t = round_f32(D * Fraction(float(s255)) + Fraction(1, 2))       # ONE fused multiply-add
    u = min(int(Fraction(float(t))), 255)                           # truncation toward zero (t >= 0), then the clamp
    return u, int(np.asarray(h).view(np.uint16)), int(np.asarray(m, np.float32).view(np.uint32))


def _inputs(depth_far):
    far = np.float32(depth_far)
    _, s255 = ref.constants(depth_far)
    edges = (np.arange(255, dtype=np.float64) + 0.5) / np.float64(s255)   # where the uint8 element steps from k to k + 1
    e32 = edges.astype(np.float32)
    near = np.concatenate([np.nextafter(e32, np.float32(-np.inf)), e32, np.nextafter(e32, np.float32(np.inf)),
                           np.nextafter(np.nextafter(e32, np.float32(-np.inf)), np.float32(-np.inf)), np.nextafter(np.nextafter(e32, np.float32(np.inf)), np.float32(np.inf))])
    rng = np.random.default_rng(int(float(far) * 1000))
    rnd = (rng.random(3000) * float(far)).astype(np.float32)
    d = np.concatenate([np.array([0.0, far], np.float32), near.astype(np.float32), rnd])
    return d[(d >= 0) & (d <= far)]


@pytest.mark.parametrize("depth_far", [10.0, 0.7, 1.3, 0.3])
def test_the_model_is_the_exact_rule(depth_far):
    """4.  all three element types at 0, depth_far, the float32 neighbours of every uint8 step (k + 0.5) / s255 and 3000 random depths: the numpy model -- whose uint8
    rule forms d s255 + 0.5 in float64 and rounds once more -- gives the bits of the exact chain, so it equals the fused operation on these inputs"""
    inv_far, s255 = ref.constants(depth_far)
    far64 = float(np.float32(depth_far))
    assert inv_far.dtype == np.float32 and s255.dtype == np.float32
    assert Fraction(float(inv_far)) == Fraction(float(round_f32(1 / Fraction(far64)))) and Fraction(float(s255)) == Fraction(float(round_f32(255 / Fraction(far64))))
    d = _inputs(depth_far)
    assert d.size > 3700 and d[0] == 0 and d[1] == np.float32(depth_far)
    exact = np.array([_exact(x, inv_far, s255) for x in d], np.int64)
    u8, f16, f32 = (ref.depth_elements(d, t, depth_far) for t in ("uint8", "float16", "float32"))
    assert u8.dtype == np.uint8 and f16.dtype == np.float16 and f32.dtype == np.float32
    np.testing.assert_array_equal(u8.astype(np.int64), exact[:, 0])
    np.testing.assert_array_equal(f16.view(np.uint16).astype(np.int64), exact[:, 1])
    np.testing.assert_array_equal(f32.view(np.uint32).astype(np.int64), exact[:, 2])
    # what the inputs reach: both ends of every type, every uint8 value, and both sides of every step
    assert u8[0] == 0 and u8[1] == 255 and f32[0] == 0 and f32[1] <= 1 and f32.max() <= 1 and set(u8.tolist()) == set(range(256))
    assert not f16[0].view(np.uint16) and not f32[0].view(np.uint32)   # d = 0 is zero bits: a zero refill of the raw depths is a zero refill of the elements


def test_the_model_interleaves_r_g_b_d_per_camera():
    """the four-channel slot semantics: cameras in order, each r, g, b, d; the depth moves with the colours; a zero refill is zero bits in the depth channel too"""
    rng = np.random.default_rng(0)
    N, H, W, K, far = 5, 2, 8, 3, 0.5

    def draw():
        return [rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8) for _ in range(2)], [(rng.random((N, H, W)) * far).astype(np.float32) for _ in range(2)]

    fr, dp = draw()
    m = ref.StackDepthRef(fr, dp, K, far)
    first = ref.rgbd_elements(fr, dp, "float16", far)
    assert first.shape == (N, 8, H, W)
    for fill in ref.FILLS:
        got = m.expected("float16", fill)
        assert got.shape == (N, K, 8, H, W) and (got[:, -1].view(np.uint16) == first.view(np.uint16)).all()
        assert (got[:, 0].view(np.uint16) == (first.view(np.uint16) if fill == "repeat" else 0)).all()
    np.testing.assert_array_equal(first[:, 3], ref.depth_elements(dp[0], "float16", far)); np.testing.assert_array_equal(first[:, 7], ref.depth_elements(dp[1], "float16", far))
    np.testing.assert_array_equal(first[:, 4:7], (np.moveaxis(fr[1], -1, 1).astype(np.float32) * np.float32(1 / 255)).astype(np.float16))
    fr2, dp2 = draw()
    did = np.array([0, 1, 0, 0, 1], bool)
    m.step(fr2, dp2, did)
    second = ref.rgbd_elements(fr2, dp2, "uint8", far)
    for fill in ref.FILLS:
        got = m.expected("uint8", fill)
        np.testing.assert_array_equal(got[:, -1], second)
        np.testing.assert_array_equal(got[~did, -2], ref.rgbd_elements(fr, dp, "uint8", far)[~did])
        np.testing.assert_array_equal(got[did, 0], second[did] if fill == "repeat" else np.zeros_like(second[did]))
