"""CPU tests of the point cloud's farthest-point sampling (include/lcr.h: lcr_enable_point_cloud_sampled): the additions to the C ABI (declared, bound, exported; the ABI
version and the cloud's structs stay as they are), the refusals that need no device, VecSim's ValueErrors before any device call, and the numpy model the GPU tests compare
against (tests/cloud_fps_ref.py) held to a brute-force greedy in exact rational arithmetic."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import cloud_fps_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_point_cloud_sampling_check", "lcr_enable_point_cloud_sampled", "lcr_get_point_cloud_sampling"]
STRIDE, FPS = 0, 1


def _hdr():
    return open(os.path.join(ROOT, "include", "lcr.h")).read()


def test_the_new_functions_are_declared_bound_and_exported(hip_lib):
    hdr = _hdr()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"enum\s*\{\s*LCR_CLOUD_SAMPLE_STRIDE\s*=\s*0\s*,\s*LCR_CLOUD_SAMPLE_FPS\s*=\s*1\s*\}", hdr)
    assert re.search(r"#define\s+LCR_CLOUD_MAX_POOL\s+4096\b", hdr) and _capi.CLOUD_MAX_POOL == 4096
    assert _capi.CLOUD_SAMPLINGS == {"stride": STRIDE, "fps": FPS}
    for what in ("a crop box", "random sampling", "normals", "pools beyond 4096", "FPS over colours"):
        assert what in hdr, what   # the header says what the mode still does not do


def test_the_sampling_struct_matches_the_header_and_the_cloud_structs_keep_their_sizes():
    hdr = _hdr()
    body = hdr[hdr.index("typedef struct lcr_point_cloud_sampling {"):hdr.index("} lcr_point_cloud_sampling;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.match(r"\s*int32_t\s+(\w+)\s*$", decl)
            assert m, decl
            fields.append((m.group(1), ctypes.c_int32))
    Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(Parsed) == ctypes.sizeof(_capi.PointCloudSampling) == 8
    assert [n for n, _ in fields] == [n for n, _ in _capi.PointCloudSampling._fields_] == ["mode", "pool"]
    for n, _ in fields:
        assert getattr(Parsed, n).offset == getattr(_capi.PointCloudSampling, n).offset and getattr(Parsed, n).size == getattr(_capi.PointCloudSampling, n).size == 4
    assert ctypes.sizeof(_capi.PointCloudSpec) == 16 and ctypes.sizeof(_capi.LcrPointCloudView) == 80


def _spec(points=64):
    return _capi.PointCloudSpec(points=points, cameras=0, ids=0, colors=0)


def _sampling(mode, pool):
    return _capi.PointCloudSampling(mode=mode, pool=pool)


# (field the message starts with, points, mode, pool)
BAD = [("mode", 64, 2, 0), ("mode", 64, -1, 0), ("pool", 64, STRIDE, 64), ("pool", 64, FPS, 0), ("pool", 64, FPS, 100), ("pool", 64, FPS, 4160), ("pool", 256, FPS, 192),
       ("pool", 8192, FPS, 4096)]


@pytest.mark.parametrize("field,points,mode,pool", BAD, ids=[f"{f}-P{p}-mode{m}-pool{q}" for f, p, m, q in BAD])
def test_a_bad_sampling_is_refused_before_the_handle_is_looked_at(hip_lib, field, points, mode, pool):
    sp, sm = _spec(points), _sampling(mode, pool)
    assert hip_lib.lcr_point_cloud_check(ctypes.byref(sp)) == 0   # the spec itself is fine
    assert hip_lib.lcr_point_cloud_sampling_check(ctypes.byref(sp), ctypes.byref(sm)) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert msg.startswith(field.encode()), (field, msg)
    assert hip_lib.lcr_enable_point_cloud_sampled(None, ctypes.byref(sp), ctypes.byref(sm)) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_last_error() == msg and b"sim is NULL" not in msg


def test_valid_samplings_reach_the_handle_check_and_null_arguments_are_refused(hip_lib):
    L = hip_lib
    for points, mode, pool in ((64, STRIDE, 0), (8192, STRIDE, 0), (64, FPS, 64), (64, FPS, 4096), (4096, FPS, 4096), (512, FPS, 2048), (128, FPS, 320)):
        sp, sm = _spec(points), _sampling(mode, pool)
        assert L.lcr_point_cloud_sampling_check(ctypes.byref(sp), ctypes.byref(sm)) == 0
        assert L.lcr_enable_point_cloud_sampled(None, ctypes.byref(sp), ctypes.byref(sm)) == _capi.LCR_ERR_INVALID and b"sim is NULL" in L.lcr_last_error()
    assert L.lcr_enable_point_cloud_sampled(None, ctypes.byref(_spec()), None) == _capi.LCR_ERR_INVALID and b"sim is NULL" in L.lcr_last_error()   # NULL: stride
    # the spec is checked first, then the sampling
    assert L.lcr_enable_point_cloud_sampled(None, ctypes.byref(_spec(100)), ctypes.byref(_sampling(2, 0))) == _capi.LCR_ERR_INVALID
    assert L.lcr_last_error().startswith(b"points")
    assert L.lcr_enable_point_cloud_sampled(None, None, None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in L.lcr_last_error()
    assert L.lcr_point_cloud_sampling_check(None, ctypes.byref(_sampling(STRIDE, 0))) == _capi.LCR_ERR_INVALID and b"spec is NULL" in L.lcr_last_error()
    assert L.lcr_point_cloud_sampling_check(ctypes.byref(_spec()), None) == _capi.LCR_ERR_INVALID and b"sampling is NULL" in L.lcr_last_error()
    assert L.lcr_get_point_cloud_sampling(None, None) == _capi.LCR_ERR_INVALID
    assert L.lcr_get_point_cloud_sampling(None, ctypes.byref(_sampling(0, 0))) == _capi.LCR_ERR_INVALID


def test_vecsim_checks_the_sampling_before_device_use(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, LowCostRobotVectorEnv, VecSim

    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())
    both = dict(observation_mode="both", image_planes=("depth", "segmentation"))
    for bad, what in ((dict(points=64, sampling="random"), "sampling must be"), (dict(points=64, sampling=1), "sampling must be"), (dict(points=64, sampling=None), "sampling must be"),
                      (dict(points=64, pool=128), "pool goes with sampling='fps'"), (dict(points=64, sampling="stride", pool=128), "pool goes with sampling='fps'"),
                      (dict(points=64, sampling="fps"), "needs a pool"), (dict(points=64, sampling="fps", pool=100), "pool must be a multiple of 64"),
                      (dict(points=64, sampling="fps", pool=0), "pool must be a multiple of 64"), (dict(points=64, sampling="fps", pool=4160), "pool must be a multiple of 64"),
                      (dict(points=64, sampling="fps", pool=128.0), "pool must be a multiple of 64"), (dict(points=64, sampling="fps", pool=True), "pool must be a multiple of 64"),
                      (dict(points=256, sampling="fps", pool=192), "pool must be at least points"), (dict(points=8192, sampling="fps", pool=4096), "pool must be at least points"),
                      (dict(points=64, sampling="fps", pool=128, normals=True), "unknown point_cloud fields"), (dict(points=100, sampling="fps", pool=128), "points")):
        with pytest.raises(ValueError, match=what):
            VecSim("reach", 4, point_cloud=bad, **both)
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, point_cloud=dict(points=64, sampling="fps", pool=128))
    for good in (dict(points=512, sampling="fps", pool=2048), dict(points=64, sampling="fps", pool=64), dict(points=4096, sampling="fps", pool=4096),
                 dict(sampling="fps", pool=1024), dict(points=128, sampling="stride"), dict(points=128, sampling="fps", pool=320, colors=True, cameras=("top",))):
        with pytest.raises(AssertionError, match="lcr_create was reached"):
            VecSim("reach", 4, point_cloud=good, **both)
    for cls in (LowCostRobotVecEnv, LowCostRobotVectorEnv):   # the vector adapters go on refusing the cloud
        with pytest.raises(ValueError, match="terminal_observation"):
            cls("reach", 4, point_cloud=dict(points=64, sampling="fps", pool=128), **both)
    rest, sm = _capi.PointCloudSampling.take(dict(points=512, sampling="fps", pool=2048, colors=True))
    assert rest == dict(points=512, colors=True) and sm.as_dict() == {"mode": "fps", "pool": 2048}
    assert _capi.PointCloudSampling.take(256)[1].as_dict() == _capi.PointCloudSampling.take(dict(points=256))[1].as_dict() == {"mode": "stride", "pool": 0}


# ---- the model ----

def _exact_dist(a, b):
    """the pinned distance with every rounding made by cloud_fps_ref.round_f32 on exact rationals"""
    F = lambda v: Fraction(float(v))
    r = cloud_fps_ref.round_f32
    dx, dy, dz = (r(F(a[k]) - F(b[k])) for k in range(3))
    m = r(F(dx) * F(dx))
    t = r(F(dy) * F(dy) + F(m))
    return r(F(dz) * F(dz) + F(t))


def _brute_force(pts, P):
    """the header's greedy rule, literally, on exact distances"""
    Q = len(pts)
    mind = [Fraction(10) ** 40] * Q   # + inf
    order = []
    for _ in range(P):
        best = max(mind)
        i = mind.index(best)          # the lowest index among the largest
        order.append(i)
        mind[i] = Fraction(-1)
        for j in range(Q):
            if mind[j] >= 0:
                mind[j] = min(mind[j], Fraction(float(_exact_dist(pts[j], pts[i]))))
    return order


def _clouds():
    rng = np.random.default_rng(12)
    uniform = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    dup = uniform.copy(); dup[20:] = dup[rng.integers(0, 20, 20)]                                      # duplicates: distance 0
    lattice = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.25)   # exact ties
    binades = (rng.uniform(1, 2, (40, 3)) * 2.0 ** rng.integers(-6, 6, (40, 3)) * rng.choice([-1, 1], (40, 3))).astype(np.float32)  # twelve binades
    tiny = (rng.uniform(-1, 1, (24, 3)) * 2.0 ** -66).astype(np.float32)                                # squared distances in the float32 denormal range
    # fused steps that land on a rounding midpoint: 1 + 2^-24 (dx = 1, dy = 2^-12), and the same a binade up
    mid = np.array([[0, 0, 0], [1, 2.0 ** -12, 0], [1, 0, 2.0 ** -12], [2, 2.0 ** -11, 0], [1, 2.0 ** -12, 2.0 ** -12], [0.5, 0.5, 0.5]], np.float32)
    return {"uniform": uniform, "duplicates": dup, "lattice": lattice, "binades": binades, "denormal": tiny, "midpoint": mid}


@pytest.mark.parametrize("name", list(_clouds()))
def test_fps_order_is_the_brute_force_greedy_in_exact_arithmetic(name):
    pts = _clouds()[name]
    Q = len(pts)
    before = cloud_fps_ref.FALLBACKS[0]
    got = cloud_fps_ref.fps_order(pts, Q)
    assert got.tolist() == _brute_force(pts, Q), name
    assert sorted(got.tolist()) == list(range(Q)) and got[0] == 0
    if name in ("midpoint", "denormal"):
        assert cloud_fps_ref.FALLBACKS[0] > before   # the exact recomputation was taken
    if name == "duplicates":   # the M distinct points first, then the duplicates at distance 0 in pool order
        tail = got[20:].tolist()
        assert tail == sorted(tail)
    for P in (1, 2, Q // 2, Q - 1):   # the prefix property
        assert cloud_fps_ref.fps_order(pts, P).tolist() == got[:P].tolist(), (name, P)
    # batched: the same orders for a stack of clouds
    both = cloud_fps_ref.fps_order(np.stack([pts, pts[::-1]]), Q // 2)
    assert both[0].tolist() == got[:Q // 2].tolist() and both[1].tolist() == cloud_fps_ref.fps_order(pts[::-1].copy(), Q // 2).tolist()


def test_the_distance_is_pinned():
    """the model's distance against the exact evaluation, element by element, with the constructed midpoint cases: 1 + 2^-24 is a tie between 1 and 1 + 2^-23 and goes to the
    even 1; (1 + 2^-23) + 2^-24 is a tie that goes UP to the even 1 + 2^-22"""
    f = np.float32
    assert cloud_fps_ref.fused(f(2.0 ** -12), f(1.0)) == f(1.0)
    assert cloud_fps_ref.fused(f(2.0 ** -12), f(1.0 + 2.0 ** -23)) == f(1.0 + 2.0 ** -22)
    assert cloud_fps_ref.fused(f(2.0 ** -12 * (1 + 2.0 ** -23)), f(1.0)) == f(1.0 + 2.0 ** -23)   # just above the tie
    for name, pts in _clouds().items():
        d = cloud_fps_ref.dist(pts[:, None, :], pts[None, :, :])
        assert d.dtype == np.float32 and (d >= 0).all() and (np.diag(d) == 0).all()
        for i in range(0, len(pts), 3):
            for j in range(len(pts)):
                assert d[i, j].view(np.uint32) == np.asarray(_exact_dist(pts[i], pts[j]), np.float32).view(np.uint32), (name, i, j)


def test_the_fused_step_on_random_triples():
    """fmaf(a, b, c) of the model on 10^5 random triples over many binades.  The model's first step, the fp64 sum of the exact product and c, is math.fma(a, b, c) where the
    interpreter has it (3.13); its float32 result is the exact rational sum rounded once, on every 50th triple"""
    rng = np.random.default_rng(3)
    n = 100_000
    a = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-40, 40, n)).astype(np.float32)
    got = cloud_fps_ref.fused(a, c)
    a64, c64 = a.astype(np.float64), c.astype(np.float64)
    if hasattr(math, "fma"):
        want = np.array([math.fma(x, x, y) for x, y in zip(a64.tolist(), c64.tolist())])
        np.testing.assert_array_equal(a64 * a64 + c64, want)
        exact = np.array([cloud_fps_ref.round_f32(Fraction(w)) for w in want.tolist()[::50]])   # (not the fused result itself: fp64 has rounded once already)
        assert (np.abs(exact.view(np.int32).astype(np.int64) - got[::50].view(np.int32).astype(np.int64)) <= 1).all()
    for i in range(0, n, 50):
        assert got[i] == cloud_fps_ref.round_f32(Fraction(float(a[i])) * Fraction(float(a[i])) + Fraction(float(c[i]))), i
    # a single rounding never differs from the double rounding by more than one float32 ulp
    twice = (a64 * a64 + c64).astype(np.float32)
    assert (np.abs(got.view(np.int32).astype(np.int64) - twice.view(np.int32).astype(np.int64)) <= 1).all()


def test_pool_sources():
    cand = np.zeros(200, bool)
    assert (cloud_fps_ref.pool_sources(cand, 64) == -1).all()
    cand[[3, 50, 51, 199]] = True
    src = cloud_fps_ref.pool_sources(cand, 64)
    assert src.shape == (64,) and set(src.tolist()) == {3, 50, 51, 199} and (np.diff(src) >= 0).all() and np.bincount(src)[[3, 50, 51, 199]].tolist() == [16] * 4
    cand[:] = True
    np.testing.assert_array_equal(cloud_fps_ref.pool_sources(cand, 64), (np.arange(64) * 2 + 1) * 200 // 128)
