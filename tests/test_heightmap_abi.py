"""CPU tests of the heightmap (include/lcr.h: "The heightmap", lcr_enable_heightmap): the additions to the C ABI (declared, bound, exported; the ABI version stays 7), the
structs against the binding, every refusal that needs no device with the field and the axis named, the accepted extremes, VecSim's and the adapters' ValueErrors before any
device call, the keyword through ShardedVecSim, and the numpy model the GPU tests compare against (tests/heightmap_ref.py) held to an evaluation in exact rational arithmetic
on seeded synthetic pixels with the constructed cases among them."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import heightmap_ref
from tests.cloud_fps_ref import round_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_heightmap_check", "lcr_enable_heightmap", "lcr_get_heightmap"]
F32 = np.float32
CTYPES = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
BOX = ((-0.125, -0.0625, 0.0), (0.125, 0.25, 0.25))
DIMS = (8, 10)


def _hdr():
    return open(os.path.join(ROOT, "include", "lcr.h")).read()


def _spec(lo=BOX[0], hi=BOX[1], dims=DIMS, **kw):
    s = _capi.HeightmapSpec()
    for k in range(3):
        s.lo[k], s.hi[k] = lo[k], hi[k]
    for k in range(2):
        s.dims[k] = dims[k]
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_the_new_functions_are_declared_bound_and_exported(hip_lib):
    hdr = _hdr()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    section = hdr[hdr.index("== The heightmap"):hdr.index("typedef struct lcr_heightmap_spec {")]
    for what in ("d_k = fmaf(sx, X_k, fmaf(sy, Y_k, - Z_k))", "p_k = fmaf(t, d_k, ro_k)", "u_k = p_k - lo_k", "v_k = u_k * inv_k", "u_k >= 0.0f && v_k < (float)H_k", "i_k = (int)v_k",
                 "inv_k = (float)((double)H_k / ((double)hi_k - (double)lo_k))", "u_z = p_z - lo_z", "u_z >= 0.0f && p_z <= hi_z", "sign bit cleared",
                 "((uint64)hb << 32) | (0xFFFFFFFF - g)", "MAXIMUM key", "the smallest g", "[N][C][Hy][Hx]", "LCR_ERR_OOM", "differ only in `source` and `filled`"):
        assert what in section, what
    for what in ("mean height", "per-cell counts", "oriented or per-env boxes", "float16 / uint8 output", "a per-cell surface id", "the recorder", "no _terminal call"):
        assert what in section, what   # the header says what the map does not do
    assert re.search(r"#define\s+LCR_HEIGHTMAP_MAX_CELLS\s+16384\b", hdr) and re.search(r"#define\s+LCR_HEIGHTMAP_MAX_DIM\s+256\b", hdr)
    assert _capi.HEIGHTMAP_MAX_CELLS == 16384 and _capi.HEIGHTMAP_MAX_DIM == 256 and _capi.HEIGHTMAP_FEATURES == {"height": 1, "rgb": 2}


def _parse(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s+(\*?)\s*(.*)$", decl)
        assert m, decl
        ptr, typ = bool(m.group(3)), m.group(2)
        for item in m.group(4).split(","):
            item = item.strip()
            a = re.match(r"(\*?)(\w+)(?:\[(\d+)\])?$", item)
            assert a, decl
            if ptr or a.group(1):
                ct = ctypes.c_void_p
            elif typ == "lcr_heightmap_spec":
                ct = _capi.HeightmapSpec
            else:
                ct = CTYPES[typ]
            fields.append((a.group(2), ct * int(a.group(3)) if a.group(3) else ct))
    return fields


def test_the_structs_match_the_header():
    hdr = _hdr()
    for name, bound, size in (("lcr_heightmap_spec", _capi.HeightmapSpec, 48), ("lcr_heightmap_view", _capi.LcrHeightmapView, 128)):
        fields = _parse(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in fields] == [n for n, _ in bound._fields_], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)
    # the grid's structs keep their sizes
    assert ctypes.sizeof(_capi.VoxelGridSpec) == 56 and ctypes.sizeof(_capi.LcrVoxelGridView) == 136


@pytest.mark.parametrize("field", ["lo", "hi"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_corner_that_is_not_finite_is_refused(hip_lib, field, k, bad):
    s = _spec()
    getattr(s, field)[k] = bad
    assert hip_lib.lcr_heightmap_check(ctypes.byref(s)) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert msg.startswith(b"%s[%d]" % (field.encode(), k)) and b"not finite" in msg and b"(%c)" % b"xyz"[k] in msg, msg
    # before the handle is looked at
    assert hip_lib.lcr_enable_heightmap(None, ctypes.byref(s)) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_last_error() == msg and b"sim is NULL" not in msg


@pytest.mark.parametrize("k", [0, 1, 2])
def test_an_empty_box_is_refused_naming_the_axis(hip_lib, k):
    for a, b in ((0.25, 0.125), (0.25, 0.25)):   # lo > hi, and lo == hi: a map has no flat box
        lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
        lo[k], hi[k] = a, b
        assert hip_lib.lcr_heightmap_check(ctypes.byref(_spec(lo, hi))) == _capi.LCR_ERR_INVALID
        msg = hip_lib.lcr_last_error()
        assert msg.startswith(b"lo[%d] >= hi[%d]" % (k, k)) and b"along %c" % b"xyz"[k] in msg and b"0.25" in msg, msg


def test_dims_features_source_cameras_and_ids_are_refused_by_name(hip_lib):
    L = hip_lib
    for k in range(2):
        for bad in (0, -4, 257, 260):
            dims = [8, 8]
            dims[k] = bad
            assert L.lcr_heightmap_check(ctypes.byref(_spec(dims=dims))) == _capi.LCR_ERR_INVALID
            msg = L.lcr_last_error()
            assert msg.startswith(b"dims[%d] (%c)" % (k, b"xy"[k])) and b"1 .. 256" in msg and str(bad).encode() in msg, msg
    for bad in (1, 2, 6, 10, 254):
        assert L.lcr_heightmap_check(ctypes.byref(_spec(dims=(bad, 8)))) == _capi.LCR_ERR_INVALID
        msg = L.lcr_last_error()
        assert msg.startswith(b"dims[0] (x) must be a multiple of 4") and str(bad).encode() in msg, msg
    for dims in ((256, 65), (132, 125), (256, 256), (68, 241)):
        assert L.lcr_heightmap_check(ctypes.byref(_spec(dims=dims))) == _capi.LCR_ERR_INVALID
        msg = L.lcr_last_error()
        assert msg.startswith(b"dims") and b"cells" in msg and b"16384" in msg and str(dims[0] * dims[1]).encode() in msg, msg
    for dims in ((4, 1), (256, 64), (128, 128), (64, 256), (12, 7), (100, 129)):   # the accepted extremes among them
        assert L.lcr_heightmap_check(ctypes.byref(_spec(dims=dims))) == 0, (dims, L.lcr_last_error())
    for field, bads, word in (("features", (4, 8, 7), b"features"), ("source", (2, -1), b"source"), ("cameras", (8, 9), b"cameras"), ("ids", (1, 0x800, 0x7FD), b"ids")):
        for bad in bads:
            assert L.lcr_heightmap_check(ctypes.byref(_spec(**{field: bad}))) == _capi.LCR_ERR_INVALID, (field, bad)
            assert L.lcr_last_error().startswith(word), (field, bad, L.lcr_last_error())
    for good in (dict(features=0), dict(features=1), dict(features=2), dict(features=3), dict(source=1), dict(cameras=7, ids=0x7FE)):
        assert L.lcr_heightmap_check(ctypes.byref(_spec(**good))) == 0, (good, L.lcr_last_error())
    assert L.lcr_heightmap_check(None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in L.lcr_last_error()


def test_a_null_handle_is_refused_behind_the_spec(hip_lib):
    L = hip_lib
    assert L.lcr_enable_heightmap(None, ctypes.byref(_spec())) == _capi.LCR_ERR_INVALID and b"sim is NULL" in L.lcr_last_error()
    assert L.lcr_enable_heightmap(None, None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in L.lcr_last_error()
    assert L.lcr_enable_heightmap(None, ctypes.byref(_spec(dims=(6, 8)))) == _capi.LCR_ERR_INVALID and L.lcr_last_error().startswith(b"dims[0]")
    assert L.lcr_get_heightmap(None, ctypes.byref(_capi.LcrHeightmapView())) == _capi.LCR_ERR_INVALID
    assert L.lcr_get_heightmap(None, None) == _capi.LCR_ERR_INVALID


def test_vecsim_and_the_adapters_refuse_before_any_device_call(hip_lib):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecenv import LowCostRobotVecEnv, LowCostRobotVectorEnv

    box, dims = BOX, DIMS
    img = dict(observation_mode="both", image_planes=("depth", "segmentation"))
    for kw, word in ((dict(heightmap=dict(box=box, dims=dims)), "image observations"),
                     (dict(heightmap=dict(box=box, dims=dims), observation_mode="both"), "image_planes=('depth', 'segmentation')"),
                     (dict(heightmap=dict(box=box, dims=dims), observation_mode="both", image_planes=("depth",)), "segmentation plane"),
                     (dict(heightmap=dict(box=box, dims=dims), observation_mode="both", image_planes=("segmentation",)), "depth and the segmentation plane"),
                     (dict(heightmap=dict(box=box, dims=dims, cameras=("wrist",)), **img), "no wrist_camera"),
                     (dict(heightmap=dict(dims=dims), **img), "neither has a default"),
                     (dict(heightmap=dict(box=box), **img), "neither has a default"),
                     (dict(heightmap=dict(box=box, dims=(6, 8)), **img), "multiple of 4"),
                     (dict(heightmap=dict(box=box, dims=(8, 257)), **img), "1 .. 256"),
                     (dict(heightmap=dict(box=box, dims=(8, 8, 8)), **img), "dims must be (Hx, Hy)"),
                     (dict(heightmap=dict(box=box, dims=(256, 65)), **img), "at most 16384"),
                     (dict(heightmap=dict(box=((0, 0, 0), (1, 1, math.inf)), dims=dims), **img), "hi[2] is not finite"),
                     (dict(heightmap=dict(box=((0, 0, 0), (1, None, 1)), dims=dims), **img), "hi[1]"),
                     (dict(heightmap=dict(box=((0, 0.5, 0), (1, 0.5, 1)), dims=dims), **img), "lo[1] >= hi[1]"),
                     (dict(heightmap=dict(box=box, dims=dims, features=("height", "normals")), **img), "features"),
                     (dict(heightmap=dict(box=box, dims=dims, source=1), **img), "source"),
                     (dict(heightmap=dict(box=box, dims=dims, ids=("sky",)), **img), "ids"),
                     (dict(heightmap=dict(box=box, dims=dims, dtype="uint8"), **img), "unknown heightmap fields"),
                     (dict(heightmap=64, **img), "heightmap must be None or a dict")):
        with pytest.raises(ValueError, match=re.escape(word)):
            VecSim("reach", 4, **kw)
    for Adapter in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        with pytest.raises(ValueError, match="heightmap is for on-device loops over VecSim"):
            Adapter("reach", 4, heightmap=dict(box=box, dims=dims), **img)
    sp = _capi.HeightmapSpec.from_any(dict(box=box, dims=dims, features=("rgb",), ids=("arm", "floor"), cameras=("top",), source=True))
    assert sp.as_dict() == {"lo": box[0], "hi": box[1], "dims": dims, "cameras": ("top",), "ids": (1, 2, 3, 4, 5, 6, 7, 8), "features": ("height", "rgb"), "source": True}


def test_sharded_vecsim_gives_every_shard_the_spec(monkeypatch):
    from gym_lowcostrobot_amd import sharding, vecsim

    made = []

    class Fake:
        action_dim = 4

        def __init__(self, task, n, **kw):
            made.append((task, n, kw))

        def alloc_actions(self):
            return None

    monkeypatch.setattr(vecsim, "VecSim", Fake)
    spec = dict(box=BOX, dims=DIMS, features=("height", "rgb"))
    sharding.ShardedVecSim("push", 128, [0, 0], observation_mode="both", image_planes=("depth", "segmentation"), heightmap=spec)
    assert len(made) == 2 and all(n == 64 and kw["heightmap"] is spec for _, n, kw in made)
    assert [kw["env_id_offset"] for _, _, kw in made] == [0, 64]


# ---- the model against exact rational arithmetic ----

def _fr(x):
    return Fraction(float(x))


def _exact_axis(p, lo, inv, D):
    """the header's cell of one coordinate, in Fractions with one rounding to float32 per operation -> (inside, index)"""
    u = round_f32(_fr(p) - _fr(lo))
    v = round_f32(_fr(u) * _fr(inv))
    inside = _fr(u) >= 0 and _fr(v) < D
    return inside, (math.floor(_fr(v)) if inside else 0)


def _exact_height(pz, lo_z, hi_z):
    """-> (inside along z, the height as a Fraction: |u_z| of the float32 u_z)"""
    u = round_f32(_fr(pz) - _fr(lo_z))
    return (_fr(u) >= 0 and _fr(pz) <= _fr(hi_z)), abs(_fr(u))


def _inv(lo, hi, D):
    return F32(float(D) / (float(F32(hi)) - float(F32(lo))))   # the header's inv_k


def _bits_of(h):
    """the float32 bit pattern of a non-negative Fraction that is a float32 value"""
    f = F32(float(h))
    assert _fr(f) == h
    return int(np.asarray(f, F32).view(np.uint32))


def _against_exact(points, seg_ok, lo, hi, inv, dims):
    """points (G, 3) float32 of one env's pixels in the order of g, seg_ok (G,) bool: the model's per-pixel decisions, hb and per-cell winners against a brute-force loop in
    exact arithmetic.  -> the model's dict and the exact per-pixel (inside, ix, iy, height) list"""
    G = len(points)
    pts = np.asarray(points, F32).reshape(1, G, 3)
    seg = [np.where(seg_ok, 9, 0).astype(np.uint8).reshape(1, 1, G)]
    rng = np.random.default_rng(5)
    rgb = [rng.integers(0, 256, (1, 1, G, 3), dtype=np.uint8)]
    got = heightmap_ref.heightmap(None, seg, rgb, None, dict(lo=lo, hi=hi, dims=dims, ids=0, rgb=True), inv, points=pts)
    Hx, Hy = dims
    best = {}
    exact = []
    for g in range(G):
        p = pts[0, g]
        inx, ix = _exact_axis(p[0], lo[0], inv[0], Hx)
        iny, iy = _exact_axis(p[1], lo[1], inv[1], Hy)
        inz, h = _exact_height(p[2], lo[2], hi[2])
        inside = bool(seg_ok[g]) and inx and iny and inz
        exact.append((inside, ix, iy, h))
        assert bool(got["inside"][0, g]) == inside, (g, p.tolist())
        if inside:
            assert int(got["lin"][0, g]) == iy * Hx + ix, (g, p.tolist())
            assert int(got["hb"][0, g]) == _bits_of(h), (g, p.tolist())
            c = iy * Hx + ix
            if c not in best or (h, -g) > (best[c][0], -best[c][1]):   # the highest point; among equal heights the smallest g
                best[c] = (h, g)
    src = np.full(Hx * Hy, -1, np.int64)
    hbits = np.zeros(Hx * Hy, np.uint32)
    for c, (h, g) in best.items():
        src[c], hbits[c] = g, _bits_of(h)
    np.testing.assert_array_equal(got["source"].reshape(-1), src)
    np.testing.assert_array_equal(got["heightmap"][0, 0].reshape(-1).view(np.uint32), hbits)
    assert int(got["count"][0]) == sum(e[0] for e in exact) and int(got["filled"][0]) == len(best)
    want_rgb = np.zeros((3, Hx * Hy), F32)
    for c, (h, g) in best.items():
        want_rgb[:, c] = rgb[0][0, 0, g].astype(F32) * F32(1 / 255)
    np.testing.assert_array_equal(got["heightmap"][0, 1:].reshape(3, -1).view(np.uint32), want_rgb.view(np.uint32))
    return got, exact


def test_the_model_on_seeded_pixels_with_the_constructed_cases():
    dims = (8, 10)
    lo, hi = np.array(BOX[0], F32), np.array(BOX[1], F32)
    inv = np.array([_inv(lo[k], hi[k], dims[k]) for k in range(2)], F32)
    assert (inv == F32(32.0)).all() and lo[2] == 0.0 and not np.signbit(lo[2])
    rng = np.random.default_rng(11)
    G = 2 * 144                                   # two slots of 12 x 12 pixels
    pts = rng.uniform(np.array([-0.16, -0.1, -0.03]), np.array([0.16, 0.29, 0.3]), (G, 3)).astype(F32)
    pts[:, 2] = np.round(pts[:, 2] * 64) / 64     # few distinct heights: ties happen among the random pixels too
    seg_ok = rng.uniform(size=G) < 0.85
    mid = [0.0, 0.1, 0.1]
    down = F32(-np.inf)

    def at(k, x):
        p = list(mid)
        p[k] = x
        return p

    case = {}

    def put(name, g, p, ok=True):
        pts[g], seg_ok[g] = np.asarray(p, F32), ok
        case[name] = g

    # a point exactly on each of the six faces
    put("lo_x", 3, at(0, lo[0])); put("lo_y", 4, at(1, lo[1])); put("lo_z", 5, [0.11, 0.24, lo[2]])
    put("hi_x", 6, at(0, hi[0])); put("hi_y", 7, at(1, hi[1])); put("hi_z", 8, [0.11, 0.2, hi[2]])
    # p_z = - 0.0 against lo_z = + 0.0: u_z = - 0.0 passes the test, its height is + 0.0; a cell of its own
    put("neg_zero", 9, [-0.12, 0.24, -0.0])
    # a denormal u: along z (height word 1) and along x and y (cell 0), in corner cells of their own
    put("denormal_z", 10, [0.12, -0.06, 1e-45])
    put("below_lo_z", 11, [0.12, -0.06, -1e-45])
    put("one_ulp_above_hi_z", 12, [0.11, 0.2, np.nextafter(hi[2], F32(np.inf))])
    # bit-equal heights from two slots in one cell: the smaller g wins; and a higher point of the second slot wins over a lower one of the first
    put("tie_slot0", 100, [-0.1, -0.05, 0.28125 - 0.0625]); put("tie_slot1", 144 + 20, [-0.1001, -0.0501, 0.28125 - 0.0625])
    put("low_slot0", 101, [0.05, -0.05, 0.03125 * 7]); put("high_slot1", 144 + 21, [0.0501, -0.0501, np.nextafter(F32(0.03125 * 7), F32(np.inf))])
    for g in range(G):   # keep the random pixels out of the constructed cells and below the constructed heights there
        if g not in case.values():
            ins, c = heightmap_ref.cell_of(pts[g:g + 1], lo, inv, dims)
            if ins[0] and (int(c[0, 0]), int(c[0, 1])) in ((0, 0), (5, 0), (7, 0), (7, 9), (0, 9), (7, 8)):
                seg_ok[g] = False
    got, exact = _against_exact(pts, seg_ok, lo, hi, inv, dims)
    assert seg_ok.sum() > 200 and 100 < int(got["count"][0]) < G
    src = got["source"][0]
    hm = got["heightmap"][0, 0].view(np.uint32)
    for name in ("lo_x", "lo_y", "lo_z", "hi_z", "neg_zero", "denormal_z"):
        assert exact[case[name]][0], name
    for name in ("hi_x", "hi_y", "below_lo_z", "one_ulp_above_hi_z"):    # v = H exactly: outside along x and y; both z faces belong to the box, one ulp beyond does not
        assert not exact[case[name]][0], name
    assert exact[case["lo_x"]][1] == 0 and exact[case["lo_y"]][2] == 0
    # the z faces: height + 0.0 on lo_z and hi_z - lo_z on hi_z, each the winner of its cell; a filled cell at height 0.0 shows only in source / filled
    assert src[9, 7] == case["lo_z"] and hm[9, 7] == 0
    assert src[8, 7] == case["hi_z"] and hm[8, 7] == np.asarray(F32(0.25)).view(np.uint32)
    assert np.signbit(F32(-0.0) - lo[2]) and src[9, 0] == case["neg_zero"] and hm[9, 0] == 0       # not 0x80000000
    assert src[0, 7] == case["denormal_z"] and hm[0, 7] == 1
    assert src[0, 0] == case["tie_slot0"] and exact[case["tie_slot1"]][0] and exact[case["tie_slot1"]][1:] == exact[case["tie_slot0"]][1:]
    # (slot 1's higher point wins its cell although its g is larger)
    assert exact[case["low_slot0"]][1:3] == exact[case["high_slot1"]][1:3] == (5, 0) and src[0, 5] == case["high_slot1"]
    assert (got["count"] > got["filled"]).all()


def test_a_denormal_u_along_x_and_a_higher_point_of_a_later_slot():
    """lo = 0 along x and y: a denormal p is a denormal u, inside, in cell 0 (denormals are kept: u * inv is not flushed); the smallest denormal below zero is outside"""
    dims = (4, 3)
    lo, hi = np.array([0.0, 0.0, -0.5], F32), np.array([0.3, 0.7, 0.5], F32)
    inv = np.array([_inv(lo[k], hi[k], dims[k]) for k in range(2)], F32)
    tiny = [F32(1e-45), F32(1e-40), F32(1.1754942e-38)]
    assert all(0 < float(t) < 2.0 ** -126 for t in tiny)
    pts = [[t, 0.5, 0.0] for t in tiny] + [[0.2, t, 0.1] for t in tiny] + [[-1e-45, 0.5, 0.0], [0.2, -1e-45, 0.0]]
    pts += [[0.2, 0.001, 0.25], [0.2, 0.002, 0.1]]          # cell (2, 0) again, higher, from "a later slot": g = 8 wins over g = 3 .. 5
    got, exact = _against_exact(np.array(pts, F32), np.ones(len(pts), bool), lo, hi, inv, dims)
    assert [e[0] for e in exact] == [True] * 6 + [False, False, True, True]
    assert all(e[1] == 0 for e in exact[:3]) and all(e[2] == 0 for e in exact[3:6])
    assert got["source"][0, 0, 2] == 8 and got["source"][0, 2, 0] == 0


def test_the_box_is_half_open_along_x_and_y_only_up_to_rounding():
    """with a cell size that is no power of two a point BELOW hi_k can have v_k round up to H_k: it is outside, by the model and by the exact evaluation alike"""
    found = 0
    for lo_, hi_, D in ((0.0, 0.3, 12), (-0.1, 0.2, 12), (0.05, 0.35, 8), (0.0, 0.7, 64), (-0.3, 0.3, 20)):
        lo, hi = F32(lo_), F32(hi_)
        inv = _inv(lo, hi, D)
        p = hi
        pts = []
        for _ in range(64):
            p = np.nextafter(p, F32(-np.inf))
            pts.append([p, 0.5, 0.5])
        for axis in (0, 1):
            P = np.array(pts, F32)
            if axis:
                P = P[:, [1, 0, 2]]
            lo3, hi3 = np.array([0, 0, 0], F32), np.array([1, 1, 1], F32)
            lo3[axis], hi3[axis] = lo, hi
            inv2, dims = np.array([1, 1], F32), [1, 1]
            inv2[axis], dims[axis] = inv, D
            _, exact = _against_exact(P, np.ones(len(P), bool), lo3, hi3, inv2, tuple(dims))
            found += sum(not e[0] for e in exact)
            assert all(e[1 + axis] == D - 1 for e in exact if e[0])
    assert found > 0   # the regime exists among the cases
