"""CPU tests of the voxel grid (include/lcr.h: "The voxel grid", lcr_enable_voxel_grid): the additions to the C ABI (declared, bound, exported; the ABI version stays 7),
the structs against the binding, every refusal that needs no device with the field named, VecSim's and the adapters' ValueErrors before any device call, and the numpy model
the GPU tests compare against (tests/voxel_ref.py) held to an evaluation in exact rational arithmetic on constructed points."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import voxel_ref
from tests.cloud_fps_ref import round_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_voxel_grid_check", "lcr_enable_voxel_grid", "lcr_get_voxel_grid"]
F32 = np.float32
CTYPES = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


def _hdr():
    return open(os.path.join(ROOT, "include", "lcr.h")).read()


def _spec(lo=(-0.125, -0.0625, 0.0), hi=(0.125, 0.25, 0.25), dims=(8, 10, 8), **kw):
    s = _capi.VoxelGridSpec()
    for k in range(3):
        s.lo[k], s.hi[k], s.dims[k] = lo[k], hi[k], dims[k]
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
    assert "== The voxel grid" in hdr
    section = hdr[hdr.index("== The voxel grid"):hdr.index("typedef struct lcr_voxel_grid_spec {")]
    for what in ("d_k = fmaf(sx, X_k, fmaf(sy, Y_k, - Z_k))", "p_k = fmaf(t, d_k, ro_k)", "u_k = p_k - lo_k", "v_k = u_k * inv_k", "u_k >= 0.0f && v_k < (float)D_k", "i_k = (int)v_k",
                 "inv_k = (float)((double)D_k / ((double)hi_k - (double)lo_k))", "half-open UP TO THIS ROUNDING", "the smallest g", "[N][C][Dz][Dy][Dx]", "LCR_ERR_OOM"):
        assert what in section, what
    for what in ("mean colours", "per-voxel counts", "oriented or per-env boxes", "float16", "the recorder", "no _terminal call"):
        assert what in section, what   # the header says what the grid does not do
    assert re.search(r"#define\s+LCR_VOXEL_MAX_CELLS\s+32768\b", hdr) and re.search(r"#define\s+LCR_VOXEL_MAX_DIM\s+64\b", hdr)
    assert _capi.VOXEL_MAX_CELLS == 32768 and _capi.VOXEL_MAX_DIM == 64 and _capi.VOXEL_FEATURES == {"occupancy": 1, "rgb": 2}


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
            elif typ == "lcr_voxel_grid_spec":
                ct = _capi.VoxelGridSpec
            else:
                ct = CTYPES[typ]
            fields.append((a.group(2), ct * int(a.group(3)) if a.group(3) else ct))
    return fields


def test_the_structs_match_the_header():
    hdr = _hdr()
    for name, bound, size in (("lcr_voxel_grid_spec", _capi.VoxelGridSpec, 56), ("lcr_voxel_grid_view", _capi.LcrVoxelGridView, 136)):
        fields = _parse(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in fields] == [n for n, _ in bound._fields_], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)
    # the cloud's and the stack's structs keep their sizes
    assert ctypes.sizeof(_capi.PointCloudSpec) == 16 and ctypes.sizeof(_capi.LcrPointCloudView) == 80 and ctypes.sizeof(_capi.ObsStackSpec) == 16


@pytest.mark.parametrize("field", ["lo", "hi"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_corner_that_is_not_finite_is_refused(hip_lib, field, k, bad):
    s = _spec()
    getattr(s, field)[k] = bad
    assert hip_lib.lcr_voxel_grid_check(ctypes.byref(s)) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert msg.startswith(b"%s[%d]" % (field.encode(), k)) and b"not finite" in msg and b"(%c)" % b"xyz"[k] in msg, msg
    # before the handle is looked at
    assert hip_lib.lcr_enable_voxel_grid(None, ctypes.byref(s)) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_last_error() == msg and b"sim is NULL" not in msg


@pytest.mark.parametrize("k", [0, 1, 2])
def test_an_empty_box_is_refused_naming_the_axis(hip_lib, k):
    for a, b in ((0.25, 0.125), (0.25, 0.25)):   # lo > hi, and lo == hi: a grid has no flat box
        lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
        lo[k], hi[k] = a, b
        assert hip_lib.lcr_voxel_grid_check(ctypes.byref(_spec(lo, hi))) == _capi.LCR_ERR_INVALID
        msg = hip_lib.lcr_last_error()
        assert msg.startswith(b"lo[%d] >= hi[%d]" % (k, k)) and b"along %c" % b"xyz"[k] in msg and b"0.25" in msg, msg


def test_dims_features_dtype_source_cameras_and_ids_are_refused_by_name(hip_lib):
    L = hip_lib
    for k in range(3):
        for bad in (0, -4, 65, 68):
            dims = [8, 8, 8]
            dims[k] = bad
            assert L.lcr_voxel_grid_check(ctypes.byref(_spec(dims=dims))) == _capi.LCR_ERR_INVALID
            msg = L.lcr_last_error()
            assert msg.startswith(b"dims[%d] (%c)" % (k, b"xyz"[k])) and str(bad).encode() in msg, msg
    for bad in (1, 2, 6, 10, 63):
        assert L.lcr_voxel_grid_check(ctypes.byref(_spec(dims=(bad, 8, 8)))) == _capi.LCR_ERR_INVALID
        msg = L.lcr_last_error()
        assert msg.startswith(b"dims[0] (x) must be a multiple of 4") and str(bad).encode() in msg, msg
    for dims in ((64, 64, 9), (36, 31, 30), (64, 64, 64)):
        assert L.lcr_voxel_grid_check(ctypes.byref(_spec(dims=dims))) == _capi.LCR_ERR_INVALID
        msg = L.lcr_last_error()
        assert msg.startswith(b"dims") and b"voxels" in msg and b"32768" in msg and str(dims[0] * dims[1] * dims[2]).encode() in msg, msg
    for dims in ((64, 64, 8), (32, 32, 32), (4, 1, 1), (12, 7, 5), (60, 60, 9)):
        assert L.lcr_voxel_grid_check(ctypes.byref(_spec(dims=dims))) == 0, (dims, L.lcr_last_error())
    for field, bads, word in (("features", (4, 8, 7), b"features"), ("dtype", (1, 3, -1), b"dtype"), ("source", (2, -1), b"source"), ("cameras", (8, 9), b"cameras"),
                              ("ids", (1, 0x800, 0x7FD), b"ids")):
        for bad in bads:
            assert L.lcr_voxel_grid_check(ctypes.byref(_spec(**{field: bad}))) == _capi.LCR_ERR_INVALID, (field, bad)
            assert L.lcr_last_error().startswith(word), (field, bad, L.lcr_last_error())
    assert b"float16" in (L.lcr_voxel_grid_check(ctypes.byref(_spec(dtype=1))), L.lcr_last_error())[1]
    for good in (dict(features=0), dict(features=1), dict(features=2), dict(features=3), dict(dtype=2), dict(source=1), dict(cameras=7, ids=0x7FE)):
        assert L.lcr_voxel_grid_check(ctypes.byref(_spec(**good))) == 0, (good, L.lcr_last_error())
    assert L.lcr_voxel_grid_check(None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in L.lcr_last_error()


def test_a_null_handle_is_refused_behind_the_spec(hip_lib):
    L = hip_lib
    assert L.lcr_enable_voxel_grid(None, ctypes.byref(_spec())) == _capi.LCR_ERR_INVALID and b"sim is NULL" in L.lcr_last_error()
    assert L.lcr_enable_voxel_grid(None, None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in L.lcr_last_error()
    assert L.lcr_enable_voxel_grid(None, ctypes.byref(_spec(dims=(6, 8, 8)))) == _capi.LCR_ERR_INVALID and L.lcr_last_error().startswith(b"dims[0]")
    assert L.lcr_get_voxel_grid(None, ctypes.byref(_capi.LcrVoxelGridView())) == _capi.LCR_ERR_INVALID
    assert L.lcr_get_voxel_grid(None, None) == _capi.LCR_ERR_INVALID


def test_vecsim_and_the_adapters_refuse_before_any_device_call(hip_lib):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecenv import LowCostRobotVecEnv, LowCostRobotVectorEnv

    box, dims = ((-0.125, -0.0625, 0.0), (0.125, 0.25, 0.25)), (8, 10, 8)
    img = dict(observation_mode="both", image_planes=("depth", "segmentation"))
    for kw, word in ((dict(voxel_grid=dict(box=box, dims=dims)), "image observations"),
                     (dict(voxel_grid=dict(box=box, dims=dims), observation_mode="both"), "image_planes=('depth', 'segmentation')"),
                     (dict(voxel_grid=dict(box=box, dims=dims), observation_mode="both", image_planes=("depth",)), "segmentation plane"),
                     (dict(voxel_grid=dict(box=box, dims=dims, cameras=("wrist",)), **img), "no wrist_camera"),
                     (dict(voxel_grid=dict(dims=dims), **img), "neither has a default"),
                     (dict(voxel_grid=dict(box=box), **img), "neither has a default"),
                     (dict(voxel_grid=dict(box=box, dims=(6, 8, 8)), **img), "multiple of 4"),
                     (dict(voxel_grid=dict(box=box, dims=(8, 8, 65)), **img), "1 .. 64"),
                     (dict(voxel_grid=dict(box=box, dims=(64, 64, 9)), **img), "at most 32768"),
                     (dict(voxel_grid=dict(box=((0, 0, 0), (1, 1, math.inf)), dims=dims), **img), "hi[2] is not finite"),
                     (dict(voxel_grid=dict(box=((0, 0, 0), (1, None, 1)), dims=dims), **img), "hi[1]"),
                     (dict(voxel_grid=dict(box=((0, 0.5, 0), (1, 0.5, 1)), dims=dims), **img), "lo[1] >= hi[1]"),
                     (dict(voxel_grid=dict(box=box, dims=dims, features=("occupancy", "normals")), **img), "features"),
                     (dict(voxel_grid=dict(box=box, dims=dims, dtype="float16"), **img), "dtype"),
                     (dict(voxel_grid=dict(box=box, dims=dims, source=1), **img), "source"),
                     (dict(voxel_grid=dict(box=box, dims=dims, ids=("sky",)), **img), "ids"),
                     (dict(voxel_grid=dict(box=box, dims=dims, points=64), **img), "unknown voxel_grid fields"),
                     (dict(voxel_grid=64, **img), "voxel_grid must be None or a dict")):
        with pytest.raises(ValueError, match=re.escape(word)):
            VecSim("reach", 4, **kw)
    for Adapter in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        with pytest.raises(ValueError, match="voxel_grid is for on-device loops over VecSim"):
            Adapter("reach", 4, voxel_grid=dict(box=box, dims=dims), **img)
    sp = _capi.VoxelGridSpec.from_any(dict(box=box, dims=dims, features=("rgb",), ids=("arm", "floor"), cameras=("top",), dtype=np.float32, source=True))
    assert sp.as_dict() == {"lo": box[0], "hi": box[1], "dims": dims, "cameras": ("top",), "ids": (1, 2, 3, 4, 5, 6, 7, 8), "features": ("occupancy", "rgb"), "dtype": "float32",
                            "source": True}


# ---- the model against exact rational arithmetic ----

def _exact_axis(p, lo, inv, D):
    """the header's voxel of one coordinate, in Fractions with one rounding to float32 per operation -> (inside, index)"""
    u = round_f32(Fraction(float(p)) - Fraction(float(lo)))
    v = round_f32(Fraction(float(u)) * Fraction(float(inv)))
    inside = Fraction(float(u)) >= 0 and Fraction(float(v)) < D
    return inside, (math.floor(Fraction(float(v))) if inside else 0)


def _exact(p, lo, inv, dims):
    got = [_exact_axis(p[k], lo[k], inv[k], dims[k]) for k in range(3)]
    return all(g[0] for g in got), [g[1] for g in got]


def _inv(lo, hi, D):
    return F32(float(D) / (float(F32(hi)) - float(F32(lo))))   # the header's inv_k


def _against_exact(points, lo, inv, dims):
    points = np.asarray(points, F32)
    ins, idx = voxel_ref.voxel_of(points, lo, inv, dims)
    for i, p in enumerate(points):
        want_in, want_idx = _exact(p, lo, inv, dims)
        assert bool(ins[i]) == want_in, (i, p.tolist())
        if want_in:
            assert idx[i].tolist() == want_idx, (i, p.tolist())
    return ins, idx


def test_the_model_on_constructed_points():
    dims = (8, 10, 8)
    lo, hi = np.array([-0.125, -0.0625, 0.0], F32), np.array([0.125, 0.25, 0.25], F32)
    inv = np.array([_inv(lo[k], hi[k], dims[k]) for k in range(3)], F32)
    assert (inv == F32(32.0)).all()
    mid = [0.0, 0.1, 0.1]

    def at(k, x):
        p = list(mid)
        p[k] = x
        return p

    down = F32(-np.inf)
    # u = - 0.0 (p_z = - 0.0 against lo_z = + 0.0): inside, in cell 0; and u = + 0.0 on the other two faces
    ins, idx = _against_exact([at(2, -0.0), at(0, lo[0]), at(1, lo[1])], lo, inv, dims)
    assert np.signbit(F32(-0.0) - lo[2]) and ins.all() and idx[0, 2] == 0 and idx[1, 0] == 0 and idx[2, 1] == 0
    # one ulp below lo: outside
    ins, _ = _against_exact([at(k, np.nextafter(lo[k], down)) for k in range(2)] + [at(2, -1e-45)], lo, inv, dims)
    assert not ins.any()
    # u denormal: inside, in cell 0 (denormals are kept: u * 32 is not flushed); the smallest denormal below zero is outside
    tiny = [F32(1e-45), F32(1e-40), F32(1.1754942e-38)]
    ins, idx = _against_exact([at(2, t) for t in tiny], lo, inv, dims)
    assert all(0 < float(t) < 2.0 ** -126 for t in tiny) and ins.all() and (idx[:, 2] == 0).all()
    # v lands exactly on D_k: outside (the half-open top); one ulp below: inside, in the last cell
    ins, _ = _against_exact([at(k, hi[k]) for k in range(3)], lo, inv, dims)
    assert not ins.any()
    below = [at(k, np.nextafter(hi[k], down)) for k in range(3)]
    ins, idx = _against_exact(below, lo, inv, dims)
    # (along z, where lo is 0.0, the subtraction is exact and v is one ulp below D_z.  Along x and y the float below hi_k is ALREADY outside: u = hi_k - 2^-27 - lo_k lies
    #  halfway between two float32 values and rounds to even, to hi_k - lo_k, so v = D_k -- the half-open box "up to this rounding" of the header, at a power-of-two cell)
    assert ins.tolist() == [False, False, True] and idx[2, 2] == dims[2] - 1
    assert (F32(below[2][2]) - lo[2]) * inv[2] == np.nextafter(F32(dims[2]), down)
    for k in range(2):
        assert F32(below[k][k]) < hi[k] and (F32(below[k][k]) - lo[k]) * inv[k] == F32(dims[k])
    # one ulp of u below hi_k - lo_k: v is one ulp below D_k, inside, in the last cell
    last = [at(k, lo[k] + np.nextafter(hi[k] - lo[k], down)) for k in range(3)]
    ins, idx = _against_exact(last, lo, inv, dims)
    assert ins.all() and [idx[k, k] for k in range(3)] == [dims[k] - 1 for k in range(3)]
    for k in range(3):
        assert (F32(last[k][k]) - lo[k]) * inv[k] == np.nextafter(F32(dims[k]), down), k
    # every interior cell boundary along z (lo_z = 0.0: u is exact): the boundary belongs to the upper cell, the float below it to the lower; along x the model is only
    # held to the exact evaluation (a float below a boundary may round onto it, as at hi above)
    pts = [at(2, F32(i) / inv[2]) for i in range(1, dims[2])] + [at(2, np.nextafter(F32(i) / inv[2], down)) for i in range(1, dims[2])]
    ins, idx = _against_exact(pts, lo, inv, dims)
    assert ins.all() and idx[:, 2].tolist() == list(range(1, dims[2])) + list(range(0, dims[2] - 1))
    _against_exact([at(0, lo[0] + F32(i) / inv[0]) for i in range(1, dims[0])] + [at(0, np.nextafter(lo[0] + F32(i) / inv[0], down)) for i in range(1, dims[0])], lo, inv, dims)


def test_the_box_is_half_open_only_up_to_rounding():
    """with a cell size that is no power of two a point BELOW hi_k can have v_k round up to D_k: it is outside, by the model and by the exact evaluation alike"""
    found = 0
    for lo_, hi_, D in ((0.0, 0.3, 10), (-0.1, 0.2, 12), (0.05, 0.35, 7), (0.0, 0.7, 64), (-0.3, 0.3, 20)):
        lo, hi = F32(lo_), F32(hi_)
        inv = _inv(lo, hi, D)
        p = hi
        pts = []
        for _ in range(64):
            p = np.nextafter(p, F32(-np.inf))
            pts.append([p, 0.5, 0.5])
        lo3, inv3, dims = np.array([lo, 0, 0], F32), np.array([inv, 1, 1], F32), (D, 1, 1)
        ins, idx = _against_exact(pts, lo3, inv3, dims)
        found += int((~ins).sum())
        assert (idx[ins][:, 0] == D - 1).all()
    assert found > 0   # the regime exists among the cases


def test_a_voxel_hit_from_two_slots_keeps_the_smaller_pixel_index():
    """two slots with the same camera looking straight down: every pixel pair falls in the same voxel, and the source is slot 0's pixel unless that pixel is no candidate;
    the grid, source, count and occupied of the model against a brute-force loop over the pixels in exact arithmetic"""
    H = W = 4
    N, S = 2, 2
    pose = np.zeros((S, 13, N), F32)
    pose[:, 2] = 1.0                      # ro = (0, 0, 1)
    pose[:, 3] = 1.0; pose[:, 7] = 1.0; pose[:, 11] = 1.0   # X, Y, Z: the world axes; the camera looks along - z
    pose[:, 12] = 0.0625                  # s
    depth = [np.ones((N, H, W), F32) for _ in range(S)]   # every ray ends on z = 0
    seg = [np.full((N, H, W), 9, np.uint8) for _ in range(S)]
    seg[0][0, 0:2, :] = 0                 # env 0: the two rows of slot 0 that fall in cell iy = 1 see the sky -- there slot 1 is the source
    seg[0][1, :, 2] = 1                   # env 1: a column of slot 0 sees the floor, which is no candidate by the default ids
    seg[1][1, 3, 3] = 0x80 | 9            # the marker bit is ignored
    rng = np.random.default_rng(0)
    rgb = [rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8) for _ in range(S)]
    lo, hi, dims = np.array([-0.125, -0.125, -0.125], F32), np.array([0.125, 0.125, 0.125], F32), (4, 2, 2)
    inv = np.array([_inv(lo[k], hi[k], dims[k]) for k in range(3)], F32)
    for dtype in ("uint8", "float32"):
        got = voxel_ref.grid(depth, seg, rgb, pose, dict(lo=lo, dims=dims, ids=0, rgb=True, dtype=dtype), inv)
        Dx, Dy, Dz = dims
        src = np.full((N, Dz, Dy, Dx), -1, np.int64)
        cnt = np.zeros(N, np.int64)
        for e in range(N):
            for g in range(S * H * W):
                sl, pix = divmod(g, H * W)
                if (int(seg[sl][e].reshape(-1)[pix]) & 0x7F) not in range(2, 11):
                    continue
                inside, (ix, iy, iz) = _exact(got["points"][e, g], lo, inv, dims)
                if inside:
                    cnt[e] += 1
                    if src[e, iz, iy, ix] < 0:
                        src[e, iz, iy, ix] = g      # (g ascends: the first is the smallest)
        np.testing.assert_array_equal(got["source"], src)
        np.testing.assert_array_equal(got["count"], cnt)
        np.testing.assert_array_equal(got["occupied"], (src >= 0).sum(axis=(1, 2, 3)))
        flat = np.concatenate([f.reshape(N, -1, 3) for f in rgb], axis=1)
        want = np.zeros((N, 4, Dz, Dy, Dx), np.uint8)
        for e in range(N):
            for z, y, x in np.argwhere(src[e] >= 0):
                want[e, 0, z, y, x] = 255
                want[e, 1:, z, y, x] = flat[e, src[e, z, y, x]]
        if dtype == "float32":
            want = want.astype(F32) * F32(1 / 255)
        assert got["voxels"].dtype == want.dtype
        np.testing.assert_array_equal(got["voxels"].view(np.uint32 if dtype == "float32" else np.uint8), want.view(np.uint32 if dtype == "float32" else np.uint8))
        # both slots see every voxel; slot 0 wins wherever its pixel is a candidate
        s0 = src[src >= 0] < H * W
        assert s0.any() and (~s0).any() and cnt.min() > (src >= 0).sum(axis=(1, 2, 3)).max()
