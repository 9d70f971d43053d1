"""CPU tests of the point cloud (include/lcr.h: lcr_enable_point_cloud): the additions to the C ABI (declared, bound, exported; the ABI version and every existing struct stay
as they are), the refusals that need no device, VecSim's ValueErrors before any device call, and the properties of the numpy model the GPU tests compare against
(tests/cloud_ref.py): the selection rule for M = P, 0 < M < P and M = 0, the 64-bit index, and the unprojection on a synthetic camera."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import cloud_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_point_cloud_check", "lcr_enable_point_cloud", "lcr_get_point_cloud"]
CTYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "const float *": ctypes.c_void_p, "const int32_t *": ctypes.c_void_p,
          "lcr_point_cloud_spec": _capi.PointCloudSpec}


def _parse_struct(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const float \*|const int32_t \*|int32_t|uint32_t|uint64_t|lcr_point_cloud_spec)\s*(.*)$", decl, flags=re.S)
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
    assert re.search(r"#define\s+LCR_CLOUD_DEFAULT_IDS\s+0x7FCu\b", hdr) and _capi.CLOUD_DEFAULT_IDS == 0x7FC == cloud_ref.DEFAULT_IDS
    assert _capi.CLOUD_IDS == cloud_ref.IDS == {"floor": 2, "arm": 0x1FC, "cube": 0x200, "cube2": 0x400}
    assert _capi.CLOUD_IDS["arm"] | _capi.CLOUD_IDS["cube"] | _capi.CLOUD_IDS["cube2"] == _capi.CLOUD_DEFAULT_IDS
    assert tuple(_capi.STACK_CAMERAS) == cloud_ref.CAMERAS
    for what in ("a crop box", "farthest-point sampling", "normals", "a base-frame transform", "the cloud of an episode that has ended"):
        assert what in hdr, what   # the header says what is not in the feature


def test_the_existing_structs_are_unchanged(hip_lib):
    cfg = _capi.LcrConfig()
    assert hip_lib.lcr_config_default(ctypes.byref(cfg), 0) == 0
    assert cfg.struct_size == ctypes.sizeof(_capi.LcrConfig) == 200
    assert ctypes.sizeof(_capi.LcrObsView) == 64 and ctypes.sizeof(_capi.LcrPlanesView) == 48
    assert ctypes.sizeof(_capi.LookVariant) == 136 and ctypes.sizeof(_capi.LookSampler) == 80
    assert ctypes.sizeof(_capi.WristCamera) == 44 and ctypes.sizeof(_capi.LcrWristView) == 88
    assert ctypes.sizeof(_capi.ObsStackSpec) == 16 and ctypes.sizeof(_capi.LcrObsStackView) == 48


def test_cloud_structs_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    for name, bound, size in (("lcr_point_cloud_spec", _capi.PointCloudSpec, 16), ("lcr_point_cloud_view", _capi.LcrPointCloudView, 80)):
        fields = _parse_struct(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in bound._fields_] == [n for n, _ in fields], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)


def _spec(points=1024, cameras=0, ids=0, colors=0):
    return _capi.PointCloudSpec(points=points, cameras=cameras, ids=ids, colors=colors)


BAD = [("points", dict(points=0)), ("points", dict(points=63)), ("points", dict(points=100)), ("points", dict(points=8256)), ("points", dict(points=-64)),
       ("cameras", dict(cameras=8)), ("cameras", dict(cameras=0x13)), ("ids", dict(ids=1)), ("ids", dict(ids=0x7FD)), ("ids", dict(ids=1 << 11)), ("ids", dict(ids=0xFFC)),
       ("colors", dict(colors=2)), ("colors", dict(colors=-1))]


@pytest.mark.parametrize("field,over", BAD, ids=[f"{f}-{i}" for i, (f, _) in enumerate(BAD)])
def test_a_bad_spec_is_refused_before_the_handle_is_looked_at(hip_lib, field, over):
    assert hip_lib.lcr_point_cloud_check(ctypes.byref(_spec(**over))) == _capi.LCR_ERR_INVALID
    msg = hip_lib.lcr_last_error()
    assert msg.startswith(field.encode()), (field, msg)
    assert hip_lib.lcr_enable_point_cloud(None, ctypes.byref(_spec(**over))) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_last_error() == msg and b"sim is NULL" not in msg


def test_valid_specs_reach_the_handle_check_and_null_handles_are_refused(hip_lib):
    for sp in (_spec(), _spec(64, 1, 2, 1), _spec(8192, 7, 0x7FE, 0), _spec(128, 4, 1 << 10, 1)):
        assert hip_lib.lcr_point_cloud_check(ctypes.byref(sp)) == 0
        assert hip_lib.lcr_enable_point_cloud(None, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID and b"sim is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_point_cloud_check(None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_enable_point_cloud(None, None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_get_point_cloud(None, None) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_get_point_cloud(None, ctypes.byref(_capi.LcrPointCloudView())) == _capi.LCR_ERR_INVALID


def test_vecsim_checks_the_cloud_before_device_use(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, LowCostRobotVectorEnv, VecSim

    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())
    both = dict(observation_mode="both", image_planes=("depth", "segmentation"))
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, point_cloud=1024)   # state-only observations
    with pytest.raises(ValueError, match="observation_mode"):
        VecSim("reach", 4, observation_mode="state", point_cloud={"points": 64})
    for planes in ((), ("depth",), ("segmentation",)):
        with pytest.raises(ValueError, match=r"pass both.*image_planes=\('depth', 'segmentation'\)"):
            VecSim("reach", 4, observation_mode="both", image_planes=planes, point_cloud=1024)
    with pytest.raises(ValueError, match="wrist"):
        VecSim("reach", 4, point_cloud={"cameras": ("front", "wrist")}, **both)
    for bad, what in ((0, "points"), (63, "points"), (100, "points"), (8256, "points"), (True, "point_cloud must be"), ("64", "point_cloud must be"), (64.0, "point_cloud must be"),
                      ({"points": 128.0}, "points"), ({"cameras": ("side",)}, "cameras"), ({"cameras": "front"}, "cameras"), ({"cameras": ()}, "cameras"),
                      ({"ids": ("sky",)}, "ids"), ({"ids": (0,)}, "ids"), ({"ids": (11,)}, "ids"), ({"ids": "arm"}, "ids"), ({"ids": ()}, "ids"), ({"colors": 2}, "colors"),
                      ({"points": 64, "normals": True}, "unknown point_cloud fields")):
        with pytest.raises(ValueError, match=what):
            VecSim("reach", 4, point_cloud=bad, **both)
    # (valid values pass the checks: the constructor then goes on to lcr_create)
    for good in (64, 8192, {"points": 256, "cameras": ("top",), "ids": ("arm", "cube", "cube2", "floor"), "colors": True}, {"ids": [9, 10]}, {}):
        with pytest.raises(AssertionError, match="lcr_create was reached"):
            VecSim("reach", 4, point_cloud=good, **both)
    with pytest.raises(AssertionError, match="lcr_create was reached"):
        VecSim("reach", 4, wrist_camera=True, point_cloud={"cameras": ("wrist",)}, **both)
    # the vector adapters do not expose the cloud
    for cls in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        with pytest.raises(ValueError, match="terminal_observation"):
            cls("reach", 4, point_cloud=64, **both)
    sp = _capi.PointCloudSpec.from_any({"points": 256, "cameras": ("wrist", "front"), "ids": ("cube", "floor", 3), "colors": True})
    assert (sp.points, sp.cameras, sp.ids, sp.colors) == (256, 5, (1 << 9) | (1 << 1) | (1 << 3), 1)
    assert sp.as_dict() == {"points": 256, "cameras": ("front", "wrist"), "ids": (1, 3, 9), "colors": True}
    sp = _capi.PointCloudSpec.from_any(1024)
    assert (sp.points, sp.cameras, sp.ids, sp.colors) == (1024, 0, 0, 0)


# ---- the model ----

def test_selection_identity_repeats_and_empty():
    """M = P is the identity; 0 < M < P uses every candidate at least floor(P / M) times, monotonically; M >= P is strictly increasing with strides floor(M / P) or that
    plus one; M = 0 gives -1"""
    for P in (64, 128, 8192):
        np.testing.assert_array_equal(cloud_ref.select(P, P), np.arange(P))
        for M in (1, 2, 3, 63, P // 2, P - 1):
            idx = cloud_ref.select(M, P)
            assert idx[0] == 0 and idx[-1] == M - 1 and (np.diff(idx) >= 0).all() and (np.diff(idx) <= 1).all()
            assert np.bincount(idx, minlength=M).min() >= P // M, (M, P)
        for M in (P + 1, 2 * P - 1, 3 * P + 5, 786432):
            idx = cloud_ref.select(M, P)
            d = np.diff(idx)
            assert 0 <= idx[0] and idx[-1] < M and (d >= M // P).all() and (d <= M // P + 1).all(), (M, P)
        assert (cloud_ref.select(0, P) == -1).all()


def test_the_index_needs_64_bits():
    """P = 8192 and M = 786 432 (three 512 x 512 cameras, every pixel a candidate): (2 j + 1) M passes 2^32; a 32-bit product picks other candidates"""
    P, M = 8192, 3 * 512 * 512
    j = np.arange(P, dtype=np.uint64)
    assert int((2 * j[-1] + 1) * np.uint64(M)) > 2 ** 32
    want = cloud_ref.select(M, P)
    np.testing.assert_array_equal(want, ((2 * j + 1) * np.uint64(M) // np.uint64(2 * P)).astype(np.int64))
    np.testing.assert_array_equal(want, 96 * np.arange(P) + 48)
    wrapped = (((2 * j + 1) * np.uint64(M)) & np.uint64(0xFFFFFFFF)) // np.uint64(2 * P)
    assert (wrapped.astype(np.int64) != want).any()


def _synthetic(rng, N, H, W, slots):
    seg = [rng.integers(0, 11, (N, H, W)).astype(np.uint8) | (rng.random((N, H, W)) < 0.1).astype(np.uint8) * 0x80 for _ in range(slots)]
    depth = [rng.uniform(0.2, 1.5, (N, H, W)).astype(np.float32) for _ in range(slots)]
    rgb = [rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8) for _ in range(slots)]
    poses = np.zeros((slots, 13, N), np.float32)
    for s in range(slots):
        for e in range(N):
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if np.linalg.det(Q) < 0:
                Q[:, 2] = -Q[:, 2]
            poses[s, 0:3, e] = rng.uniform(-0.5, 0.6, 3)
            poses[s, 3:12, e] = Q.T.reshape(-1)     # X, Y, Z: the rows of Q^T are orthonormal
            poses[s, 12, e] = 2 * np.tan(np.radians(rng.uniform(30, 60)) / 2) / H
    return depth, seg, rgb, poses


def test_model_on_synthetic_planes():
    rng = np.random.default_rng(0)
    N, H, W, slots, P = 4, 8, 12, 2, 64
    depth, seg, rgb, poses = _synthetic(rng, N, H, W, slots)
    seg[0][1] = 1; seg[1][1] = 0x80   # env 1: floor and sky (with the marker bit) only: M = 0 for the default ids
    seg[0][2] = 0; seg[1][2] = 0; seg[1][2, 3, 5] = 9 | 0x80; seg[1][2, 7, 11] = 4   # env 2: two candidates, one under the marker
    pts, count, source = cloud_ref.cloud(depth, seg, rgb, poses, dict(points=P, ids=0, colors=True))
    assert pts.shape == (N, P, 6) and count.shape == (N,) and source.shape == (N, P)
    assert count[1] == 0 and (source[1] == -1).all() and not pts[1].any()
    assert count[2] == 2 and set(source[2]) == {H * W + 3 * W + 5, H * W + 7 * W + 11} and (np.diff(source[2]) >= 0).all() and (source[2] == source[2][0]).sum() == P // 2
    flat = np.concatenate([s.reshape(N, -1) for s in seg], axis=1) & 0x7F
    for e in (0, 3):
        cand = np.flatnonzero(flat[e] >= 2)
        assert count[e] == cand.size > P
        np.testing.assert_array_equal(source[e], cand[cloud_ref.select(cand.size, P)])
    # a point re-projects to its pixel: in camera coordinates it is t (sx, sy, -1).  The axes are float32 numbers, orthonormal to 2^-24 per component only: the
    # products below are off by at most 3 x 2^-24 x |p - ro| (< 3 m) x 3 terms < 2e-6
    for e, j in ((0, 0), (0, P - 1), (3, 17), (2, 40)):
        sl, pix = divmod(int(source[e, j]), H * W)
        row, px = divmod(pix, W)
        ro, R, s = poses[sl, 0:3, e].astype(float), poses[sl, 3:12, e].astype(float).reshape(3, 3), float(poses[sl, 12, e])
        pc = R @ (pts[e, j, :3] - ro)
        t = float(depth[sl][e, row, px])
        np.testing.assert_allclose(pc, [t * (px + 0.5 - 0.5 * W) * s, -t * (row + 0.5 - 0.5 * H) * s, -t], rtol=0, atol=2e-6)
        np.testing.assert_array_equal(pts[e, j, 3:].astype(np.float32).view(np.uint32), (rgb[sl][e, row, px].astype(np.float32) * np.float32(1 / 255)).view(np.uint32))
    # other ids: the floor alone; without colours the channels are x y z
    p3, c3, s3 = cloud_ref.cloud(depth, seg, None, poses, dict(points=P, ids=2))
    assert p3.shape == (N, P, 3) and c3[1] == H * W and (s3[1] < H * W).all()
    b = cloud_ref.xyz_bound(depth, poses, source, H, W)
    assert b.shape == (N, P) and (b > 0).all() and b.max() < 1e-5
