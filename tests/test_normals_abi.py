"""CPU tests of the surface normals (include/lcr.h: "Surface normals", lcr_enable_normals): the additions to the C ABI (declared, bound, exported; the ABI version stays 7),
the structs against the binding, every refusal that needs no device, VecSim's and the adapters' ValueErrors before any device call, the keyword through ShardedVecSim, and
the numpy model the GPU tests compare against (tests/normals_ref.py) held to the CPU ray caster: the face the rule gives a box pixel is the face the slab test's ray ENTERS
the box by.

The comparison with the ray caster.  The 8 seed-17 states of tests/test_image_planes_abi._states for push, stack, pick_place and reach, both fixed cameras, at 240 x 320,
64 x 64 and 16 x 16; planes from the fp32 twin of tests/planes_ref.py, boxes from oracle.render_oracle.scene rounded to float32.  The entry face of the slab test is the
argmax of the per-axis entry parameters, its side the sign of the ray in the box frame (fp64).  The model's face must equal it at every box pixel whose margin -- the
largest e minus the second largest -- is at least 1e-5 m, about ten float32 roundings of half-metre coordinates; at most 0.25 % of the box pixels may lie below that margin
and be left out.  Measured here: 443 845 box pixels, no mismatch at any margin, 278 (0.063 %) below the margin."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import normals_ref, planes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_normals_check", "lcr_enable_normals", "lcr_get_normals"]
CTYPES = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
TASKS = ["push", "stack", "pick_place", "reach"]
CAMS = ("camera_front", "camera_top")
SIZES = [(240, 320), (64, 64), (16, 16)]
MARGIN, MAX_LEFT_OUT = 1e-5, 0.0025


def _hdr():
    return open(os.path.join(ROOT, "include", "lcr.h")).read()


def _spec(cameras=3, frame=0):
    s = _capi.NormalsSpec()
    s.cameras, s.frame = cameras, frame
    return s


def test_the_three_functions_are_declared_bound_and_exported(hip_lib):
    hdr = _hdr()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"LCR_NORMALS_WORLD = 0\b", hdr) and re.search(r"LCR_NORMALS_CAMERA = 1\b", hdr)
    assert _capi.NORMALS_FRAMES == {"world": 0, "camera": 1}
    assert (_capi.NORMALS_BOXES, _capi.NORMALS_BOX_FLOATS) == (9, 15) == (normals_ref.N_BOXES, normals_ref.BOX_FLOATS)


def test_the_header_section_pins_the_rule():
    hdr = _hdr()
    section = hdr[hdr.index("== Surface normals"):hdr.index("typedef struct lcr_normals_spec {")]
    for what in ("i = seg & 0x7F", "The marker bit is ignored", "w = 1 + 2 axis + side", "the floor is w = 5", "(0, 0, 127, 5)", "u     = p - c",
                 "fmaf(u.x, A_k.x, fmaf(u.y, A_k.y, u.z * A_k.z))", "e_k   = |l_k| - h_k", "e_0 >= e_1 && e_0 >= e_2 ? 0 : e_1 >= e_2 ? 1 : 2", "l_axis < 0.0f",
                 "clamp((int)rintf(127.0f * component), -127, 127)", "fmaf(n.x, C.x, fmaf(n.y, C.y, n.z * C.z))", "[9][15][N]", "depth_far belongs beyond the scene",
                 "LCR_WRIST_GUARD_BYTE", "LCR_ERR_OOM", "307 200 bytes"):
        assert what in section, what
    for what in ("float output", "terminal planes", "recorder", "a normals channel of the stack or the cloud", "the marker's own faces"):
        assert what in section, what   # the header says what the normals do not do


def _parse(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s+(.*)$", decl, flags=re.S)
        assert m, decl
        for item in m.group(3).split(","):
            item = item.strip()
            if item.startswith("*"):
                ct = ctypes.c_void_p
            elif m.group(2) == "lcr_normals_spec":
                ct = _capi.NormalsSpec
            else:
                ct = CTYPES[m.group(2)]
            fields.append((item.lstrip("* "), ct))
    return fields


def test_the_structs_match_the_header_field_by_field():
    hdr = _hdr()
    for name, bound, size in (("lcr_normals_spec", _capi.NormalsSpec, 8), ("lcr_normals_view", _capi.LcrNormalsView, 72)):
        fields = _parse(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in fields] == [n for n, _ in bound._fields_], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)
    assert [n for n, _ in _capi.LcrNormalsView._fields_] == ["enabled", "spec", "slots", "image_width", "image_height", "normals_front", "normals_top", "normals_wrist",
                                                            "boxes", "camera_pose", "bytes_per_env"]
    # the object boxes' structs keep their sizes
    assert ctypes.sizeof(_capi.ObjectBoxesSpec) == 76 and ctypes.sizeof(_capi.LcrObjectBoxesView) == 112


def test_check_and_enable_refuse_bad_specs_before_they_look_at_the_handle(hip_lib):
    L, bad = hip_lib, _capi.LCR_ERR_INVALID
    for f in (lambda sp: L.lcr_normals_check(ctypes.byref(sp)), lambda sp: L.lcr_enable_normals(None, ctypes.byref(sp))):
        for cams in (8, 9, 0x80000000):
            assert f(_spec(cameras=cams)) == bad
            assert L.lcr_last_error().startswith(b"cameras") and str(cams).encode() in L.lcr_last_error(), L.lcr_last_error()
        for frame in (2, -1):
            assert f(_spec(frame=frame)) == bad
            assert L.lcr_last_error().startswith(b"frame") and str(frame).encode() in L.lcr_last_error(), L.lcr_last_error()
    assert L.lcr_normals_check(None) == bad and b"spec is NULL" in L.lcr_last_error()
    assert L.lcr_enable_normals(None, None) == bad and b"spec is NULL" in L.lcr_last_error()
    for good in (_spec(0, 0), _spec(7, 1), _spec(4, 0), _spec(1, 1)):
        assert L.lcr_normals_check(ctypes.byref(good)) == 0, L.lcr_last_error()
        assert L.lcr_enable_normals(None, ctypes.byref(good)) == bad and b"sim is NULL" in L.lcr_last_error()   # the handle behind the spec
    assert L.lcr_get_normals(None, ctypes.byref(_capi.LcrNormalsView())) == bad
    assert L.lcr_get_normals(None, None) == bad
    # normals are no third plane bit
    assert L.lcr_enable_image_planes(None, 4, 10.0) == bad and b"planes" in L.lcr_last_error()


def test_vecsim_and_the_adapters_refuse_before_lcr_create(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecenv import LowCostRobotVecEnv, LowCostRobotVectorEnv

    def no_device(*a, **k):
        raise AssertionError("lcr_create was reached")

    class Guard:   # the loaded library with lcr_create replaced: the refusals below must come before it is asked for a device
        def __getattr__(self, name):
            return no_device if name == "lcr_create" else getattr(hip_lib, name)

    monkeypatch.setattr(_capi, "load", lambda: Guard())
    both = dict(observation_mode="both", image_planes=("depth", "segmentation"))
    for kw, word in ((dict(surface_normals=True), "image observations"),
                     (dict(surface_normals=True, observation_mode="both"), "the depth plane is missing"),
                     (dict(surface_normals=True, observation_mode="both", image_planes=("segmentation",)), "the depth plane is missing"),
                     (dict(surface_normals=True, observation_mode="both", image_planes=("depth",)), "the segmentation plane is missing"),
                     (dict(surface_normals=dict(cameras=("front", "wrist")), **both), "no wrist_camera"),
                     (dict(surface_normals=dict(cameras=("side",)), **both), "cameras"),
                     (dict(surface_normals=dict(cameras=()), **both), "cameras"),
                     (dict(surface_normals=dict(cameras="front"), **both), "cameras"),
                     (dict(surface_normals=dict(frame="object"), **both), "frame must be 'world' or 'camera'"),
                     (dict(surface_normals=dict(frame=1), **both), "frame must be 'world' or 'camera'"),
                     (dict(surface_normals=dict(float=True), **both), "unknown surface_normals fields"),
                     (dict(surface_normals=3, **both), "surface_normals must be None, True or a dict")):
        with pytest.raises(ValueError, match=re.escape(word)):
            VecSim("reach", 4, **kw)
    for Adapter in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        for spec in (True, dict(frame="camera")):
            with pytest.raises(ValueError, match="surface_normals is for on-device loops over VecSim"):
                Adapter("reach", 4, surface_normals=spec, **both)
    assert _capi.NormalsSpec.from_any(True).as_dict() == {"cameras": ("front", "top"), "frame": "world"}
    assert _capi.NormalsSpec.from_any({}, wrist=True).as_dict() == {"cameras": ("front", "top", "wrist"), "frame": "world"}
    assert _capi.NormalsSpec.from_any(dict(cameras=("top",), frame="camera")).as_dict() == {"cameras": ("top",), "frame": "camera"}


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
    spec = dict(cameras=("front",), frame="camera")
    sharding.ShardedVecSim("push", 128, [0, 0], observation_mode="both", image_planes=("depth", "segmentation"), surface_normals=spec)
    assert len(made) == 2 and all(n == 64 and kw["surface_normals"] is spec for _, n, kw in made)
    assert [kw["env_id_offset"] for _, _, kw in made] == [0, 64]


# ---- the rule against the ray caster ----

def oracle_boxes(task, qpos, target=None):
    """the nine opaque boxes of oracle.render_oracle.scene as the model reads them: (9, 15) float64 -- c, X, Y, Z, h; zeros for a second cube the task does not have"""
    from oracle import render_oracle

    out = np.zeros((9, 15))
    opaque = [b for b in render_oracle.scene(task, qpos, target)[1] if b[4] >= 1.0]
    assert len(opaque) == (9 if task == "stack" else 8)
    for k, (bc, R, bh, _col, _alpha) in enumerate(opaque):
        out[k, 0:3] = bc
        out[k, 3:12] = np.asarray(R).T.reshape(-1)   # the columns of R are the box axes
        out[k, 12:15] = bh
    return out


def oracle_pose(task, cam, H):
    """ro, X, Y, Z, s of a fixed camera as the library lays a pose out: (13,) float64"""
    from oracle import render_oracle

    pos, X, Y, Z = render_oracle.camera(task, cam)
    return np.concatenate([pos, X, Y, Z, [2.0 * np.tan(np.radians(45.0) / 2) / H]])


def entry_face(seg, boxes, pose, H, W):
    """the face the slab test's ray enters its box by, in fp64, at every box pixel of seg: the argmax of the per-axis entry parameters, the side from the sign of the ray in
    the box frame -> (face code 1 .. 6 (H, W) int64, 0 where the pixel shows no box)"""
    pos, X, Y, Z, s = pose[0:3], pose[3:6], pose[6:9], pose[9:12], pose[12]
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx = ((u + 0.5 - 0.5 * W) * s)[..., None]
    sy = (-(v + 0.5 - 0.5 * H) * s)[..., None]
    d = sx * X + sy * Y - Z
    ids = (seg & 0x7F).astype(int)
    code = np.zeros((H, W), np.int64)
    for b in range(9):
        m = ids == b + 2
        if not m.any():
            continue
        R = boxes[b, 3:12].reshape(3, 3).T
        ol = R.T @ (pos - boxes[b, 0:3])
        dl = d[m] @ R
        dls = np.where(np.abs(dl) > 1e-9, dl, 1e-9)
        t1 = (-boxes[b, 12:15] - ol) / dls; t2 = (boxes[b, 12:15] - ol) / dls
        axis = np.minimum(t1, t2).argmax(-1)
        side = np.take_along_axis(dl, axis[:, None], 1)[:, 0] > 0     # a ray that travels along + axis enters by the negative face
        code[m] = 1 + 2 * axis + side
    return code


@functools.lru_cache(maxsize=None)
def _census(task, size):
    """-> (box pixels, pixels below the margin, mismatches at or above it, mismatches at any margin, faces seen)"""
    from tests.test_image_planes_abi import _states

    H, W = size
    qpos, target = _states(task)
    n_box = n_low = n_bad = n_bad_any = 0
    seen = set()
    for e in range(qpos.shape[1]):
        boxes = oracle_boxes(task, qpos[:, e], target[:, e])
        for cam in CAMS:
            depth, seg = planes_ref.planes(task, qpos[:, e], target[:, e], cam, W, H, dtype=np.float32)
            pose = oracle_pose(task, cam, H)
            out, index, margin = normals_ref.planes(depth[None], seg[None], boxes.astype(np.float32)[:, :, None], pose.astype(np.float32)[:, None], "world", detail=True)
            want = entry_face(seg, boxes, pose, H, W)
            box = want > 0
            got = out[0, ..., 3].astype(np.int64)
            # the floor and the sky, wherever they show
            ids = seg & 0x7F
            assert (out[0][ids == 1] == (0, 0, 127, 5)).all() and (out[0][ids == 0] == 0).all()
            clear = margin[0] >= np.float32(MARGIN)
            n_box += int(box.sum()); n_low += int((box & ~clear).sum())
            n_bad += int((box & clear & (got != want)).sum()); n_bad_any += int((box & (got != want)).sum())
            seen |= set(np.unique(got[box]).tolist())
    return n_box, n_low, n_bad, n_bad_any, seen


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", TASKS)
def test_the_rule_gives_the_face_the_ray_enters_by(task, size):
    n_box, n_low, n_bad, n_bad_any, seen = _census(task, size)
    print(f"[normals vs slab test] {task} {size[0]}x{size[1]}: {n_box} box pixels, {n_low} below the {MARGIN} m margin, {n_bad} mismatches at or above it, {n_bad_any} at any margin, "
          f"faces {sorted(seen)}")
    assert n_box > 0 and n_bad == 0
    assert n_low <= MAX_LEFT_OUT * n_box
    assert len(seen) >= 2   # the camera above sees + Z faces, the camera in front sees sides: more than one face code, or the comparison compares nothing


def test_the_floor_the_sky_and_ids_the_planes_never_hold():
    seg = np.array([[0, 1, 0x81, 0x80], [11, 127, 1, 0]], np.uint8)
    depth = np.full((2, 4), 3.0, np.float32)
    pose = oracle_pose("reach", "camera_front", 2).astype(np.float32)
    out = normals_ref.plane(depth, seg, np.zeros((9, 15), np.float32), pose, "world")
    assert out.dtype == np.int8 and out.shape == (2, 4, 4)
    assert out[0].tolist() == [[0, 0, 0, 0], [0, 0, 127, 5], [0, 0, 127, 5], [0, 0, 0, 0]]     # the marker bit is ignored: floor under the marker, sky under the marker
    assert out[1].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 127, 5], [0, 0, 0, 0]]       # ids above 10: four zeros


@pytest.mark.parametrize("cam", CAMS)
def test_the_camera_frame_is_the_world_normal_rotated_and_requantised(cam):
    """a box face in the camera frame: dot(n, C_axis) of the UNquantised world normal for the camera's X, Y, Z, then quantised; the face code does not change.  The floor seen
    by a camera is (rint(127 X.z), rint(127 Y.z), rint(127 Z.z), 5)"""
    from tests.test_image_planes_abi import _states

    H, W = 64, 64
    qpos, target = _states("stack")
    boxes = oracle_boxes("stack", qpos[:, 0], target[:, 0]).astype(np.float32)
    pose = oracle_pose("stack", cam, H).astype(np.float32)
    depth, seg = planes_ref.planes("stack", qpos[:, 0], target[:, 0], cam, W, H, dtype=np.float32)
    world = normals_ref.plane(depth, seg, boxes, pose, "world")
    camera = normals_ref.plane(depth, seg, boxes, pose, "camera")
    np.testing.assert_array_equal(world[..., 3], camera[..., 3])
    ids = seg & 0x7F
    C = pose[3:12].reshape(3, 3).astype(np.float64)          # rows: the camera's X, Y, Z in the world
    floor = np.rint(127.0 * C[:, 2]).astype(np.int8)
    assert (ids == 1).any() and (camera[ids == 1] == (*floor, 5)).all()
    assert ((ids >= 2).sum() > 50)
    checked = 0
    for b in range(9):
        for w in range(1, 7):
            m = (ids == b + 2) & (world[..., 3] == w)
            if not m.any():
                continue
            n = boxes[b, 3 + 3 * ((w - 1) >> 1): 6 + 3 * ((w - 1) >> 1)].astype(np.float64) * (-1.0 if (w - 1) & 1 else 1.0)
            assert (world[m][:, :3] == np.rint(127.0 * n).astype(np.int8)).all()
            want = 127.0 * (C @ n)                               # fp64; the model's float32 chain is within 127 * 3 ulp of it
            got = camera[m][:, :3].astype(np.float64)
            assert (got == got[0]).all() and (np.abs(got[0] - want) <= 0.5 + 1e-4).all(), (b, w, got[0], want)
            # rotating the QUANTISED world normal instead loses up to 0.5 a component before the rotation: not the rule, but close
            assert (np.abs(C @ world[m][0, :3].astype(np.float64) - got[0]) <= 0.5 * np.sqrt(3) + 0.5 + 1e-4).all()
            checked += 1
    assert checked >= 4
    assert np.abs(np.linalg.norm(camera[ids >= 2][:, :3].astype(np.float64), axis=1) - 127.0).max() <= np.sqrt(3) * 0.5 + 1e-3   # unit normals, to the quantisation
