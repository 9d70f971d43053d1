"""CPU tests of the object boxes (include/lcr.h: "Object boxes", lcr_enable_object_boxes): the additions to the C ABI (declared, bound, exported; the ABI version stays 7),
the structs against the binding, what the header's section says, every refusal that needs no device with the field named, VecSim's and the adapters' ValueErrors before any
device call, the keyword through ShardedVecSim, and the numpy model the GPU tests compare against (tests/boxes_ref.py) on hand-made planes whose records are written down
here by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_lowcostrobot_amd import _capi
from tests import boxes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lcr_object_boxes_check", "lcr_enable_object_boxes", "lcr_get_object_boxes"]
CTYPES = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
MARKER = 0x80000000
CUBE, CUBE2, FLOOR, ARM = 1 << 9, 1 << 10, 1 << 1, 0x7F << 2


def _hdr():
    return open(os.path.join(ROOT, "include", "lcr.h")).read()


def _spec(objects=(ARM, CUBE), cameras=3, depth=0, n_objects=None):
    s = _capi.ObjectBoxesSpec()
    s.cameras, s.depth = cameras, depth
    for i, m in enumerate(objects):
        s.objects[i] = m
    s.n_objects = len(objects) if n_objects is None else n_objects
    return s


def test_the_new_functions_are_declared_bound_and_exported(hip_lib):
    hdr = _hdr()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.lcr_abi_version() == 7 and _capi.ABI_VERSION == 7
    assert re.search(r"#define\s+LCR_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"#define\s+LCR_BOXES_MAX_OBJECTS\s+16\b", hdr) and re.search(r"#define\s+LCR_BOXES_MARKER\s+0x80000000u", hdr)
    assert _capi.BOXES_MAX_OBJECTS == 16 and _capi.BOXES_MARKER == MARKER
    assert _capi.BOXES_FIELDS == ("x0", "y0", "x1", "y1", "count", "sum_x", "sum_y", "nearest") == boxes_ref.FIELDS
    assert _capi.BOXES_OBJECTS == boxes_ref.NAMES and _capi.BOXES_OBJECTS["link_6"] == 1 << 8 and _capi.BOXES_OBJECTS["base_link"] == 1 << 2
    assert _capi.BOXES_DEFAULT_OBJECTS == ("arm", "cube", "cube2", "marker")


def test_the_header_section_says_what_the_record_is_and_what_is_not_in_it():
    hdr = _hdr()
    section = hdr[hdr.index("== Object boxes"):hdr.index("typedef struct lcr_object_boxes_spec {")]
    for what in ("((m >> (b & 0x7f)) & 1) != 0", "(m & LCR_BOXES_MARKER) && (b & 0x80)", "x0 = min c", "y0 = min r", "x1 = max c + 1", "y1 = max r + 1",
                 "count = the number of matching pixels", "sum_x = the sum of c", "sum_y = the sum of r", "nearest", "compared as uint32",
                 "all eight are zero", "count == 0", "[N][slots][O][8]", "front,\n *               top, wrist", "INTEGERS", "LCR_ERR_OOM"):
        assert what in section, what
    for what in ("amodal boxes", "oriented boxes", "instances beyond the surface ids", "a normalised float form", "the recorder", "an episode that has ended", "no _terminal call"):
        assert what in section, what   # the header says what the boxes do not do
    for i, name in enumerate(_capi.BOXES_FIELDS):
        assert re.search(r"LCR_BOXES_%s = %d\b" % (name.upper(), i), hdr), name


def _parse(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    consts = {"LCR_BOXES_MAX_OBJECTS": 16}
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
            a = re.match(r"(\*?)(\w+)(?:\[(\w+)\])?$", item)
            assert a, decl
            if ptr or a.group(1):
                ct = ctypes.c_void_p
            elif typ == "lcr_object_boxes_spec":
                ct = _capi.ObjectBoxesSpec
            else:
                ct = CTYPES[typ]
            dim = a.group(3)
            fields.append((a.group(2), ct * int(consts.get(dim, dim)) if dim else ct))
    return fields


def test_the_structs_match_the_header():
    hdr = _hdr()
    for name, bound, size in (("lcr_object_boxes_spec", _capi.ObjectBoxesSpec, 76), ("lcr_object_boxes_view", _capi.LcrObjectBoxesView, 112)):
        fields = _parse(hdr, name)
        Parsed = type("Parsed", (ctypes.Structure,), {"_fields_": fields})
        assert ctypes.sizeof(Parsed) == ctypes.sizeof(bound) == size, name
        assert [n for n, _ in fields] == [n for n, _ in bound._fields_], name
        for n, _ in fields:
            assert getattr(Parsed, n).offset == getattr(bound, n).offset and getattr(Parsed, n).size == getattr(bound, n).size, (name, n)
    # the heightmap's structs keep their sizes
    assert ctypes.sizeof(_capi.HeightmapSpec) == 48 and ctypes.sizeof(_capi.LcrHeightmapView) == 128


def test_the_check_refuses_by_name(hip_lib):
    L = hip_lib
    bad = _capi.LCR_ERR_INVALID
    for n in (0, 17, -1):
        assert L.lcr_object_boxes_check(ctypes.byref(_spec(n_objects=n))) == bad
        msg = L.lcr_last_error()
        assert msg.startswith(b"n_objects") and b"1 .. 16" in msg and str(n).encode() in msg, msg
    for objects, i, word in (((ARM, 0), 1, b"is empty"), ((0,), 0, b"is empty"), ((CUBE, ARM, CUBE | 1), 2, b"bit 0"), ((1,), 0, b"bit 0"),
                             ((1 << 11,), 0, b"bits 11 .. 30"), ((ARM, CUBE | 1 << 30), 1, b"bits 11 .. 30"), ((MARKER | 1 << 20,), 0, b"bits 11 .. 30")):
        assert L.lcr_object_boxes_check(ctypes.byref(_spec(objects))) == bad, objects
        msg = L.lcr_last_error()
        assert msg.startswith(b"objects[%d]" % i) and word in msg, (objects, msg)
    for cams in (0, 8, 9):
        assert L.lcr_object_boxes_check(ctypes.byref(_spec(cameras=cams))) == bad
        assert L.lcr_last_error().startswith(b"cameras") and str(cams).encode() in L.lcr_last_error(), L.lcr_last_error()
    for depth in (2, -1):
        assert L.lcr_object_boxes_check(ctypes.byref(_spec(depth=depth))) == bad
        assert L.lcr_last_error().startswith(b"depth") and b"0 or 1" in L.lcr_last_error(), L.lcr_last_error()
    assert L.lcr_object_boxes_check(None) == bad and b"spec is NULL" in L.lcr_last_error()
    # the accepted extremes: one object and sixteen, every camera, the marker alone, every id with the marker, overlapping objects; masks beyond n_objects are not looked at
    for good in (_spec((MARKER,), 1), _spec((0x7FE | MARKER,) * 16, 7, 1), _spec((ARM, 1 << 8, CUBE, CUBE | CUBE2), 4), _spec((CUBE, 0, 1), n_objects=1)):
        assert L.lcr_object_boxes_check(ctypes.byref(good)) == 0, L.lcr_last_error()


def test_a_null_handle_is_refused_behind_the_spec(hip_lib):
    L = hip_lib
    assert L.lcr_enable_object_boxes(None, ctypes.byref(_spec())) == _capi.LCR_ERR_INVALID and b"sim is NULL" in L.lcr_last_error()
    assert L.lcr_enable_object_boxes(None, None) == _capi.LCR_ERR_INVALID and b"spec is NULL" in L.lcr_last_error()
    assert L.lcr_enable_object_boxes(None, ctypes.byref(_spec((0,)))) == _capi.LCR_ERR_INVALID and L.lcr_last_error().startswith(b"objects[0]")
    assert L.lcr_get_object_boxes(None, ctypes.byref(_capi.LcrObjectBoxesView())) == _capi.LCR_ERR_INVALID
    assert L.lcr_get_object_boxes(None, None) == _capi.LCR_ERR_INVALID


def test_vecsim_and_the_adapters_refuse_before_any_device_call(hip_lib):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecenv import LowCostRobotVecEnv, LowCostRobotVectorEnv

    seg = dict(observation_mode="both", image_planes=("segmentation",))
    for kw, word in ((dict(object_boxes=True), "image observations"),
                     (dict(object_boxes=True, observation_mode="both"), "object_boxes is made of the segmentation plane"),
                     (dict(object_boxes=True, observation_mode="both", image_planes=("depth",)), "object_boxes is made of the segmentation plane"),
                     (dict(object_boxes=dict(depth=True), **seg), "needs the depth plane"),
                     (dict(object_boxes=dict(cameras=("front", "wrist")), **seg), "no wrist_camera"),
                     (dict(object_boxes=dict(objects=("arm", "gripper")), **seg), "objects[1] is 'gripper'"),
                     (dict(object_boxes=dict(objects=("sky",)), **seg), "objects[0] is 'sky'"),
                     (dict(object_boxes=dict(objects=(0,)), **seg), "objects[0] is 0"),
                     (dict(object_boxes=dict(objects=(11,)), **seg), "objects[0] is 11"),
                     (dict(object_boxes=dict(objects=(True,)), **seg), "objects[0] is True"),
                     (dict(object_boxes=dict(objects=(("cube", 2.5),)), **seg), "objects[0]"),
                     (dict(object_boxes=dict(objects=((),)), **seg), "objects[0]"),
                     (dict(object_boxes=dict(objects=()), **seg), "non-empty tuple"),
                     (dict(object_boxes=dict(objects="cube"), **seg), "non-empty tuple"),
                     (dict(object_boxes=dict(objects=("cube",) * 17), **seg), "at most 16"),
                     (dict(object_boxes=dict(cameras=("side",)), **seg), "cameras"),
                     (dict(object_boxes=dict(cameras=()), **seg), "cameras"),
                     (dict(object_boxes=dict(depth=1), **seg), "depth must be a bool"),
                     (dict(object_boxes=dict(normalised=True), **seg), "unknown object_boxes fields"),
                     (dict(object_boxes=4, **seg), "object_boxes must be None, True or a dict")):
        with pytest.raises(ValueError, match=re.escape(word)):
            VecSim("reach", 4, **kw)
    for Adapter in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        for spec in (True, dict(objects=("cube",))):
            with pytest.raises(ValueError, match="object_boxes is for on-device loops over VecSim"):
                Adapter("reach", 4, object_boxes=spec, **seg)
    sp = _capi.ObjectBoxesSpec.from_any(dict(objects=("floor", "arm", 9, ("cube", "cube2"), ("marker", 10), "link_6", [2, "link_1"]), cameras=("top",), depth=True))
    assert sp.as_dict() == {"cameras": ("top",), "objects": ("floor", "arm", 9, ("cube", "cube2"), ("marker", 10), "link_6", (2, "link_1")),
                            "masks": (FLOOR, ARM, CUBE, CUBE | CUBE2, MARKER | CUBE2, 1 << 8, 0b1100), "depth": True}
    # the defaults: the same four objects for every task, every camera the handle has
    assert _capi.ObjectBoxesSpec.from_any(True).as_dict() == {"cameras": ("front", "top"), "objects": ("arm", "cube", "cube2", "marker"), "masks": (ARM, CUBE, CUBE2, MARKER), "depth": False}
    assert _capi.ObjectBoxesSpec.from_any({}, wrist=True).as_dict()["cameras"] == ("front", "top", "wrist")
    assert [boxes_ref.mask_of(o) for o in sp.as_dict()["objects"]] == list(sp.as_dict()["masks"])


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
    spec = dict(objects=("cube", "marker"), depth=True)
    sharding.ShardedVecSim("push", 128, [0, 0], observation_mode="both", image_planes=("depth", "segmentation"), object_boxes=spec)
    assert len(made) == 2 and all(n == 64 and kw["object_boxes"] is spec for _, n, kw in made)
    assert [kw["env_id_offset"] for _, _, kw in made] == [0, 64]


# ---- the model on hand-made planes ----

def _rec(seg, mask, depth=None):
    """the model both ways: record() on the plane, and boxes() on a batch of it"""
    seg = np.asarray(seg, np.uint8)
    one = boxes_ref.record(seg, mask, depth)
    batch = boxes_ref.boxes([seg[None]], [mask], None if depth is None else [np.asarray(depth, np.float32)[None]])
    assert batch.shape == (1, 1, 1, 8) and batch.dtype == np.int32
    np.testing.assert_array_equal(batch[0, 0, 0].view(np.uint32).astype(np.int64), one)
    return one.tolist()


def test_the_model_an_empty_object_and_the_corners():
    seg = np.zeros((12, 20), np.uint8)
    seg[3:5, 2:9] = 4
    assert _rec(seg, CUBE) == [0] * 8                                       # absent: all eight zero
    assert _rec(seg, CUBE, np.ones((12, 20), np.float32)) == [0] * 8        # with depth too
    assert _rec(seg, 1 << 4) == [2, 3, 9, 5, 14, 7 * 2 * 5, 7 * (3 + 4), 0]
    for (r, c) in ((0, 0), (0, 19), (11, 0), (11, 19)):                     # one pixel in each corner, one at a time: the box is that pixel
        one = np.zeros((12, 20), np.uint8)
        one[r, c] = 9
        assert _rec(one, CUBE) == [c, r, c + 1, r + 1, 1, c, r, 0]
    four = np.zeros((12, 20), np.uint8)
    four[[0, 0, 11, 11], [0, 19, 0, 19]] = 9                                # and all four: the whole frame
    assert _rec(four, CUBE) == [0, 0, 20, 12, 4, 38, 22, 0]


def test_the_model_a_run_across_a_row_end_at_width_20():
    """W = 20 is no multiple of 16: pixels 16 .. 31 are one 16-byte chunk of the kernel and lie in rows 0 and 1.  A run over 18 .. 22 is columns 18, 19 of row 0 and 0, 1, 2
    of row 1"""
    seg = np.zeros((16, 20), np.uint8)
    seg.reshape(-1)[18:23] = 10
    assert _rec(seg, CUBE2) == [0, 0, 20, 2, 5, 18 + 19 + 0 + 1 + 2, 3, 0]
    assert _rec(seg, CUBE) == [0] * 8


def test_the_model_the_marker_over_a_cube_pixel_counts_for_both_and_objects_overlap():
    seg = np.zeros((16, 16), np.uint8)
    seg[4:8, 4:8] = 9                      # the cube: 16 pixels
    seg[6:10, 6:10] |= 0x80                # the marker over its lower right 2 x 2, and over sky
    seg[12, 1:4] = 10
    assert _rec(seg, CUBE) == [4, 4, 8, 8, 16, 16 * 5.5, 16 * 5.5, 0]       # the marked cube pixels are still the cube
    assert _rec(seg, MARKER) == [6, 6, 10, 10, 16, 16 * 7.5, 16 * 7.5, 0]   # and the marker too
    both = _rec(seg, CUBE | MARKER)
    assert both[:5] == [4, 4, 10, 10, 28]                                    # a union counts a pixel once
    union, c1, c2 = _rec(seg, CUBE | CUBE2), _rec(seg, CUBE), _rec(seg, CUBE2)
    assert c2 == [1, 12, 4, 13, 3, 6, 36, 0]
    assert union[4:7] == [c1[4] + c2[4], c1[5] + c2[5], c1[6] + c2[6]] and union[:4] == [1, 4, 8, 13]
    # ids the planes never hold select nothing, whatever the mask
    odd = np.full((16, 16), 31, np.uint8)
    odd[0, 0] = 127
    assert _rec(odd, 0x7FE | MARKER) == [0] * 8


def test_the_model_a_full_frame_and_the_nearest_depth():
    seg = np.full((512, 512), 1, np.uint8)
    full = _rec(seg, FLOOR)
    assert full == [0, 0, 512, 512, 262144, 66977792, 66977792, 0] and full[5] == 512 * 512 * 511 // 2 < 2 ** 31
    rng = np.random.default_rng(3)
    depth = rng.uniform(0.05, 10.0, (24, 20)).astype(np.float32)
    seg = rng.choice(np.array([0, 1, 5, 9, 0x89, 0x80], np.uint8), (24, 20))
    for mask in (CUBE, MARKER, ARM, FLOOR | CUBE):
        m = boxes_ref.matches(seg, mask)
        near = _rec(seg, mask, depth)[7]
        # positive floats order as their words do: the minimum word is the word of the minimum depth
        assert m.any() and near == int(np.asarray(depth[m].min(), np.float32).view(np.uint32))
        assert _rec(seg, mask)[7] == 0                                       # without depth: 0
    # a word with the top bit set in the int32 view: the model keeps the bits
    far = np.full((16, 16), np.float32(10.0))
    far.view(np.uint32)[:] = 0x80000001
    got = boxes_ref.boxes([np.full((1, 16, 16), 9, np.uint8)], [CUBE], [far[None]])
    assert got[0, 0, 0, 7] == np.int32(-0x7FFFFFFF) and got.view(np.uint32)[0, 0, 0, 7] == 0x80000001


def test_the_model_random_planes_both_ways():
    rng = np.random.default_rng(9)
    segs = [rng.choice(np.array([0, 1, 2, 8, 9, 10, 0x81, 0x89], np.uint8), (5, 16, 20), p=[0.5, 0.2, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05]) for _ in range(2)]
    segs[1][3] = 0                       # an env with nothing but sky in one slot
    depths = [rng.uniform(0.1, 5.0, (5, 16, 20)).astype(np.float32) for _ in range(2)]
    masks = [ARM, CUBE, CUBE2, MARKER, CUBE | CUBE2, FLOOR]
    got = boxes_ref.boxes(segs, masks, depths)
    assert got.shape == (5, 2, 6, 8) and (got[3, 1] == 0).all() and (got[..., 4] > 0).sum() > 40
    for e in range(5):
        for s in range(2):
            for o, mask in enumerate(masks):
                np.testing.assert_array_equal(got[e, s, o].view(np.uint32).astype(np.int64), boxes_ref.record(segs[s][e], mask, depths[s][e]))
    np.testing.assert_array_equal(boxes_ref.boxes(segs, masks)[..., :7], got[..., :7])
    assert (boxes_ref.boxes(segs, masks)[..., 7] == 0).all()
