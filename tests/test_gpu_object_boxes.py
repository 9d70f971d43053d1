"""The object boxes on the GPU (VecSim(..., object_boxes=dict(objects=, cameras=, depth=)); lcr_enable_object_boxes): the library's device buffer against the numpy model of
tests/boxes_ref.py, which is fed the library's own segmentation and depth planes read back.

What is exact: everything.  A record is minima, maxima, counts and sums of integers (include/lcr.h: "Object boxes"), so every int32 is compared exactly, after enabling and
after every step of seeded random actions, and the guard regions are read back at the end of each rollout.

Each rollout ASSERTS the regime it is there for, so a case that never reaches it fails:
  stack   n = 70 (a ragged second wave of envs), 36 x 52 (117 chunks: a ragged second wave of chunks; W = 52 is no multiple of 16, chunks cross row ends), front + top +
          wrist, depth, 55 steps (an auto-reset of every env).  Objects floor, arm, cube, cube2, marker, link_6 and the union (cube, cube2): the marker records are empty
          throughout (StackTwoCubes has no marker); arm and both cubes are non-empty in front and top at reset (the arm and, through front, both cubes in EVERY env;
          through top both cubes in most envs -- a cube that the arm hides from the camera above it has an empty record, which is the occlusion the records are there to
          report); the union's count is the sum of the cubes'; the floor touches a frame border; over the rollout the wrist camera
          gives both an empty and a non-empty cube record.
  push    n = 5 at 16 x 20 (H x W: 20 chunks, a frame smaller than a workgroup, chunks across row ends) and at 20 x 16, front + top, 6 steps: the marker record is
          non-empty, so bit 7 of the byte is exercised.
  reach   n = 3 at the default 240 x 320, 1 step; n = 3 at 512 x 512 with the floor object (the large sums), 1 step; n = 64 at 84 x 84 (441 chunks), 3 steps.
The regimes were checked first on the CPU at reset states of the oracle (seeds 1000 ..; tests/planes_ref.py and tests/wrist_ref.py, the model on their planes): stack
36 x 52, 70 states -- the arm through front and top and both cubes through front visible in all 70; through top one of the cubes hidden under the arm in 14 (never both):
56 of 70 with everything visible; the floor on a border in all; the wrist camera at its reset pose without the cube in all of 16, so a non-empty wrist record has to come
from the rollout.  push 16 x 20 and 20 x 16 -- the marker visible through front and top in 16 of 16.
On an MI355X the rollouts gave (every record equal to the model's in all of them): stack 3 920 env-checks, 76 auto-resets, 57 875 of 82 320 records non-empty, no marker
record; at reset the arm through front and top and both cubes through front in 70 of 70 envs, both cubes through top in 56, one env with both hidden under the arm; the
union equal to the sum in all 11 760 (env, slot) checks; the floor on a border in 10 944 records; the wrist camera without the cube in 3 462 records and with it in 458.
push 16 x 20 69 and 20 x 16 63 non-empty marker records of 70.  default 24 of 48 records non-empty, the largest sum_x 1 218 710.  large 36 of 36 non-empty, 12 records
as wide as the frame, the largest sum_x 58 461 287.  many 998 of 2 048 non-empty.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import boxes_ref

pytestmark = pytest.mark.gpu

ALL = ("front", "top", "wrist")
STACK_OBJECTS = ("floor", "arm", "cube", "cube2", "marker", "link_6", ("cube", "cube2"))
# name, task, n, size (H, W), cameras, objects (None: the defaults), depth, steps
ROLLOUTS = [
    ("stack", "stack", 70, (36, 52), ALL, STACK_OBJECTS, True, 55),
    ("push", "push", 5, (16, 20), ("front", "top"), None, False, 6),
    ("push", "push", 5, (20, 16), ("front", "top"), None, True, 6),
    ("default", "reach", 3, None, ("front", "top"), None, True, 1),
    ("large", "reach", 3, (512, 512), ("front", "top"), ("floor", "arm", "cube"), True, 1),
    ("many", "reach", 64, (84, 84), ("front", "top"), None, False, 3),
]
ROLLOUT_IDS = [f"{r[0]}-{r[1]}-n{r[2]}-" + ("default" if r[3] is None else f"{r[3][0]}x{r[3][1]}") for r in ROLLOUTS]


def _boxes(cams=None, objects=None, depth=False):
    d = dict(depth=depth)
    if cams is not None:
        d["cameras"] = cams
    if objects is not None:
        d["objects"] = objects
    return d


def _kw(size, wrist, depth=True, **more):
    kw = dict(observation_mode="both", image_planes=("depth", "segmentation") if depth else ("segmentation",), wrist_camera=True if wrist else None, **more)
    if size is not None:
        kw["image_size"] = size
    return kw


def _check(sim, when, boxes=None, spec=None):
    """the invariant: the records are the header's function of the env's current planes, exactly (`boxes`: the records read some other way) -> the model's array"""
    sp = spec or sim.object_boxes_spec
    cams = sp["cameras"]
    segs = [getattr(sim, "seg_" + c).numpy() for c in cams]
    depths = [getattr(sim, "depth_" + c).numpy() for c in cams] if sp["depth"] else None
    want = boxes_ref.boxes(segs, sp["masks"], depths)
    got = sim.object_boxes.numpy() if boxes is None else boxes
    assert got.shape == want.shape == (sim.n, len(cams), len(sp["masks"]), 8) and got.dtype == np.int32
    bad = np.argwhere(got != want)
    assert bad.size == 0, (when, len(bad), bad[:6].tolist(), [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:6]])
    return want


def _check_guards(sim, when, arr=None):
    from gym_lowcostrobot_amd import _capi
    from tests.test_gpu_wrist import _guards

    for side, g in zip(("before", "behind"), _guards(sim, sim.object_boxes if arr is None else arr)):
        assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (when, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())


@functools.lru_cache(maxsize=None)
def _rollout(case):
    """runs one rollout, checking the invariant after enabling and after every step -> the regime counters"""
    from gym_lowcostrobot_amd import VecSim, _capi

    name, task, n, size, cams, objects, depth, steps = case
    sim = VecSim(task, n, base_seed=17, object_boxes=_boxes(cams, objects, depth), **_kw(size, "wrist" in cams, depth))
    given = _capi.BOXES_DEFAULT_OBJECTS if objects is None else objects
    assert sim.object_boxes_spec == {"cameras": cams, "objects": given, "masks": tuple(boxes_ref.mask_of(o) for o in given), "depth": depth}
    H, W = sim.seg_front.shape[1:]
    idx = {o: i for i, o in enumerate(given)}
    F = {f: i for i, f in enumerate(_capi.BOXES_FIELDS)}
    act = sim.alloc_actions()
    st = {"resets": 0, "checks": 0, "records": 0, "nonempty": 0, "max_sum_x": 0, "marker_nonempty": 0, "marker_on_cube": 0, "reset_arm_everywhere": None, "reset_cubes_front": None, "reset_cubes_top": None,
          "reset_cubes_top_both_hidden": None,
          "union_is_sum": 0, "floor_on_border": 0, "wrist_cube_empty": 0, "wrist_cube_nonempty": 0, "nearest_nonzero": 0, "full_width": 0}
    for t in range(-1, steps):
        if t >= 0:
            sim.fill_random_actions(act, 23, t); sim.step_device(act.ptr)
            st["resets"] += int(sim.outputs()["did_reset"].sum())
        m = _check(sim, f"step {t}")
        st["checks"] += n
        st["records"] += m[..., 0].size
        st["nonempty"] += int((m[..., F["count"]] > 0).sum())
        st["max_sum_x"] = max(st["max_sum_x"], int(m[..., F["sum_x"]].max()))
        st["nearest_nonzero"] += int((m[..., F["nearest"]] != 0).sum())
        st["full_width"] += int(((m[..., F["x0"]] == 0) & (m[..., F["x1"]] == W)).sum())
        if depth:   # nearest is the smallest depth of the matching pixels, a positive float below depth_far, wherever a record is not empty
            near = np.ascontiguousarray(m[..., F["nearest"]]).view(np.float32)
            full = m[..., F["count"]] > 0
            assert (near[full] > 0).all() and (near[full] <= 10.0).all() and (near[~full] == 0).all()
        else:
            assert (m[..., F["nearest"]] == 0).all()
        assert (m[m[..., F["count"]] == 0] == 0).all()
        if "marker" in idx:
            st["marker_nonempty"] += int((m[:, :, idx["marker"], F["count"]] > 0).sum())
            segs = np.stack([getattr(sim, "seg_" + c).numpy() for c in cams])
            st["marker_on_cube"] += int(((segs & 0x80) != 0)[(segs & 0x7F) == 9].sum())   # pixels that count for the cube and for the marker
        if name == "stack":
            if t == -1:
                seen = m[:, :2][:, :, [idx["arm"], idx["cube"], idx["cube2"]], F["count"]] > 0        # [env][front, top][arm, cube, cube2]
                st["reset_arm_everywhere"] = bool(seen[:, :, 0].all())
                st["reset_cubes_front"] = int(seen[:, 0, 1:].all(axis=1).sum())
                st["reset_cubes_top"] = int(seen[:, 1, 1:].all(axis=1).sum())
                st["reset_cubes_top_both_hidden"] = int((~seen[:, 1, 1:]).all(axis=1).sum())
            u, c1, c2 = (m[:, :, idx[o]] for o in (("cube", "cube2"), "cube", "cube2"))
            st["union_is_sum"] += int(((u[..., 4:7] == c1[..., 4:7] + c2[..., 4:7]).all(axis=-1)).sum())
            fl = m[:, :, idx["floor"]]
            st["floor_on_border"] += int(((fl[..., F["count"]] > 0) & ((fl[..., F["x0"]] == 0) | (fl[..., F["x1"]] == W))).sum())
            wc = m[:, cams.index("wrist"), idx["cube"], F["count"]]
            st["wrist_cube_empty"] += int((wc == 0).sum()); st["wrist_cube_nonempty"] += int((wc > 0).sum())
    _check_guards(sim, "after the rollout")
    np.testing.assert_array_equal(sim.observations()["object_boxes"], sim.object_boxes.numpy())
    sim.free(act); sim.close()
    print(f"object boxes rollout {ROLLOUT_IDS[ROLLOUTS.index(case)]}: {st}")
    return st


@pytest.mark.parametrize("case", ROLLOUTS, ids=ROLLOUT_IDS)
def test_rollout_against_the_model(hip_lib, case):
    """Random actions; after enabling and after every step every record is the model's, exactly, and the case is in the regime it is there for"""
    name, task, n, size, cams, objects, depth, steps = case
    st = _rollout(case)
    assert st["checks"] == n * (steps + 1) and st["nonempty"] > 0, st
    if steps >= 55:
        assert st["resets"] >= n, st                       # 55 steps cross an auto-reset of every env
    if name == "stack":
        assert st["marker_nonempty"] == 0, st              # StackTwoCubes has no marker: its records are empty throughout
        # (the oracle's reset states on the CPU: 70, 70 and 56 of 70 -- a cube under the arm is hidden from the camera above; both can be, which is counted, not refused)
        assert st["reset_arm_everywhere"] is True and st["reset_cubes_front"] == n and 2 * st["reset_cubes_top"] > n, st
        assert st["union_is_sum"] == st["checks"] * len(cams), st
        assert st["floor_on_border"] > 0, st
        assert st["wrist_cube_empty"] > 0 and st["wrist_cube_nonempty"] > 0, st
        assert st["nearest_nonzero"] > 0, st
    if name == "push":
        assert 20 in size and st["marker_nonempty"] > 0, st   # bit 7 of the byte
    if name == "default":
        assert size is None, st
    if name == "large":
        # the floor fills rows of 512 pixels: sums far beyond 2^16 a record, below 2^31
        assert st["full_width"] > 0 and 2 ** 24 < st["max_sum_x"] < 2 ** 31, st
    if name == "many":
        assert n == 64 and size == (84, 84), st


def test_the_entry_points(hip_lib):
    """The invariant after reset(), a masked reset, set_state followed by the all-zero-mask reset, set_look, and a step whose frames ran on the second stream, read through
    observations()"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 6, (36, 52)
    variants = [{}, {"cam_dpos": [[0.03, 0.0, 0.02], [0.0, 0.04, 0.05]], "fovy_deg": [50.0, 40.0]}]
    sim = VecSim("push", n, object_boxes=_boxes(None, ("arm", "cube", "marker", "floor"), True), **_kw(size, True, base_seed=2, look_variants=variants))
    assert sim.object_boxes_spec["cameras"] == ALL      # the default: every camera the handle has
    rng = np.random.default_rng(4)
    _check(sim, "enabled")
    for t in range(2):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))   # (frames and records on the second stream: LCR_RENDER_OVERLAP is not set)
        obs = sim.observations()
        m = _check(sim, f"step {t} through observations()", boxes=obs["object_boxes"])
        assert obs["object_boxes"].shape == (n, 3, 4, 8) and obs["object_boxes"].dtype == np.int32 and (m[:, :2, 0, 4] > 0).all()

    before = sim.object_boxes.numpy()
    sim.reset()
    _check(sim, "reset()")
    assert (sim.object_boxes.numpy() != before).any()

    before = sim.object_boxes.numpy()
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    sim.reset(mask=mask, seeds=np.arange(100, 100 + n, dtype=np.uint64))
    _check(sim, "reset(mask)")
    after = sim.object_boxes.numpy()
    np.testing.assert_array_equal(after[mask == 0], before[mask == 0])
    assert (after[mask == 1] != before[mask == 1]).any()

    qpos = sim.get_state()["qpos"]
    qpos[:5] += rng.uniform(-0.3, 0.3, (5, n))
    sim.set_state(qpos=qpos)
    sim.reset(mask=np.zeros(n, np.uint8))
    _check(sim, "reset(zeros) after set_state")
    assert (sim.object_boxes.numpy() != after).any()

    before = sim.object_boxes.numpy()
    variant, rgb9 = (np.arange(n) % 2).astype(np.int32), rng.uniform(0, 1, (9, n)).astype(np.float32)
    sim.set_look(variant=variant, rgb=rgb9)
    _check(sim, "set_look")
    assert (sim.object_boxes.numpy()[variant == 1] != before[variant == 1]).any()       # the moved cameras see the objects elsewhere
    np.testing.assert_array_equal(sim.object_boxes.numpy()[variant == 0], before[variant == 0])
    _check_guards(sim, "after the entry points")
    sim.close()


def _raw(sim, L):
    """records and spec from lcr_get_object_boxes: boxes enabled through the C ABI on a live VecSim"""
    from gym_lowcostrobot_amd import _capi
    from gym_lowcostrobot_amd.vecsim import DeviceArray

    bv = _capi.LcrObjectBoxesView()
    assert L.lcr_get_object_boxes(sim.handle, ctypes.byref(bv)) == 0 and bv.enabled == 1
    O, S = int(bv.spec.n_objects), int(bv.slots)
    assert bv.bytes_per_env == S * O * 8 * 4 and (bv.image_height, bv.image_width) == tuple(sim.seg_front.shape[1:])
    assert all(bv.spec.objects[i] == 0 for i in range(O, _capi.BOXES_MAX_OBJECTS))
    return DeviceArray(sim, bv.boxes, (sim.n, S, O, 8), np.int32), bv.spec.as_dict()


def test_enabled_through_the_c_abi_on_a_live_vecsim(hip_lib):
    """Boxes enabled with lcr_enable_object_boxes on a handle that has already stepped are the records of its current planes, the raw view gives the bytes of a handle made
    with the keyword, the same spec again does nothing and another is refused naming both"""
    from gym_lowcostrobot_amd import VecSim, _capi

    L = hip_lib
    n, size = 6, (36, 52)
    kw = _kw(size, True, base_seed=2)
    spec = _boxes(None, ("arm", "cube", "marker", ("cube", "marker")), True)
    sim = VecSim("push", n, object_boxes=spec, **kw)
    late = VecSim("push", n, **kw)
    assert late.object_boxes is None and late.object_boxes_spec is None and "object_boxes" not in late.observations()
    rng = np.random.default_rng(4)
    for t in range(2):
        a = rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32)
        sim.step(a); late.step(a)
    bv = _capi.LcrObjectBoxesView()
    ctypes.memset(ctypes.byref(bv), 0x5A, ctypes.sizeof(bv))
    assert L.lcr_get_object_boxes(late.handle, ctypes.byref(bv)) == 0 and bytes(bv) == bytes(ctypes.sizeof(bv))   # enabled = 0, and the pointer NULL
    csp = _capi.ObjectBoxesSpec.from_any(spec, wrist=True)
    csp.objects[10] = 0xFFFFFFFF   # (beyond n_objects: not looked at, reported as 0)
    assert L.lcr_enable_object_boxes(late.handle, ctypes.byref(csp)) == 0, L.lcr_last_error()
    raw, rspec = _raw(late, L)
    assert rspec["masks"] == sim.object_boxes_spec["masks"] and rspec["cameras"] == ALL and rspec["depth"] is True
    for t in range(2):
        if t:
            a = rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32)
            sim.step(a); late.step(a)
            raw, _ = _raw(late, L)   # (joins)
        _check(late, f"enabled late, {t}", boxes=raw.numpy(), spec=rspec)
        np.testing.assert_array_equal(raw.numpy(), sim.object_boxes.numpy(), err_msg=f"the handle enabled late, {t}")
    first = raw.ptr
    assert L.lcr_enable_object_boxes(late.handle, ctypes.byref(csp)) == 0 and _raw(late, L)[0].ptr == first          # the same spec again: nothing happens
    other = _capi.ObjectBoxesSpec.from_any(_boxes(None, ("arm", "cube", "marker"), True), wrist=True)
    assert L.lcr_enable_object_boxes(late.handle, ctypes.byref(other)) == _capi.LCR_ERR_INVALID
    msg = L.lcr_last_error()
    assert b"fixed for the life" in msg and b"4 objects" in msg.split(b"asked for")[0] and b"3 objects" in msg.split(b"asked for")[1], msg
    _check_guards(late, "enabled late", raw)
    late.close(); sim.close()

    # what lcr_enable_object_boxes refuses of a handle, each by name; no plane is switched on
    sp = _capi.ObjectBoxesSpec.from_any(_boxes(("front", "top"), None, False))
    spd = _capi.ObjectBoxesSpec.from_any(_boxes(("front", "top"), None, True))
    state = VecSim("push", n, observation_mode="state")
    assert L.lcr_enable_object_boxes(state.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID and b"no image observations" in L.lcr_last_error()
    state.close()
    for planes, s_, word in (((), sp, b"the segmentation plane is missing"), (("depth",), sp, b"the segmentation plane is missing"), (("segmentation",), spd, b"the depth plane is missing")):
        h = VecSim("push", n, observation_mode="both", image_size=(16, 16), image_planes=planes)
        assert L.lcr_enable_object_boxes(h.handle, ctypes.byref(s_)) == _capi.LCR_ERR_INVALID and word in L.lcr_last_error(), L.lcr_last_error()
        assert (h.seg_front is None) == ("segmentation" not in planes) and (h.depth_front is None) == ("depth" not in planes)   # no plane was switched on
        if planes == ("segmentation",):   # the segmentation plane alone is enough without depth
            assert L.lcr_enable_object_boxes(h.handle, ctypes.byref(sp)) == 0, L.lcr_last_error()
            raw, rspec = _raw(h, L)
            want = boxes_ref.boxes([h.seg_front.numpy(), h.seg_top.numpy()], rspec["masks"])
            np.testing.assert_array_equal(raw.numpy(), want)
            assert (want[..., 7] == 0).all() and (want[:, :, 0, 4] > 0).all()
        h.close()
    h = VecSim("push", n, **_kw((16, 16), False))
    wr = _capi.ObjectBoxesSpec.from_any(_boxes(("front", "wrist"), None, False))
    assert L.lcr_enable_object_boxes(h.handle, ctypes.byref(wr)) == _capi.LCR_ERR_INVALID and b"wrist camera" in L.lcr_last_error()
    h.close()


BESIDE = ("image_front", "image_top", "image_wrist", "depth_front", "depth_top", "depth_wrist", "seg_front", "seg_top", "seg_wrist", "obs_stack", "point_cloud",
          "point_cloud_count", "heightmap", "heightmap_count", "reward", "terminated", "truncated", "is_success", "did_reset", "terminal_obs")
LOOK_BOX = ((-0.12, -0.05, 0.0), (0.12, 0.3, 0.2))


def test_off_means_off(hip_lib):
    """Two handles with the same seeds, one with boxes and one without: the frames, planes, stack, cloud, map and outputs of the handle without them are those of the handle
    with them over a short rollout with auto-resets -- the boxes change nothing beside themselves -- and the handle without has no key and no attribute"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=21, max_episode_steps=4, obs_stack=2, point_cloud=dict(points=64, ids=("arm", "cube", "cube2", "floor")),
             heightmap=dict(box=LOOK_BOX, dims=(8, 10), ids=("arm", "cube", "cube2", "floor")))
    on = VecSim("stack", n, object_boxes=_boxes(None, STACK_OBJECTS, True), **kw)
    off = VecSim("stack", n, **kw)
    assert off.object_boxes is None and off.object_boxes_spec is None and "object_boxes" not in off.observations() and "object_boxes" in on.observations()
    acts = [(s_, s_.alloc_actions()) for s_ in (on, off)]
    for t in range(-1, 6):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 11, t); s_.step_device(a.ptr)
        for name in BESIDE:
            np.testing.assert_array_equal(getattr(on, name).numpy().view(np.uint8), getattr(off, name).numpy().view(np.uint8), err_msg=f"{name} beside the boxes, step {t}")
        st_on, st_off = on.get_state(), off.get_state()
        for k in ("qpos", "qvel"):
            np.testing.assert_array_equal(st_on[k], st_off[k], err_msg=f"{k} beside the boxes, step {t}")
    _check(on, "beside the stack, the cloud and the map")
    assert (on.heightmap_count.numpy() > 0).all() and (on.point_cloud_count.numpy() > 0).all()
    _check_guards(on, "after the rollout")
    for s_, a in acts:
        s_.free(a); s_.close()


def test_two_handles_with_the_same_seeds_give_the_same_bytes(hip_lib):
    from gym_lowcostrobot_amd import VecSim

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=3, max_episode_steps=4, object_boxes=_boxes(None, STACK_OBJECTS, True))
    sims = [VecSim("stack", n, **kw) for _ in range(2)]
    acts = [(s_, s_.alloc_actions()) for s_ in sims]
    for t in range(10):
        for s_, a in acts:
            s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
    np.testing.assert_array_equal(sims[0].object_boxes.numpy(), sims[1].object_boxes.numpy())
    m = _check(sims[0], "after ten steps")
    assert (m[:, :2, 1, 4] > 0).all()   # the arm through front and top
    for s_, a in acts:
        _check_guards(s_, "after the rollout")
        s_.free(a); s_.close()


def test_sharded_boxes_are_the_unsharded_boxes(hip_lib):
    """Two shards of 64 envs keep the records of the unsharded 128-env handle, byte for byte; every shard has the spec"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = _kw((16, 16), True, base_seed=9, max_episode_steps=3, object_boxes=_boxes(None, None, True))
    one = VecSim("push", 128, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], **kw)
    assert all(s_.object_boxes.shape == (64, 3, 4, 8) and s_.object_boxes_spec == one.object_boxes_spec for s_ in sh.shards)
    act = one.alloc_actions()
    for t in range(4):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
    got = np.concatenate([s_.object_boxes.numpy() for s_ in sh.shards], axis=0)
    np.testing.assert_array_equal(got, one.object_boxes.numpy())
    m = _check(one, "after the steps")
    assert (m[..., 4] > 0).any()
    one.free(act); one.close(); sh.close()


def test_the_vector_adapters_refuse_the_boxes(hip_lib):
    from gym_lowcostrobot_amd.vecenv import LowCostRobotVecEnv, LowCostRobotVectorEnv

    for Adapter in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        with pytest.raises(ValueError, match="cannot make the boxes of the episode that ended"):
            Adapter("reach", 4, object_boxes=True, **_kw((16, 16), False))
