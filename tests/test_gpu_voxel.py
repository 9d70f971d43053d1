"""The voxel grid on the GPU (VecSim(..., voxel_grid=dict(box=(lo, hi), dims=(Dx, Dy, Dz), ...)); lcr_enable_voxel_grid): the library's device buffers against the numpy model
of tests/voxel_ref.py, which is fed the library's own planes, frames, reported camera poses and reported inv_cell.

What is exact: everything.  The point and the voxel of a candidate are pinned to the bit (include/lcr.h: "The voxel grid"), and the model evaluates the same chain with an
exact fused multiply-add and float32 numpy arithmetic, so which voxel a pixel falls in is a reproducible decision: the grid's bytes (or float32 bits), `source`, `count` and
`occupied` are compared exactly, after enabling and after every step of random actions, and the guard regions are read back at the end of each rollout.

Each rollout ASSERTS the regime it is there for, so a case that never reaches it fails:
  FLOOR_BOX  (-0.125, -0.0625, 0.0) .. (0.125, 0.25, 0.25), dims 8 x 10 x 8: every inv_k is 32 exactly and lo_z is 0.0 exactly, a face on the floor plane.  stack 36 x 52, all
             three cameras, + floor, n = 70 (a ragged second wave of envs), 55 steps (an auto-reset of every env): floor pixels of the top camera (z = 0.0 exactly) fall inside
             and outside, floor pixels of the front camera with z < 0 are all outside, some voxel is hit from two cameras
  TOP_BOX    (-0.5, -0.5, -0.125) .. (0.5, 0.5, 0.0), dims 8 x 8 x 4: the half-open top.  Floor points through top have z = 0.0, so v_z = 4.0 exactly: all outside; floor points
             through front are inside only with z < 0, all in layer 3
  ABOVE_BOX  z in 1.0 .. 2.0, dims 4 x 3 x 5: above everything.  push 64 x 64: count = 0 everywhere although candidates by id exist; the grid is zero, source - 1
  CUBE_BOX   (-0.2, 0.0, -0.01) .. (0.2, 0.35, 0.06), dims 12 x 7 x 5 (V = 420, no multiple of 64): the cube's spawn region and the arm's foot in it.  reach 16 x 16,
             float32, occupancy only: 0 < occupied < V
  BIG_BOX    (-0.25, -0.125, 0.0) .. (0.25, 0.375, 0.5), dims 32 x 32 x 32, the largest V (the 128 KiB build, or z-slabs), and 32 x 32 x 16, the largest V of the 64 KiB
             build.  reach 128 x 128, every camera, + floor, rgb: some voxel holds more than one candidate
On an MI355X the rollouts gave: FLOOR_BOX 3 920 env-checks, 76 auto-resets, floor pixels of the top camera 1 208 958 inside and 5 519 610 outside, 2 543 566 floor pixels of
the front camera with z < 0 and none of them inside, 303 304 voxels seen through front and top, 89 .. 147 occupied voxels an env; TOP_BOX top floor 0 inside of 30 580, front
floor 4 310 inside, all in layer 3; ABOVE_BOX 448 of 448 grids zero beside 1 015 098 candidates by id; CUBE_BOX 6 .. 24 occupied voxels of 420; BIG_BOX 173 759 candidates in
1 119 .. 1 156 (32^3) and 1 083 .. 1 107 (32 x 32 x 16) occupied voxels an env.
"""
import ctypes
import functools
import types

import numpy as np
import pytest

from tests import cloud_ref, voxel_ref

pytestmark = pytest.mark.gpu

ALL = ("front", "top", "wrist")
WITH_FLOOR = ("arm", "cube", "cube2", "floor")
FLOOR_BOX = ((-0.125, -0.0625, 0.0), (0.125, 0.25, 0.25))
TOP_BOX = ((-0.5, -0.5, -0.125), (0.5, 0.5, 0.0))
ABOVE_BOX = ((-0.5, -0.5, 1.0), (0.5, 0.5, 2.0))
CUBE_BOX = ((-0.2, 0.0, -0.01), (0.2, 0.35, 0.06))
BIG_BOX = ((-0.25, -0.125, 0.0), (0.25, 0.375, 0.5))
LOOK_BOX = ((-0.12, -0.05, 0.0), (0.12, 0.3, 0.2))
LOW_BOX = ((-0.25, -0.125, 0.0), (0.25, 0.375, 0.125))   # the arm (0.185 m high at reset) passes through its top: every z-layer holds voxels
# name, task, n, size, cameras, ids, rgb, source, dtype, box, dims, steps
ROLLOUTS = [
    ("floor", "stack", 70, (36, 52), ALL, WITH_FLOOR, True, True, "uint8", FLOOR_BOX, (8, 10, 8), 55),
    ("top", "stack", 6, (36, 52), ("front", "top"), WITH_FLOOR, False, True, "uint8", TOP_BOX, (8, 8, 4), 2),
    ("above", "push", 64, (64, 64), ("top", "wrist"), None, True, True, "uint8", ABOVE_BOX, (4, 3, 5), 6),
    ("cube", "reach", 5, (16, 16), ("front", "top"), None, False, False, "float32", CUBE_BOX, (12, 7, 5), 55),
    ("big", "reach", 3, (128, 128), ALL, WITH_FLOOR, True, True, "uint8", BIG_BOX, (32, 32, 32), 1),
    ("big64k", "reach", 3, (128, 128), ALL, WITH_FLOOR, True, False, "float32", BIG_BOX, (32, 32, 16), 1),
]
ROLLOUT_IDS = [f"{r[0]}-{r[1]}-n{r[2]}-{r[10][0]}x{r[10][1]}x{r[10][2]}" for r in ROLLOUTS]


def _grid(box, dims, cams=None, ids=None, rgb=False, source=False, dtype="uint8"):
    d = dict(box=box, dims=dims, features=("occupancy", "rgb") if rgb else ("occupancy",), source=source, dtype=dtype)
    if cams is not None:
        d["cameras"] = cams
    if ids is not None:
        d["ids"] = ids
    return d


def _kw(size, wrist, **more):
    return dict(observation_mode="both", image_size=size, image_planes=("depth", "segmentation"), wrist_camera=True if wrist else None, **more)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _view_of(sim):
    """the grid's buffers and spec as VecSim exposes them"""
    return types.SimpleNamespace(voxels=sim.voxel_grid, source=sim.voxel_grid_source, count=sim.voxel_grid_count, occupied=sim.voxel_grid_occupied, pose=sim.voxel_grid_pose,
                                 spec=sim.voxel_grid_spec)


def _raw_view(sim, L):
    """the same from lcr_get_voxel_grid: a grid enabled through the C ABI on a live VecSim"""
    from gym_lowcostrobot_amd import _capi
    from gym_lowcostrobot_amd.vecsim import DeviceArray

    vv = _capi.LcrVoxelGridView()
    assert L.lcr_get_voxel_grid(sim.handle, ctypes.byref(vv)) == 0 and vv.enabled == 1
    spec = dict(vv.spec.as_dict(), inv_cell=tuple(float(x) for x in vv.inv_cell))
    Dx, Dy, Dz = spec["dims"]
    N = sim.n
    return types.SimpleNamespace(voxels=DeviceArray(sim, vv.voxels, (N, int(vv.channels), Dz, Dy, Dx), np.dtype(spec["dtype"])),
                                 source=DeviceArray(sim, vv.source, (N, Dz, Dy, Dx), np.int32) if vv.source else None, count=DeviceArray(sim, vv.count, (N,), np.int32),
                                 occupied=DeviceArray(sim, vv.occupied, (N,), np.int32), pose=DeviceArray(sim, vv.camera_pose, (int(vv.slots), 13, N), np.float32), spec=spec)


def _check(sim, when, view=None):
    """the invariant: voxels, source, count and occupied are the header's function of the env's current planes, frames, reported poses and reported inv_cell, exactly
    -> the model's dict (voxel_ref.grid)"""
    g = view or _view_of(sim)
    sp = g.spec
    cams = sp["cameras"]
    depth = [getattr(sim, "depth_" + c).numpy() for c in cams]
    seg = [getattr(sim, "seg_" + c).numpy() for c in cams]
    rgb = [getattr(sim, "image_" + c).numpy() for c in cams]
    pose = g.pose.numpy()
    Dx, Dy, Dz = sp["dims"]
    colours = "rgb" in sp["features"]
    assert pose.shape == (len(cams), 13, sim.n) and g.voxels.shape == (sim.n, 4 if colours else 1, Dz, Dy, Dx) and g.voxels.dtype == np.dtype(sp["dtype"])
    want = voxel_ref.grid(depth, seg, rgb, pose, dict(lo=sp["lo"], dims=sp["dims"], ids=cloud_ref.ids_mask(sp["ids"]), rgb=colours, dtype=sp["dtype"]), sp["inv_cell"])
    np.testing.assert_array_equal(g.count.numpy(), want["count"], err_msg=f"count, {when}")
    np.testing.assert_array_equal(g.occupied.numpy(), want["occupied"], err_msg=f"occupied, {when}")
    if g.source is not None:
        bad = np.argwhere(g.source.numpy() != want["source"])
        assert bad.size == 0, (when, "source", len(bad), bad[:6].tolist())
    else:
        assert not sp["source"]
    bad = np.argwhere(_bits(g.voxels.numpy()) != _bits(want["voxels"]))
    assert bad.size == 0, (when, "voxels", len(bad), bad[:6].tolist())
    return want


def _check_guards(sim, when, arr=None):
    from gym_lowcostrobot_amd import _capi
    from tests.test_gpu_wrist import _guards

    for side, g in zip(("before", "behind"), _guards(sim, sim.voxel_grid if arr is None else arr)):
        assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (when, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())


def _expected_spec(box, dims, cams, ids, rgb, source, dtype):
    f = np.float32
    inv = tuple(float(f(float(d) / (float(f(h)) - float(f(l))))) for l, h, d in zip(box[0], box[1], dims))
    return {"lo": tuple(float(f(v)) for v in box[0]), "hi": tuple(float(f(v)) for v in box[1]), "dims": tuple(dims), "cameras": cams,
            "ids": tuple(i for i in range(11) if cloud_ref.ids_mask(ids) >> i & 1), "features": ("occupancy", "rgb") if rgb else ("occupancy",), "dtype": dtype, "source": source,
            "inv_cell": inv}


@functools.lru_cache(maxsize=None)
def _rollout(case):
    """runs one rollout, checking the invariant after enabling and after every step -> the regime counters"""
    from gym_lowcostrobot_amd import VecSim

    name, task, n, size, cams, ids, rgb, source, dtype, box, dims, steps = case
    wrist = "wrist" in cams
    sim = VecSim(task, n, base_seed=17, voxel_grid=_grid(box, dims, cams, ids, rgb, source, dtype), **_kw(size, wrist))
    assert sim.voxel_grid_spec == _expected_spec(box, dims, cams, ids, rgb, source, dtype)
    assert (sim.voxel_grid_source is not None) == source
    H, W = size
    V = dims[0] * dims[1] * dims[2]
    act = sim.alloc_actions()
    st = {"resets": 0, "byid": 0, "count": 0, "occ_min": V, "occ_max": 0, "multi": 0, "shared": 0, "top_floor_in": 0, "top_floor_out": 0, "front_floor_in": 0, "front_floor_out": 0,
          "front_floor_neg": 0, "front_floor_neg_in": 0, "front_floor_layers": set(), "zero_grids": 0, "checks": 0}
    for t in range(-1, steps):
        if t >= 0:
            sim.fill_random_actions(act, 23, t); sim.step_device(act.ptr)
            st["resets"] += int(sim.outputs()["did_reset"].sum())
        m = _check(sim, f"step {t}")
        st["checks"] += n
        st["byid"] += int(m["by_id"].sum()); st["count"] += int(m["count"].sum())
        st["occ_min"] = min(st["occ_min"], int(m["occupied"].min())); st["occ_max"] = max(st["occ_max"], int(m["occupied"].max()))
        st["multi"] += int((m["count"] > m["occupied"]).sum())
        grid_bytes = sim.voxel_grid.numpy()
        st["zero_grids"] += int((~grid_bytes.reshape(n, -1).any(axis=1)).sum())
        if st["count"] == 0 and sim.voxel_grid_source is not None:
            assert (sim.voxel_grid_source.numpy() == -1).all()
        slot_of = {c: i for i, c in enumerate(cams)}
        floor = {c: (getattr(sim, "seg_" + c).numpy().reshape(n, -1) & 0x7F) == 1 for c in ("front", "top") if c in slot_of}
        for c, fl in floor.items():
            sl = slice(slot_of[c] * H * W, (slot_of[c] + 1) * H * W)
            ins = m["inside"][:, sl]
            st[c + "_floor_in"] += int((fl & ins).sum()); st[c + "_floor_out"] += int((fl & m["by_id"][:, sl] & ~ins).sum())
            if c == "front":
                z = m["points"][:, sl, 2]
                st["front_floor_neg"] += int((fl & (z < 0)).sum()); st["front_floor_neg_in"] += int((fl & (z < 0) & ins).sum())
                st["front_floor_layers"] |= set((m["lin"][:, sl][fl & ins] // (dims[0] * dims[1])).tolist())
            if c == "top" and fl.any():
                assert (m["points"][:, sl, 2][fl] == 0.0).all()   # the top camera looks straight down: the float32 z of its floor points is 0.0 exactly
        if "front" in slot_of and "top" in slot_of:   # voxels hit through front AND through top
            for e in range(n):
                a = m["lin"][e, :H * W][m["inside"][e, :H * W]]
                b = m["lin"][e, H * W:2 * H * W][m["inside"][e, H * W:2 * H * W]]
                st["shared"] += len(np.intersect1d(a, b))
    _check_guards(sim, "after the rollout")
    np.testing.assert_array_equal(_bits(sim.observations()["voxel_grid"]), _bits(sim.voxel_grid.numpy()))
    sim.free(act); sim.close()
    print(f"voxel grid rollout {case[:3]}: { {k: (sorted(v) if isinstance(v, set) else v) for k, v in st.items()} }")
    return st


@pytest.mark.parametrize("case", ROLLOUTS, ids=ROLLOUT_IDS)
def test_rollout_against_the_model(hip_lib, case):
    """Random actions; after enabling and after every step the grid, source, count and occupied are the model's, exactly, and the case is in the regime it is there for"""
    name, task, n, size, cams, ids, rgb, source, dtype, box, dims, steps = case
    st = _rollout(case)
    V = dims[0] * dims[1] * dims[2]
    assert st["checks"] == n * (steps + 1)
    if steps >= 55:
        assert st["resets"] >= n, st          # 55 steps cross an auto-reset of every env
    if name == "floor":
        f = np.float32
        assert all(f(float(d) / (float(f(h)) - float(f(l)))) == f(32.0) for l, h, d in zip(box[0], box[1], dims)) and f(box[0][2]) == 0.0
        assert st["top_floor_in"] > 0 and st["top_floor_out"] > 0, st
        assert st["front_floor_neg"] > 0 and st["front_floor_neg_in"] == 0, st
        assert st["shared"] > 0, st
    if name == "top":
        assert st["top_floor_in"] == 0 and st["top_floor_out"] > 0, st                       # v_z = 4.0 exactly: outside
        assert st["front_floor_in"] > 0 and st["front_floor_layers"] == {3}, st
    if name == "above":
        assert st["count"] == 0 and st["byid"] > 0 and st["zero_grids"] == st["checks"] and st["occ_max"] == 0, st
    if name == "cube":
        assert 0 < st["occ_min"] and st["occ_max"] < V and V % 64 != 0, st
    if name in ("big", "big64k"):
        assert st["multi"] > 0 and st["occ_min"] > 0, st
        assert V == (32768 if name == "big" else 16384)


@pytest.mark.parametrize("dims", [(32, 32, 32), (60, 60, 9)], ids=["32x32x32", "60x60x9"])
def test_the_two_ways_to_hold_a_large_grid_give_the_same_bytes(hip_lib, monkeypatch, dims):
    """LCR_VOXEL_LDS=big (the grid whole, in the 128 KiB build) and =slab (two z-slabs at 32 x 32 x 32, three at 60 x 60 x 9) beside the default: identical bytes, and the
    model's"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 3, (64, 64)
    sims = []
    for mode in ("big", "slab", None):
        if mode is None:
            monkeypatch.delenv("LCR_VOXEL_LDS", raising=False)
        else:
            monkeypatch.setenv("LCR_VOXEL_LDS", mode)
        sims.append(VecSim("stack", n, base_seed=4, voxel_grid=_grid(LOW_BOX, dims, None, WITH_FLOOR, True, True), **_kw(size, True)))
    monkeypatch.delenv("LCR_VOXEL_LDS", raising=False)
    rng = np.random.default_rng(2)
    for t in range(-1, 2):
        if t >= 0:
            a = rng.uniform(-1, 1, (n, sims[0].action_dim)).astype(np.float32)
            for s_ in sims:
                s_.step(a)
        m = _check(sims[0], f"big, step {t}")
        assert (m["count"] > m["occupied"]).all() and (m["occupied"] > 0).all()
        layers = np.unique(np.argwhere(sims[0].voxel_grid_source.numpy() >= 0)[:, 1])
        assert layers.min() == 0 and layers.max() >= dims[2] - (dims[2] + 2) // 3, layers   # voxels in the first and in the last slab, of two and of three
        for s_ in sims[1:]:
            for name in ("voxel_grid", "voxel_grid_source", "voxel_grid_count", "voxel_grid_occupied", "voxel_grid_pose"):
                np.testing.assert_array_equal(_bits(getattr(s_, name).numpy()), _bits(getattr(sims[0], name).numpy()), err_msg=f"{name}, step {t}")
    for s_ in sims:
        _check_guards(s_, "after the steps")
        s_.close()


def test_per_env_cameras(hip_lib):
    """With look variants that move and turn the cameras and change the fovy, redrawn per env at every auto-reset, and after set_look, the grid follows each env's own
    cameras, and voxel_grid_pose shows them"""
    from gym_lowcostrobot_amd import VecSim
    from tests import look_ref

    n, size = 12, (96, 96)
    sim = VecSim("push", n, base_seed=5, max_episode_steps=3, look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 9},
                 voxel_grid=_grid(LOOK_BOX, (16, 20, 12), ("front", "top"), WITH_FLOOR, True, True), **_kw(size, False))
    act = sim.alloc_actions()
    seen = set()
    for t in range(-1, 4):
        if t >= 0:
            sim.fill_random_actions(act, 3, t); sim.step_device(act.ptr)
        m = _check(sim, f"step {t}")
        seen |= set(sim.look()["variant"].tolist())
        assert (m["count"] > 0).all() and (m["count"] < m["by_id"].sum(axis=1)).all()
    assert len(seen) > 1   # the envs did change variants
    pose = sim.voxel_grid_pose.numpy()
    variant = sim.look()["variant"]
    assert len({pose[:, :, e].tobytes() for e in range(n)}) == len(set(variant.tolist()))   # one pose per variant in play
    before, pose_before = sim.voxel_grid.numpy(), pose
    variant = ((np.arange(n) + 1) % len(look_ref.GPU_VARIANTS)).astype(np.int32)
    sim.set_look(variant=variant, rgb=np.random.default_rng(1).uniform(0, 1, (9, n)).astype(np.float32))
    _check(sim, "set_look")
    assert (sim.voxel_grid_pose.numpy() != pose_before).any() and (sim.voxel_grid.numpy() != before).any()
    _check_guards(sim, "after set_look")
    sim.free(act); sim.close()


def test_the_entry_points_that_are_not_the_step(hip_lib):
    """After reset(), a masked reset, set_state followed by the all-zero-mask reset, and set_look the grid is the header's function of the current frames; and a grid enabled
    through the C ABI on a handle that has already stepped is the grid of its current frames"""
    from gym_lowcostrobot_amd import VecSim, _capi

    n, size = 6, (96, 96)
    variants = [{}, {"cam_dpos": [[0.03, 0.0, 0.02], [0.0, 0.04, 0.05]], "fovy_deg": [50.0, 40.0]}]
    kw = _kw(size, True, base_seed=2, look_variants=variants)
    spec = _grid(LOOK_BOX, (16, 20, 12), None, ("arm", "cube", "floor"), True, True, "float32")
    sim = VecSim("push", n, voxel_grid=spec, **kw)
    late = VecSim("push", n, **kw)
    rng = np.random.default_rng(4)
    _check(sim, "enabled")
    for t in range(2):
        a = rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32)
        sim.step(a); late.step(a)
    m = _check(sim, "steps")
    assert (m["occupied"] > 0).all()

    # enabling on a handle that has already stepped: the grid of the frames it has now, which are those of `sim`
    L = hip_lib
    vv = _capi.LcrVoxelGridView()
    assert L.lcr_get_voxel_grid(late.handle, ctypes.byref(vv)) == 0 and vv.enabled == 0
    assert L.lcr_enable_voxel_grid(late.handle, ctypes.byref(_capi.VoxelGridSpec.from_any(spec))) == 0, L.lcr_last_error()
    raw = _raw_view(late, L)
    assert raw.spec == sim.voxel_grid_spec
    _check(late, "enabled late", raw)
    for name in ("voxels", "source", "count", "occupied", "pose"):
        np.testing.assert_array_equal(_bits(getattr(raw, name).numpy()), _bits(getattr(_view_of(sim), name).numpy()), err_msg=f"{name} of the handle enabled late")
    a = rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32)
    sim.step(a); late.step(a)
    raw = _raw_view(late, L)   # (joins)
    _check(late, "a step after enabling late", raw)
    _check_guards(late, "enabled late", raw.voxels)
    late.close()

    before = sim.voxel_grid.numpy()
    sim.reset()
    _check(sim, "reset()")
    assert (sim.voxel_grid.numpy() != before).any()

    before = sim.voxel_grid.numpy()
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    sim.reset(mask=mask, seeds=np.arange(100, 100 + n, dtype=np.uint64))
    _check(sim, "reset(mask)")
    after = sim.voxel_grid.numpy()
    np.testing.assert_array_equal(_bits(after[mask == 0]), _bits(before[mask == 0]))
    assert (after[mask == 1] != before[mask == 1]).any()

    qpos = sim.get_state()["qpos"]
    qpos[:5] += rng.uniform(-0.3, 0.3, (5, n))
    sim.set_state(qpos=qpos)
    sim.reset(mask=np.zeros(n, np.uint8))
    _check(sim, "reset(zeros) after set_state")
    assert (sim.voxel_grid.numpy() != after).any()

    before = sim.voxel_grid.numpy()
    variant, rgb9 = (np.arange(n) % 2).astype(np.int32), rng.uniform(0, 1, (9, n)).astype(np.float32)
    sim.set_look(variant=variant, rgb=rgb9)
    _check(sim, "set_look")
    assert (sim.voxel_grid.numpy()[variant == 1] != before[variant == 1]).any()
    _check_guards(sim, "after the entry points")
    sim.close()


def test_grid_on_the_second_stream_is_the_serial_grid(hip_lib, monkeypatch):
    """The same seeded rollout of ten steps with frames and grid on the caller's stream (LCR_RENDER_OVERLAP=0) and on the second stream: identical bytes, across auto-resets
    that redraw the looks"""
    from gym_lowcostrobot_amd import VecSim
    from tests import look_ref

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=3, max_episode_steps=3, look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 7},
             voxel_grid=_grid(FLOOR_BOX, (8, 10, 8), None, WITH_FLOOR, True, True))
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", n, **kw)
    acts = [(s_, s_.alloc_actions()) for s_ in (ref, ovl)]
    for t in range(-1, 10):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
        for name in ("voxel_grid", "voxel_grid_source", "voxel_grid_count", "voxel_grid_occupied", "voxel_grid_pose"):
            np.testing.assert_array_equal(_bits(getattr(ref, name).numpy()), _bits(getattr(ovl, name).numpy()), err_msg=f"{name}, step {t}")
    assert (ovl.voxel_grid_count.numpy() > 0).all()
    _check(ovl, "second stream")
    for s_, a in acts:
        _check_guards(s_, "after the rollout")
        s_.free(a); s_.close()


def test_a_torch_read_on_the_handles_stream_behind_get_obs_sees_the_steps_grid(hip_lib, monkeypatch):
    """The stream-order contract: on a torch stream handed to set_stream, step_device, lcr_get_obs (a joining call), then a clone of sim.voxel_grid.torch() enqueued on that
    stream -- with no host wait in between -- holds the grid of that step: the bytes of a handle that draws on its own stream (LCR_RENDER_OVERLAP=0)"""
    import torch

    from gym_lowcostrobot_amd import VecSim

    n, size, steps = 70, (36, 52), 6
    kw = _kw(size, False, base_seed=8, voxel_grid=_grid(FLOOR_BOX, (8, 10, 8), None, WITH_FLOOR, True, False))
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    want = []
    a = ref.alloc_actions()
    for t in range(steps):
        ref.fill_random_actions(a, 9, t); ref.step_device(a.ptr)
        want.append(ref.voxel_grid.numpy())
    ref.free(a); ref.close()
    assert any((want[t] != want[t - 1]).any() for t in range(1, steps))   # the grid changes from step to step

    sim = VecSim("stack", n, **kw)
    stream = torch.cuda.Stream(device=sim.device)
    sim.set_stream(stream.cuda_stream)
    a = sim.alloc_actions()
    got = []
    with torch.cuda.stream(stream):
        view = sim.voxel_grid.torch()
        assert view.dtype == torch.uint8 and tuple(view.shape) == (n, 4, 8, 10, 8) and view.data_ptr() == sim.voxel_grid.ptr
        for t in range(steps):
            sim.fill_random_actions(a, 9, t); sim.step_device(a.ptr)
            sim.wait_frames()              # lcr_get_obs: the handle's stream now waits for the grid of this step
            got.append(view.clone())
    stream.synchronize()
    for t in range(steps):
        np.testing.assert_array_equal(got[t].cpu().numpy(), want[t], err_msg=f"step {t}")
    del view, got
    sim.free(a); sim.close()


def test_sharded_grid_is_the_unsharded_grid(hip_lib):
    """Two shards of 64 envs (the cut falls on a wave boundary of the step kernels) keep the grid of the unsharded 128-env handle, byte for byte; every shard has the spec"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = _kw((16, 16), True, base_seed=9, max_episode_steps=3, voxel_grid=_grid(LOOK_BOX, (8, 6, 5), None, WITH_FLOOR, True, True))
    one = VecSim("push", 128, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], **kw)
    assert all(s_.voxel_grid.shape == (64, 4, 5, 6, 8) and s_.voxel_grid_spec == one.voxel_grid_spec for s_ in sh.shards)
    act = one.alloc_actions()
    for t in range(5):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        for name, axis in (("voxel_grid", 0), ("voxel_grid_source", 0), ("voxel_grid_count", 0), ("voxel_grid_occupied", 0), ("voxel_grid_pose", 2)):
            got = np.concatenate([getattr(s_, name).numpy() for s_ in sh.shards], axis=axis)
            np.testing.assert_array_equal(_bits(got), _bits(getattr(one, name).numpy()), err_msg=f"{name}, step {t}")
    m = _check(one, "after the steps")
    assert (m["occupied"] > 0).all()
    one.free(act); one.close(); sh.close()


CLOUD = dict(points=128, sampling="fps", pool=256, crop=LOOK_BOX, ids=WITH_FLOOR, colors=True)
BESIDE = ("image_front", "image_top", "image_wrist", "depth_front", "depth_top", "depth_wrist", "seg_front", "seg_top", "seg_wrist", "obs_stack", "point_cloud",
          "point_cloud_count", "point_cloud_source", "point_cloud_pose", "reward", "terminated", "truncated", "is_success", "did_reset", "terminal_obs")


def test_the_grid_beside_a_cloud_and_a_handle_without_a_grid(hip_lib):
    """Three handles with the same seeds: grid and cropped FPS cloud (and a stack), the cloud alone, the grid alone.  The cloud's bytes equal those of the handle without the
    grid, the grid's those of the handle without the cloud; and the handle WITHOUT a grid has the frames, planes, stack, cloud and outputs of the handle with one -- the
    grid changes nothing beside itself.  lcr_get_voxel_grid on it reports enabled = 0 and NULLs"""
    from gym_lowcostrobot_amd import VecSim, _capi

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=21, max_episode_steps=4)
    grid = _grid(FLOOR_BOX, (8, 10, 8), None, WITH_FLOOR, True, True)
    both = VecSim("stack", n, voxel_grid=grid, point_cloud=CLOUD, obs_stack=2, **kw)
    cloud = VecSim("stack", n, point_cloud=CLOUD, obs_stack=2, **kw)
    alone = VecSim("stack", n, voxel_grid=grid, **kw)
    assert cloud.voxel_grid is None and cloud.voxel_grid_spec is None and cloud.voxel_grid_source is None and "voxel_grid" not in cloud.observations()
    vv = _capi.LcrVoxelGridView()
    ctypes.memset(ctypes.byref(vv), 0x5A, ctypes.sizeof(vv))
    assert hip_lib.lcr_get_voxel_grid(cloud.handle, ctypes.byref(vv)) == 0
    assert bytes(vv) == bytes(ctypes.sizeof(vv))   # enabled = 0, and every pointer NULL
    acts = [(s_, s_.alloc_actions()) for s_ in (both, cloud, alone)]
    for t in range(-1, 6):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 11, t); s_.step_device(a.ptr)
        for name in BESIDE:
            np.testing.assert_array_equal(_bits(getattr(both, name).numpy()), _bits(getattr(cloud, name).numpy()), err_msg=f"{name} beside the grid, step {t}")
        for name in ("voxel_grid", "voxel_grid_source", "voxel_grid_count", "voxel_grid_occupied", "voxel_grid_pose"):
            np.testing.assert_array_equal(_bits(getattr(both, name).numpy()), _bits(getattr(alone, name).numpy()), err_msg=f"{name} beside the cloud, step {t}")
    _check(both, "beside the cloud")
    assert (both.point_cloud_count.numpy() > 0).all() and (both.voxel_grid_count.numpy() > 0).all()
    for s_, a in acts:
        if s_.voxel_grid is not None:
            _check_guards(s_, "after the rollout")
        s_.free(a); s_.close()


def test_life_cycle(hip_lib):
    """The same spec twice is a no-op; another spec is refused with both in the message; a missing plane, a missing wrist camera and state-only observations are refused;
    close() frees the allocation"""
    from gym_lowcostrobot_amd import VecSim, _capi

    L = hip_lib
    n, size = 5, (16, 16)
    sp = _capi.VoxelGridSpec.from_any(_grid(CUBE_BOX, (12, 7, 5), source=True))
    other = _capi.VoxelGridSpec.from_any(_grid(CUBE_BOX, (12, 7, 6), source=True))

    state = VecSim("push", n, observation_mode="state")
    assert L.lcr_enable_voxel_grid(state.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID and b"no image observations" in L.lcr_last_error()
    state.close()
    for planes, word in (((), b"none is enabled"), (("depth",), b"the segmentation plane is missing"), (("segmentation",), b"the depth plane is missing")):
        s_ = VecSim("push", n, observation_mode="both", image_size=size, image_planes=planes)
        assert L.lcr_enable_voxel_grid(s_.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID
        assert b"both image planes" in L.lcr_last_error() and word in L.lcr_last_error(), L.lcr_last_error()
        s_.close()

    sim = VecSim("push", n, **_kw(size, False))
    wrist = _capi.VoxelGridSpec.from_any(_grid(CUBE_BOX, (12, 7, 5), ("front", "wrist")))
    assert L.lcr_enable_voxel_grid(sim.handle, ctypes.byref(wrist)) == _capi.LCR_ERR_INVALID and b"wrist camera" in L.lcr_last_error()
    assert L.lcr_enable_voxel_grid(sim.handle, ctypes.byref(sp)) == 0, L.lcr_last_error()
    vv = _capi.LcrVoxelGridView()
    assert L.lcr_get_voxel_grid(sim.handle, ctypes.byref(vv)) == 0 and vv.enabled == 1 and vv.channels == 1 and vv.slots == 2 and vv.bytes_per_env == 420
    assert (vv.image_height, vv.image_width) == size and vv.spec.cameras == 3 and vv.spec.ids == 0x7FC and vv.spec.features == 1 and vv.source and vv.count and vv.occupied
    first = vv.voxels
    assert L.lcr_enable_voxel_grid(sim.handle, ctypes.byref(sp)) == 0          # the same spec again: nothing happens
    assert L.lcr_get_voxel_grid(sim.handle, ctypes.byref(vv)) == 0 and vv.voxels == first
    assert L.lcr_enable_voxel_grid(sim.handle, ctypes.byref(other)) == _capi.LCR_ERR_INVALID   # another spec
    msg = L.lcr_last_error()
    assert b"fixed for the life" in msg and msg.count(b"box (") == 2, msg
    was, asked = msg.split(b"asked for")
    assert b"dims 12 x 7 x 5" in was and b"dims 12 x 7 x 6" in asked and b"box (-0.200000003 0 -0.00999999978) .. (0.200000003 0.349999994 0.0599999987)" in was, msg
    sim.step(np.zeros((n, sim.action_dim), np.float32))
    _check(sim, "after a step", _raw_view(sim, L))
    sim.close()

    # close() frees the allocation: the device's free memory grows by at least the grid's 2 GiB
    import torch

    big = VecSim("push", 16384, **_kw(size, False), voxel_grid=_grid(BIG_BOX, (32, 32, 32), rgb=True))
    assert big.voxel_grid.nbytes == 2 << 30 and (big.voxel_grid_occupied.numpy() > 0).all()
    dev = big.device
    held = torch.cuda.mem_get_info(dev)[0]
    big.close()
    assert torch.cuda.mem_get_info(dev)[0] - held >= 2 << 30


def test_the_vector_adapters_refuse_the_grid(hip_lib):
    from gym_lowcostrobot_amd.vecenv import LowCostRobotVecEnv, LowCostRobotVectorEnv

    for Adapter in (LowCostRobotVecEnv, LowCostRobotVectorEnv):
        with pytest.raises(ValueError, match="cannot make the grid of the episode that ended"):
            Adapter("reach", 4, voxel_grid=_grid(CUBE_BOX, (12, 7, 5)), **_kw((16, 16), False))
