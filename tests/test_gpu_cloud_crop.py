"""The point cloud inside a crop box on the GPU (VecSim(..., point_cloud=dict(points=P, crop=(lo, hi), ...)); lcr_enable_point_cloud_cropped): the library's device buffers
against the numpy model of tests/cloud_crop_ref.py, which is fed the library's own planes, frames and reported camera poses.

What is exact: everything.  The point is pinned to the bit in this mode (include/lcr.h), and the model evaluates the same chain with an exact fused multiply-add, so the
inside test is a reproducible decision: `count`, `source`, the x y z bits and the r g b bits are compared exactly, and every output point of an env with M > 0 is held to
the inside test itself.  Under FPS the twin method of tests/test_gpu_cloud_fps.py is used: A asks for P = Q and shows the pool, the model's greedy order of it reproduces
A bit for bit, B (P < Q) is A's prefix.

The boxes were chosen on the CPU: reset states of the oracle (seeds 1000 ..), tests/planes_ref.py's planes through front and top at the test's frame size, the model's
points.  At reset the arm spans x -0.07 .. 0.09, y -0.08 .. 0.22, z 0 .. 0.185, the cubes x -0.17 .. 0.12, y 0.01 .. 0.25, z 0 .. 0.015 (metres, world frame); the float32 z
of floor points through the front camera is -2.1e-8 .. 4e-2 (the large values at grazing rays far away), through the top camera, which looks straight down, 0 exactly.
  CUBE_BOX   (-0.2, 0.0, -0.01) .. (0.2, 0.35, 0.06)   the cube's spawn region and the arm's foot in it.  reach 16 x 16, front + top, arm + cube: M = 13 .. 15 of 60 .. 62
                                                        candidates by id: 0 < M < P = 64, and less than one round of groups (32)
  FLOOR_BOX  (-0.1, -0.05, 0.0) .. (0.1, 0.2, + inf)    lo_z = 0.0 EXACTLY, a face on the floor plane; the x / y faces cut through the arm and the floor patch.  stack 36 x 52,
                                                        front + top, + floor: M = 414 .. 425 of 3 588 by id (the wrist camera adds to both): M > P = 256; of the floor pixels
                                                        176 an env are inside, 3 088 outside
  ABOVE_BOX  lo_z = 1.0, the rest open                  above everything (the arm reaches 0.19 m at reset, and 0.45 m stretched out).  push 64 x 64: M = 0 with 520 .. 544
                                                        candidates by id an env
  OPEN_BOX   all six sides open                         every candidate by id is inside: reach 128 x 128, M = 31 616 through front + top
  HALF_BOX   hi_x = 0.02, the rest open                 a half-space that cuts the arm in two: the FPS pools differ from those of a handle without a box
Each GPU case ASSERTS the regime it is there for (env-steps with M > P, with 0 < M < P, with M = 0), so a case that never reaches it fails.  On an MI355X the rollouts
gave: CUBE_BOX 280 of 280 env-steps with 0 < M < P (largest M 31); FLOOR_BOX 3 920 of 3 920 with M > P (largest M 2 380), 76 auto-resets, floor pixels of the top camera
664 898 inside and 6 063 670 outside; ABOVE_BOX 448 of 448 with M = 0 beside 1 015 098 candidates by id; OPEN_BOX 6 of 6 with M > P (largest M 47 394).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import cloud_crop_ref, cloud_fps_ref, cloud_ref

pytestmark = pytest.mark.gpu

INF = math.inf
ALL = ("front", "top", "wrist")
WITH_FLOOR = ("arm", "cube", "cube2", "floor")
CUBE_BOX = ((-0.2, 0.0, -0.01), (0.2, 0.35, 0.06))
FLOOR_BOX = ((-0.1, -0.05, 0.0), (0.1, 0.2, INF))
ABOVE_BOX = ((-INF, -INF, 1.0), (INF, INF, INF))
OPEN_BOX = ((-INF, -INF, -INF), (INF, INF, INF))
HALF_BOX = ((-INF, -INF, -INF), (0.02, INF, INF))
LOOK_BOX = ((-0.12, -0.05, 0.0), (0.12, 0.3, 0.2))
# task, n, size, P, cameras, ids, colours, box, steps
ROLLOUTS = [
    ("reach", 5, (16, 16), 64, ("front", "top"), None, False, CUBE_BOX, 55),
    ("stack", 70, (36, 52), 256, ALL, WITH_FLOOR, True, FLOOR_BOX, 55),
    ("push", 64, (64, 64), 128, ("top", "wrist"), None, False, ABOVE_BOX, 6),
    ("reach", 3, (128, 128), 1024, ALL, WITH_FLOOR, False, OPEN_BOX, 1),
]
ROLLOUT_IDS = [f"{r[0]}-n{r[1]}-{r[2][0]}x{r[2][1]}-P{r[3]}" for r in ROLLOUTS]
# task, n, size, cameras, ids, colours, Q, B's P, box, steps: one case per build of the kernel (2, 4, 8, 16 pool entries a thread)
FPS = [
    ("reach", 5, (16, 16), ("front", "top"), None, False, 128, 64, CUBE_BOX, 12),
    ("stack", 6, (36, 52), ALL, WITH_FLOOR, True, 1024, 128, HALF_BOX, 2),
    ("push", 4, (64, 64), ("front", "top"), WITH_FLOOR, False, 2048, 256, HALF_BOX, 2),
    ("reach", 3, (128, 128), ALL, WITH_FLOOR, False, 4096, 256, HALF_BOX, 1),
]
FPS_IDS = [f"{r[0]}-n{r[1]}-{r[2][0]}x{r[2][1]}-Q{r[6]}-P{r[7]}" for r in FPS]


def _cloud(P, box, cams=None, ids=None, colors=False, Q=None):
    d = dict(points=P, colors=colors, crop=box)
    if cams is not None:
        d["cameras"] = cams
    if ids is not None:
        d["ids"] = ids
    if Q is not None:
        d.update(sampling="fps", pool=Q)
    return d


def _kw(size, wrist, **more):
    return dict(observation_mode="both", image_size=size, image_planes=("depth", "segmentation"), wrist_camera=True if wrist else None, **more)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _f32_box(box):
    return {"lo": tuple(float(np.float32(v)) for v in box[0]), "hi": tuple(float(np.float32(v)) for v in box[1])}


def _inputs(sim):
    cams = sim.point_cloud_spec["cameras"]
    return ([getattr(sim, "depth_" + c).numpy() for c in cams], [getattr(sim, "seg_" + c).numpy() for c in cams], [getattr(sim, "image_" + c).numpy() for c in cams])


def _check(sim, when):
    """the invariant of a strided cloud inside a box: count, source, x y z and r g b are the header's function of the env's current planes, frames and reported poses,
    exactly -> (count, candidates by id (N, slots H W), candidates (N, slots H W))"""
    sp, box = sim.point_cloud_spec, sim.point_cloud_crop
    assert box is not None and sim.point_cloud_sampling == {"mode": "stride", "pool": 0}
    lo, hi = box["lo"], box["hi"]
    depth, seg, rgb = _inputs(sim)
    pose = sim.point_cloud_pose.numpy()
    pts, cnt, src = sim.point_cloud.numpy(), sim.point_cloud_count.numpy(), sim.point_cloud_source.numpy()
    assert pts.dtype == np.float32 and pts.shape == (sim.n, sp["points"], 6 if sp["colors"] else 3) and pose.shape == (len(sp["cameras"]), 13, sim.n)
    ids = cloud_ref.ids_mask(sp["ids"])
    want, wcnt, wsrc, cand, _ = cloud_crop_ref.cloud(depth, seg, rgb, pose, dict(points=sp["points"], ids=ids, colors=sp["colors"]), (lo, hi))
    np.testing.assert_array_equal(cnt, wcnt, err_msg=f"count, {when}")
    bad = np.argwhere(src != wsrc)
    assert bad.size == 0, (when, "source", len(bad), bad[:6].tolist())
    bad = np.argwhere(_bits(pts) != _bits(want))
    assert bad.size == 0, (when, "x y z r g b bits", len(bad), bad[:6].tolist())
    assert cloud_crop_ref.inside(pts[cnt > 0][..., :3], lo, hi).all(), (when, "a point outside the box")
    assert not pts[cnt == 0].any() and (src[cnt == 0] == -1).all() and (src[cnt > 0] >= 0).all()
    return cnt, cloud_ref.candidates(seg, ids), cand


def _check_guards(sim, when):
    from tests.test_gpu_cloud import _check_guards as guards

    guards(sim, when)


@functools.lru_cache(maxsize=None)
def _rollout(case):
    """runs one strided rollout, checking the invariant after enabling and after every step -> the regime counters"""
    from gym_lowcostrobot_amd import VecSim

    task, n, size, P, cams, ids, colors, box, steps = case
    wrist = "wrist" in cams
    sim = VecSim(task, n, base_seed=17, point_cloud=_cloud(P, box, cams, ids, colors), **_kw(size, wrist))
    assert sim.point_cloud_spec == {"points": P, "cameras": cams, "ids": tuple(i for i in range(11) if cloud_ref.ids_mask(ids) >> i & 1), "colors": colors}
    assert sim.point_cloud_crop == _f32_box(box)
    twin = VecSim(task, n, base_seed=17, point_cloud={k: v for k, v in _cloud(P, box, cams, ids, colors).items() if k != "crop"}, **_kw(size, wrist)) if box is OPEN_BOX else None
    acts = [(s_, s_.alloc_actions()) for s_ in (sim, twin) if s_ is not None]
    H, W = size
    top = cams.index("top") if "top" in cams else None
    stats = {"gt": 0, "lt": 0, "zero": 0, "resets": 0, "byid": 0, "floor_in": 0, "floor_out": 0, "maxM": 0}
    for t in range(-1, steps):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 23, t); s_.step_device(a.ptr)
            stats["resets"] += int(sim.outputs()["did_reset"].sum())
        cnt, byid, cand = _check(sim, f"step {t}")
        stats["gt"] += int((cnt > P).sum()); stats["lt"] += int(((cnt > 0) & (cnt < P)).sum()); stats["zero"] += int((cnt == 0).sum())
        stats["byid"] += int(byid.sum()); stats["maxM"] = max(stats["maxM"], int(cnt.max()))
        if top is not None and cloud_ref.ids_mask(ids) & cloud_ref.IDS["floor"]:   # floor pixels of the top camera among the candidates by id: inside / outside the box
            floor = (sim.seg_top.numpy().reshape(n, -1) & 0x7F) == 1
            sl = slice(top * H * W, (top + 1) * H * W)
            stats["floor_in"] += int((floor & cand[:, sl]).sum()); stats["floor_out"] += int((floor & byid[:, sl] & ~cand[:, sl]).sum())
        if twin is not None:   # all six sides open: the cloud of a handle without a box -- the same decisions, the same pose bits, the points within the strided cloud's bound
            assert twin.point_cloud_crop is None
            np.testing.assert_array_equal(cnt, twin.point_cloud_count.numpy(), err_msg=f"count of the twin, step {t}")
            np.testing.assert_array_equal(sim.point_cloud_source.numpy(), twin.point_cloud_source.numpy(), err_msg=f"source of the twin, step {t}")
            np.testing.assert_array_equal(_bits(sim.point_cloud_pose.numpy()), _bits(twin.point_cloud_pose.numpy()), err_msg=f"camera_pose of the twin, step {t}")
            depth = _inputs(sim)[0]
            bound = cloud_ref.xyz_bound(depth, sim.point_cloud_pose.numpy(), sim.point_cloud_source.numpy().astype(np.int64), H, W)[..., None]
            err = np.abs(sim.point_cloud.numpy().astype(np.float64) - twin.point_cloud.numpy().astype(np.float64))
            assert (err <= bound).all(), (t, float((err / bound).max()))
    for s_, a in acts:
        _check_guards(s_, "after the rollout")
    np.testing.assert_array_equal(sim.observations()["point_cloud"], sim.point_cloud.numpy())
    for s_, a in acts:
        s_.free(a); s_.close()
    print(f"cropped cloud rollout {case[:4]}: {stats}, model fallbacks so far {cloud_crop_ref.FALLBACKS[0]}")
    return stats


@pytest.mark.parametrize("case", ROLLOUTS, ids=ROLLOUT_IDS)
def test_rollout_against_the_model(hip_lib, case):
    """Random actions; after enabling and after every step count, source, x y z and r g b are the model's, exactly, every point lies inside the box, and the case is in the
    regime it is there for.  The stack case at lo_z = 0.0 exactly is the one that catches arithmetic that is not pinned: floor pixels of the top camera fall inside and
    outside the box.  The open box runs beside a handle without a crop"""
    task, n, size, P, cams, ids, colors, box, steps = case
    st = _rollout(case)
    checks = n * (steps + 1)
    if steps >= 55:
        assert st["resets"] >= n, st          # 55 steps cross an auto-reset of every env
    if box is CUBE_BOX:
        assert st["lt"] > 0 and st["gt"] == 0 and st["maxM"] < 32 * 16, st
    if box is FLOOR_BOX:
        assert st["gt"] > checks // 2 and st["floor_in"] > 0 and st["floor_out"] > 0, st
    if box is ABOVE_BOX:
        assert st["zero"] == checks and st["byid"] > 0, st   # M = 0 everywhere although candidates by id exist
    if box is OPEN_BOX:
        assert st["gt"] == checks, st


def test_the_rollouts_cover_every_regime(hip_lib):
    """together the cases contain env-steps with M > P, with 0 < M < P and with M = 0 (rollouts already run are not run again)"""
    tot = {k: sum(_rollout(c)[k] for c in ROLLOUTS) for k in ("gt", "lt", "zero")}
    assert tot["gt"] > 0 and tot["lt"] > 0 and tot["zero"] > 0, tot


def _check_twins(A, B, Q, when):
    """everything the header says of an FPS cloud inside a box, for the twins A (P = Q) and B (P < Q) -> (count, A's sources)"""
    sp, box = A.point_cloud_spec, A.point_cloud_crop
    assert sp["points"] == Q and A.point_cloud_sampling == B.point_cloud_sampling == {"mode": "fps", "pool": Q} and box is not None and B.point_cloud_crop == box
    lo, hi = box["lo"], box["hi"]
    PB = B.point_cloud_spec["points"]
    cams, colors = sp["cameras"], sp["colors"]
    H, W = A.image_size
    depth, seg, rgb = _inputs(A)
    for c, d, s, f in zip(cams, depth, seg, rgb):   # a difference here is not this feature's
        np.testing.assert_array_equal(_bits(d), _bits(getattr(B, "depth_" + c).numpy()), err_msg=f"depth_{c} of the twins, {when}")
        np.testing.assert_array_equal(s, getattr(B, "seg_" + c).numpy(), err_msg=f"seg_{c} of the twins, {when}")
        np.testing.assert_array_equal(f, getattr(B, "image_" + c).numpy(), err_msg=f"image_{c} of the twins, {when}")
    pose = A.point_cloud_pose.numpy()
    np.testing.assert_array_equal(_bits(pose), _bits(B.point_cloud_pose.numpy()), err_msg=f"camera_pose of the twins, {when}")
    pts, cnt, src = A.point_cloud.numpy(), A.point_cloud_count.numpy(), A.point_cloud_source.numpy()
    C = 6 if colors else 3
    assert pts.dtype == np.float32 and pts.shape == (A.n, Q, C) and src.shape == (A.n, Q) and pose.shape == (len(cams), 13, A.n)

    # count and the pool: the model's candidates, exactly
    p = cloud_crop_ref.points_f32(depth, pose, H, W)
    cand = cloud_crop_ref.candidates(seg, cloud_ref.ids_mask(sp["ids"]), depth, pose, (lo, hi), p)
    M = cand.sum(axis=1)
    np.testing.assert_array_equal(cnt, M, err_msg=f"count, {when}")
    np.testing.assert_array_equal(B.point_cloud_count.numpy(), M, err_msg=f"count of B, {when}")
    pool_src = np.stack([cloud_fps_ref.pool_sources(cand[e], Q) for e in range(A.n)])
    by_source = np.argsort(src, axis=1, kind="stable")
    env = np.arange(A.n)[:, None]
    np.testing.assert_array_equal(src[env, by_source], pool_src, err_msg=f"A's sources as a multiset, {when}")

    # the points: the model's pinned bits at their sources, every one inside the box; the colours by the stack's rule
    live = M > 0
    assert not pts[~live].any() and (src[~live] == -1).all()
    want = np.zeros_like(pts)
    want[..., :3] = p[env, np.maximum(src, 0)]
    if colors:
        flat = np.concatenate([f.reshape(A.n, -1, 3) for f in rgb], axis=1)
        want[..., 3:] = flat[env, np.maximum(src, 0)].astype(np.float32) * cloud_ref.INV255
    want[~live] = 0
    bad = np.argwhere(_bits(pts) != _bits(want))
    assert bad.size == 0, (when, "x y z r g b bits", len(bad), bad[:6].tolist())
    assert cloud_crop_ref.inside(pts[live][..., :3], lo, hi).all(), (when, "a point outside the box")

    # the greedy order of the pool A has shown, by the model: sources and point bits exactly
    if live.any():
        pool = pts[env, by_source][live]                      # (n', Q, C) in pool order (equal sources are the same candidate: the same point)
        order = cloud_fps_ref.fps_order(np.ascontiguousarray(pool[..., :3]), Q)
        rows = np.arange(pool.shape[0])[:, None]
        bad = np.argwhere(pool_src[live][rows, order] != src[live])
        assert bad.size == 0, (when, "greedy order, sources", len(bad), bad[:6].tolist())
        bad = np.argwhere(_bits(pool[rows, order]) != _bits(pts[live]))
        assert bad.size == 0, (when, "greedy order, point bits", len(bad), bad[:6].tolist())
        assert (src[live][:, 0] == pool_src[live][:, 0]).all()   # the first point is pool entry 0

    # B is the prefix of A
    np.testing.assert_array_equal(B.point_cloud_source.numpy(), src[:, :PB], err_msg=f"B's sources, {when}")
    np.testing.assert_array_equal(_bits(B.point_cloud.numpy()), _bits(pts[:, :PB]), err_msg=f"B's points, {when}")
    return cnt, src


@pytest.mark.parametrize("case", FPS, ids=FPS_IDS)
def test_fps_under_crop_bit_for_bit(hip_lib, case):
    """The twins of every kernel build, and a third handle without a box and with the same seeds: the box cuts the arm, so the pools differ"""
    from gym_lowcostrobot_amd import VecSim

    task, n, size, cams, ids, colors, Q, PB, box, steps = case
    wrist = "wrist" in cams
    A = VecSim(task, n, base_seed=17, point_cloud=_cloud(Q, box, cams, ids, colors, Q), **_kw(size, wrist))
    B = VecSim(task, n, base_seed=17, point_cloud=_cloud(PB, box, cams, ids, colors, Q), **_kw(size, wrist))
    U = VecSim(task, n, base_seed=17, point_cloud={k: v for k, v in _cloud(Q, box, cams, ids, colors, Q).items() if k != "crop"}, **_kw(size, wrist))
    assert A.point_cloud_crop == B.point_cloud_crop == _f32_box(box) and U.point_cloud_crop is None
    acts = [(s_, s_.alloc_actions()) for s_ in (A, B, U)]
    stats = {"gt": 0, "lt": 0, "zero": 0, "differ": 0}
    for t in range(-1, steps):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 23, t); s_.step_device(a.ptr)
        cnt, src = _check_twins(A, B, Q, f"step {t}")
        stats["gt"] += int((cnt > Q).sum()); stats["lt"] += int(((cnt > 0) & (cnt < Q)).sum()); stats["zero"] += int((cnt == 0).sum())
        np.testing.assert_array_equal(_bits(A.point_cloud_pose.numpy()), _bits(U.point_cloud_pose.numpy()), err_msg=f"camera_pose beside the handle without a box, step {t}")
        assert (U.point_cloud_count.numpy() >= cnt).all()
        stats["differ"] += int((np.sort(src, axis=1) != np.sort(U.point_cloud_source.numpy(), axis=1)).any(axis=1).sum())
    for s_, a in acts:
        _check_guards(s_, "after the rollout")
        s_.free(a); s_.close()
    print(f"cropped fps {case[0]} n {n} Q {Q}: {stats}, model fallbacks so far {cloud_fps_ref.FALLBACKS[0]} + {cloud_crop_ref.FALLBACKS[0]}")
    checks = n * (steps + 1)
    assert stats["differ"] == checks, stats          # the box changed the pool of every env
    if Q == 128:
        assert stats["lt"] > 0 and stats["gt"] == 0, stats
    else:
        assert stats["gt"] == checks, stats


def test_per_env_cameras(hip_lib):
    """With look variants that move and turn the cameras and change the fovy, redrawn per env at every auto-reset, and after set_look, the inside decisions follow each
    env's own reported pose: the invariant holds, and envs of different variants are in play"""
    from gym_lowcostrobot_amd import VecSim
    from tests import look_ref

    n, size = 12, (96, 96)
    sim = VecSim("push", n, base_seed=5, max_episode_steps=3, look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 9},
                 point_cloud=_cloud(128, LOOK_BOX, ("front", "top"), WITH_FLOOR, True), **_kw(size, False))
    act = sim.alloc_actions()
    seen, Ms = set(), []
    for t in range(-1, 4):
        if t >= 0:
            sim.fill_random_actions(act, 3, t); sim.step_device(act.ptr)
        cnt, byid, cand = _check(sim, f"step {t}")
        Ms.append(cnt)
        seen |= set(sim.look()["variant"].tolist())
        assert (cand.sum(axis=1) < byid.sum(axis=1)).all() and (cnt > 0).all()
    assert len(seen) > 1   # the envs did change variants
    before, pose_before = sim.point_cloud.numpy(), sim.point_cloud_pose.numpy()
    variant = ((np.arange(n) + 1) % len(look_ref.GPU_VARIANTS)).astype(np.int32)
    sim.set_look(variant=variant, rgb=np.random.default_rng(1).uniform(0, 1, (9, n)).astype(np.float32))
    _check(sim, "set_look")
    assert (sim.point_cloud_pose.numpy() != pose_before).any() and (sim.point_cloud.numpy() != before).any()
    _check_guards(sim, "after set_look")
    sim.free(act); sim.close()


def test_the_entry_points_that_are_not_the_step(hip_lib):
    """After reset(), a masked reset, set_state followed by the all-zero-mask reset, and set_look on a handle with look variants the cloud is the header's function of the
    current frames: the FPS twins at 96 x 96 with two cameras, Q = 1024, inside a box"""
    from gym_lowcostrobot_amd import VecSim

    n, size, Q, PB = 6, (96, 96), 1024, 128
    variants = [{}, {"cam_dpos": [[0.03, 0.0, 0.02], [0.0, 0.04, 0.05]], "fovy_deg": [50.0, 40.0]}]
    kw = _kw(size, False, base_seed=2, look_variants=variants)
    twins = [VecSim("push", n, point_cloud=_cloud(P, LOOK_BOX, ("front", "top"), ("arm", "cube", "floor"), True, Q), **kw) for P in (Q, PB)]
    A, B = twins
    rng = np.random.default_rng(4)
    _check_twins(A, B, Q, "enabled")
    for t in range(2):
        a = rng.uniform(-1, 1, (n, A.action_dim)).astype(np.float32)
        for s_ in twins:
            s_.step(a)
    cnt, _ = _check_twins(A, B, Q, "steps")
    assert (cnt > Q).all()

    before = A.point_cloud.numpy()
    for s_ in twins:
        s_.reset()
    _check_twins(A, B, Q, "reset()")
    assert (A.point_cloud.numpy() != before).any()

    before = A.point_cloud.numpy()
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    for s_ in twins:
        s_.reset(mask=mask, seeds=np.arange(100, 100 + n, dtype=np.uint64))
    _check_twins(A, B, Q, "reset(mask)")
    after = A.point_cloud.numpy()
    np.testing.assert_array_equal(after[mask == 0], before[mask == 0])
    assert (after[mask == 1] != before[mask == 1]).any()

    qpos = A.get_state()["qpos"]
    qpos[:5] += rng.uniform(-0.3, 0.3, (5, n))
    for s_ in twins:
        s_.set_state(qpos=qpos)
        s_.reset(mask=np.zeros(n, np.uint8))
    _check_twins(A, B, Q, "reset(zeros) after set_state")
    assert (A.point_cloud.numpy() != after).any()

    before = A.point_cloud.numpy()
    variant, rgb9 = (np.arange(n) % 2).astype(np.int32), rng.uniform(0, 1, (9, n)).astype(np.float32)
    for s_ in twins:
        s_.set_look(variant=variant, rgb=rgb9)
    _check_twins(A, B, Q, "set_look")
    assert (A.point_cloud.numpy()[variant == 1] != before[variant == 1]).any()
    for s_ in twins:
        _check_guards(s_, "after the entry points")
        s_.close()


@pytest.mark.parametrize("Q", [None, 2048], ids=["stride", "fps-Q2048"])
def test_cropped_cloud_on_the_second_stream_is_the_serial_cloud(hip_lib, monkeypatch, Q):
    """The same seeded rollout of ten steps with frames and cloud on the caller's stream (LCR_RENDER_OVERLAP=0) and on the second stream: identical bits, across auto-resets
    that redraw the looks"""
    from gym_lowcostrobot_amd import VecSim
    from tests import look_ref

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=3, max_episode_steps=3, look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 7},
             point_cloud=_cloud(256, FLOOR_BOX, None, WITH_FLOOR, True, Q))
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", n, **kw)
    acts = [(s_, s_.alloc_actions()) for s_ in (ref, ovl)]
    for t in range(-1, 10):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
        for name in ("point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose"):
            np.testing.assert_array_equal(_bits(getattr(ref, name).numpy()), _bits(getattr(ovl, name).numpy()), err_msg=f"{name}, step {t}")
    assert (ovl.point_cloud_count.numpy() > 0).all() and ovl.point_cloud.numpy().std() > 0.01
    if Q is None:
        _check(ovl, "second stream")
    for s_, a in acts:
        _check_guards(s_, "after the rollout")
        s_.free(a); s_.close()


def test_sharded_cropped_cloud_is_the_unsharded_cloud(hip_lib):
    """Two shards of 64 envs (the cut falls on a wave boundary of the step kernels) keep the cloud of the unsharded 128-env handle, bit for bit; every shard has the box"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    box = ((-0.15, -0.05, 0.0), (0.15, 0.3, 0.1))
    kw = _kw((16, 16), True, base_seed=9, max_episode_steps=3, point_cloud=_cloud(64, box, None, WITH_FLOOR, True))
    one = VecSim("push", 128, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], **kw)
    assert all(s_.point_cloud.shape == (64, 64, 6) and s_.point_cloud_spec == one.point_cloud_spec and s_.point_cloud_crop == one.point_cloud_crop == _f32_box(box) for s_ in sh.shards)
    act = one.alloc_actions()
    for t in range(5):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        for name, axis in (("point_cloud", 0), ("point_cloud_count", 0), ("point_cloud_source", 0), ("point_cloud_pose", 2)):
            got = np.concatenate([getattr(s_, name).numpy() for s_ in sh.shards], axis=axis)
            np.testing.assert_array_equal(_bits(got), _bits(getattr(one, name).numpy()), err_msg=f"{name}, step {t}")
    cnt, byid, cand = _check(one, "after the steps")
    assert (cnt > 0).all() and (cand.sum(axis=1) < byid.sum(axis=1)).all() and one.point_cloud.numpy().std() > 0.02
    one.free(act); one.close(); sh.close()


def test_life_cycle(hip_lib):
    """The same spec, sampling and crop again is a no-op; another box is refused and both boxes are in the message; a crop on a handle enabled without one, and the reverse,
    are refused; the getter on handles with and without a crop, and without a cloud"""
    from gym_lowcostrobot_amd import VecSim, _capi

    L = hip_lib
    n, size = 5, (16, 16)
    sp = _capi.PointCloudSpec.from_any(64)
    fps = _capi.PointCloudSampling(mode=1, pool=128)

    def crop(lo, hi):
        c = _capi.PointCloudCrop()
        for k in range(3):
            c.lo[k], c.hi[k] = lo[k], hi[k]
        return c

    def getter(sim):
        on, out = ctypes.c_int32(7), crop((7, 7, 7), (7, 7, 7))
        assert L.lcr_get_point_cloud_crop(sim.handle, ctypes.byref(on), ctypes.byref(out)) == 0
        return on.value, tuple(out.lo), tuple(out.hi)

    box = crop((-0.2, 0.0, -0.01), (0.2, 0.35, INF))
    other = crop((-0.2, 0.0, -0.01), (0.2, 0.375, INF))

    state = VecSim("push", n, observation_mode="state")
    assert L.lcr_enable_point_cloud_cropped(state.handle, ctypes.byref(sp), None, ctypes.byref(box)) == _capi.LCR_ERR_INVALID and b"no image observations" in L.lcr_last_error()
    assert getter(state) == (0, (0.0,) * 3, (0.0,) * 3)                       # a handle without a cloud
    assert state.point_cloud_crop is None
    state.close()

    sim = VecSim("push", n, **_kw(size, False))
    assert getter(sim) == (0, (0.0,) * 3, (0.0,) * 3)
    assert L.lcr_enable_point_cloud_cropped(sim.handle, ctypes.byref(sp), ctypes.byref(fps), ctypes.byref(box)) == 0   # enabled late, on a live handle
    f = np.float32
    assert getter(sim) == (1, (float(f(-0.2)), 0.0, float(f(-0.01))), (float(f(0.2)), float(f(0.35)), INF))
    cv = _capi.LcrPointCloudView()
    assert L.lcr_get_point_cloud(sim.handle, ctypes.byref(cv)) == 0 and cv.enabled == 1 and cv.spec.points == 64
    first = cv.points
    assert L.lcr_enable_point_cloud_cropped(sim.handle, ctypes.byref(sp), ctypes.byref(fps), ctypes.byref(box)) == 0   # the same triple again: nothing happens
    assert L.lcr_get_point_cloud(sim.handle, ctypes.byref(cv)) == 0 and cv.points == first
    assert L.lcr_enable_point_cloud_cropped(sim.handle, ctypes.byref(sp), ctypes.byref(fps), ctypes.byref(other)) == _capi.LCR_ERR_INVALID   # another box
    msg = L.lcr_last_error()
    assert b"fixed for the life" in msg and msg.count(b"crop lo (") == 2, msg
    was, asked = msg.split(b"asked for")
    assert b"crop lo (-0.200000003 0 -0.00999999978) hi (0.200000003 0.349999994 inf)" in was and b"sampling fps, pool 128" in was, msg
    assert b"crop lo (-0.200000003 0 -0.00999999978) hi (0.200000003 0.375 inf)" in asked and b"sampling fps, pool 128" in asked, msg
    for call in (lambda: L.lcr_enable_point_cloud_cropped(sim.handle, ctypes.byref(sp), ctypes.byref(fps), None),             # the reverse: no box on a handle with one
                 lambda: L.lcr_enable_point_cloud_sampled(sim.handle, ctypes.byref(sp), ctypes.byref(fps)),
                 lambda: L.lcr_enable_point_cloud(sim.handle, ctypes.byref(sp))):
        assert call() == _capi.LCR_ERR_INVALID
        msg = L.lcr_last_error()
        assert b"fixed for the life" in msg and b"crop lo (" in msg.split(b"asked for")[0] and b"no crop" in msg.split(b"asked for")[1], msg
    assert L.lcr_enable_point_cloud_cropped(sim.handle, ctypes.byref(sp), None, ctypes.byref(box)) == _capi.LCR_ERR_INVALID   # the same box, another sampling
    assert b"sampling stride, pool 0" in L.lcr_last_error().split(b"asked for")[1]
    sim.step(np.zeros((n, sim.action_dim), np.float32))
    out = np.empty((n, 64, 3), np.float32)
    assert L.lcr_memcpy_d2h(sim.handle, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(cv.points), out.nbytes) == 0
    assert np.isfinite(out).all() and cloud_crop_ref.inside(out[out.any(axis=(1, 2))], tuple(box.lo), tuple(box.hi)).all()
    sim.close()

    plain = VecSim("push", n, point_cloud=64, **_kw(size, False))              # a cloud without a box
    assert plain.point_cloud_crop is None and getter(plain) == (0, (0.0,) * 3, (0.0,) * 3)
    assert L.lcr_enable_point_cloud_cropped(plain.handle, ctypes.byref(sp), None, ctypes.byref(box)) == _capi.LCR_ERR_INVALID   # a crop on a handle enabled without one
    msg = L.lcr_last_error()
    assert b"fixed for the life" in msg and b"no crop" in msg.split(b"asked for")[0] and b"crop lo (-0.200000003" in msg.split(b"asked for")[1], msg
    assert L.lcr_enable_point_cloud_cropped(plain.handle, ctypes.byref(sp), None, None) == 0                                   # the same cloud again, by the new call
    # without a crop on either side the refusals are today's, byte for byte
    assert L.lcr_enable_point_cloud_cropped(plain.handle, ctypes.byref(_capi.PointCloudSpec.from_any(128)), None, None) == _capi.LCR_ERR_INVALID
    assert L.lcr_last_error() == b"a point cloud (points 64, cameras 3, ids 0x7fc, colors 0) is enabled already and fixed for the life of the handle"
    assert getter(plain) == (0, (0.0,) * 3, (0.0,) * 3)
    plain.close()


def test_a_handle_without_a_crop_is_untouched(hip_lib):
    """dict(spec) and dict(spec, crop=None) give byte-equal clouds over five steps, the strided cloud of tests/cloud_ref.py; point_cloud_crop is None and the spec and the
    sampling keep their keys"""
    from gym_lowcostrobot_amd import VecSim
    from tests.test_gpu_cloud import _check as check_strided

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=21, max_episode_steps=4)
    spec = dict(points=256, ids=WITH_FLOOR, colors=True)
    named = VecSim("stack", n, point_cloud=dict(spec, crop=None), **kw)
    plain = VecSim("stack", n, point_cloud=spec, **kw)
    assert named.point_cloud_crop is None and plain.point_cloud_crop is None
    assert named.point_cloud_spec == plain.point_cloud_spec and sorted(plain.point_cloud_spec) == ["cameras", "colors", "ids", "points"]
    assert named.point_cloud_sampling == plain.point_cloud_sampling == {"mode": "stride", "pool": 0}
    acts = [(s_, s_.alloc_actions()) for s_ in (named, plain)]
    for t in range(-1, 5):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 11, t); s_.step_device(a.ptr)
        for name in ("point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose"):
            np.testing.assert_array_equal(_bits(getattr(named, name).numpy()), _bits(getattr(plain, name).numpy()), err_msg=f"{name}, step {t}")
    check_strided(named, "crop=None")
    for s_, a in acts:
        _check_guards(s_, "after the rollout")
        s_.free(a); s_.close()
    none = VecSim("stack", 4, **_kw((16, 16), False))
    assert none.point_cloud is None and none.point_cloud_crop is None
    none.close()
