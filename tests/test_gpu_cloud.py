"""The point cloud on the GPU (VecSim(..., point_cloud=...); lcr_enable_point_cloud): the library's device buffers against the numpy model of tests/cloud_ref.py, which
is fed the library's own planes, frames and reported camera poses.

What is exact and what has a bound.  `count` and `source` are integer decisions on the GPU's own segmentation bytes: compared exactly.  The r g b channels are one float32
multiply of a byte: compared bit for bit.  The x y z channels are float32 evaluations of p = ro + t (sx X + sy Y - Z); the model forms the same expression in fp64 from the
same float32 inputs (the GPU's depth, the reported pose).  Per component the float32 evaluation rounds at most six times under any association or fma contraction -- sx,
sy (one multiply each: the bracket (px + 0.5 - 0.5 W) is an exact half-integer), the two products / sums that make d, the product t d, the sum with ro -- and every
intermediate is bounded by |ro|_inf + t (|sx| + |sy| + 1) (the axes' components are at most 1 in magnitude).  Six roundings of relative size 2^-24 on quantities below that
magnitude give less than 6 x 2^-24 of it; the tests assert 8 x 2^-23 x (|ro|_inf + t (|sx| + |sy| + 1)) per component (cloud_ref.xyz_bound), the bound of the issue.

Shapes of the rollouts, the smallest at which the kernel can go wrong (a workgroup is one env; its 256 threads count 256 groups of 16 pixels per round, four rounds in
flight at a time; 64 groups are a segment of the prefix):
  reach  n 5   16 x 16    P 128   front + top          2 x 16 groups: less than one wave's round; 0 < M < P
  reach  n 5   16 x 16    P 64    front + top          the smallest P.  tests/planes_ref.py puts M of the reset states at 61 .. 64 here (checked on the CPU), astride P, which
                                                       is why the case above, with P = 128, is the one that is held to 0 < M < P
  stack  n 70  36 x 52    P 256   all three, + floor   351 groups: a ragged second round, a partial last segment; x y z r g b; M > P (the reference: 5 304 of 5 616 pixels)
  push   n 64  64 x 64    P 128   top + wrist          ids = second cube only, which a one-cube task never draws: M = 0 everywhere
  reach  n 3   512 x 512  P 8192  all three, + floor   49 152 groups, the largest LDS case, and (2 j + 1) M beyond 2^32; one step only
The look test runs at 96 x 96 with two cameras: 1 152 groups are five rounds, a full batch of four and a ragged one.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import cloud_ref

pytestmark = pytest.mark.gpu

ALL = ("front", "top", "wrist")
WITH_FLOOR = ("arm", "cube", "cube2", "floor")
# task, n, size, P, cameras, ids, colours, steps
ROLLOUTS = [
    ("reach", 5, (16, 16), 128, ("front", "top"), None, False, 55),
    ("reach", 5, (16, 16), 64, ("front", "top"), None, False, 55),
    ("stack", 70, (36, 52), 256, ALL, WITH_FLOOR, True, 55),
    ("push", 64, (64, 64), 128, ("top", "wrist"), ("cube2",), False, 55),
    ("reach", 3, (512, 512), 8192, ALL, WITH_FLOOR, False, 1),
]
ROLLOUT_IDS = [f"{r[0]}-n{r[1]}-{r[2][0]}x{r[2][1]}-P{r[3]}" for r in ROLLOUTS]
# The wrist pose: the kernel's float32 chain of at most seven frame compositions at magnitudes <= 1 m against tests/wrist_ref.py's fp64 pose of the same float32 joint
# angles.  Measured on an MI355X over the rollouts below (largest component difference over ro, X, Y, Z and s, all envs and steps): 2.17e-7 (stack 1.91e-7, push 2.17e-7, the
# 512 x 512 case 8.5e-8).  The bound is 4 x that.
WRIST_POSE_MEASURED = 2.17e-7
WRIST_POSE_BOUND = 4 * WRIST_POSE_MEASURED
LOOK_CAMERA_TOL = 1e-4   # what tests/test_gpu_look.py holds the planes drawn through the variants' cameras to


def _spec(P, cams=None, ids=None, colors=False):
    d = dict(points=P, colors=colors)
    if cams is not None:
        d["cameras"] = cams
    if ids is not None:
        d["ids"] = ids
    return d


def _kw(size, wrist, **more):
    return dict(observation_mode="both", image_size=size, image_planes=("depth", "segmentation"), wrist_camera=True if wrist else None, **more)


def _inputs(sim):
    cams = sim.point_cloud_spec["cameras"]
    return ([getattr(sim, "depth_" + c).numpy() for c in cams], [getattr(sim, "seg_" + c).numpy() for c in cams], [getattr(sim, "image_" + c).numpy() for c in cams])


def _check(sim, when):
    """the invariant: cloud, count and source are the header's function of the env's current planes, frames and reported poses -> (count, largest error / bound)"""
    sp = sim.point_cloud_spec
    H, W = sim.image_size
    depth, seg, rgb = _inputs(sim)
    pose = sim.point_cloud_pose.numpy()
    pts, cnt, src = sim.point_cloud.numpy(), sim.point_cloud_count.numpy(), sim.point_cloud_source.numpy()
    assert pts.dtype == np.float32 and pts.shape == (sim.n, sp["points"], 6 if sp["colors"] else 3) and pose.shape == (len(sp["cameras"]), 13, sim.n)
    want, wcnt, wsrc = cloud_ref.cloud(depth, seg, rgb, pose, dict(points=sp["points"], ids=cloud_ref.ids_mask(sp["ids"]), colors=sp["colors"]))
    np.testing.assert_array_equal(cnt, wcnt, err_msg=f"count, {when}")
    bad = np.argwhere(src != wsrc)
    assert bad.size == 0, (when, "source", len(bad), bad[:6].tolist())
    if sp["colors"]:
        bad = np.argwhere(pts[..., 3:].view(np.uint32) != want[..., 3:].astype(np.float32).view(np.uint32))
        assert bad.size == 0, (when, "rgb", len(bad), bad[:6].tolist())
    bound = cloud_ref.xyz_bound(depth, pose, np.asarray(src, np.int64), H, W)[..., None]
    err = np.abs(pts[..., :3].astype(np.float64) - want[..., :3])
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (when, "xyz", len(bad), bad[:6].tolist(), float((err / bound).max()))
    assert not pts[cnt == 0].any() and (src[cnt == 0] == -1).all() and (src[cnt > 0] >= 0).all()
    return cnt, float((err / bound).max())


def _check_guards(sim, when):
    from gym_lowcostrobot_amd import _capi
    from tests.test_gpu_wrist import _guards

    for side, g in zip(("before", "behind"), _guards(sim, sim.point_cloud)):
        assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (when, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())


def _scene_camera_f32(task, cam, H):
    """ro, X, Y, Z, s of a scene camera as the library holds it: the fp64 pose of oracle.render_oracle.camera and s = 2 tan(45 deg / 2) / H, rounded to float32"""
    from oracle import render_oracle

    pos, X, Y, Z = render_oracle.camera(task, "camera_" + cam)
    return np.concatenate([pos, X, Y, Z, [2.0 * np.tan(np.radians(45.0) / 2) / H]]).astype(np.float32)


def _wrist_pose_distance(sim, pose_wrist):
    """largest component difference between the reported wrist pose (13, N) and tests/wrist_ref.py's fp64 pose of the handle's current joint angles"""
    from tests import wrist_ref

    w = sim.wrist_camera
    m = wrist_ref.mount(w["link"], w["pos"], w["xyaxes"], w["fovy_deg"])
    qpos = sim.get_state()["qpos"]
    s = float(np.float32(2.0 * np.tan(np.radians(m["fovy_deg"]) / 2) / sim.image_size[0]))
    worst = 0.0
    for e in range(sim.n):
        ref = np.concatenate(list(wrist_ref.camera(m, qpos[:, e])) + [[s]])
        worst = max(worst, float(np.abs(pose_wrist[:, e].astype(np.float64) - ref).max()))
    return worst


@functools.lru_cache(maxsize=None)
def _rollout(case):
    """runs one rollout, checking the invariant after enabling and after every step -> {"gt": env-steps with M > P, "lt": with 0 < M < P, "zero": with M = 0, ...}"""
    from gym_lowcostrobot_amd import VecSim

    task, n, size, P, cams, ids, colors, steps = case
    wrist = "wrist" in cams
    sim = VecSim(task, n, base_seed=17, point_cloud=_spec(P, cams, ids, colors), **_kw(size, wrist))
    assert sim.point_cloud_spec == {"points": P, "cameras": cams, "ids": tuple(i for i in range(11) if cloud_ref.ids_mask(ids) >> i & 1), "colors": colors}
    act = sim.alloc_actions()
    stats = {"gt": 0, "lt": 0, "zero": 0, "resets": 0, "ratio": 0.0, "wrist": 0.0, "maxM": 0}
    fixed = {c: _scene_camera_f32(task, c, size[0]) for c in cams if c != "wrist"}
    for t in range(-1, steps):
        if t >= 0:
            sim.fill_random_actions(act, 23, t); sim.step_device(act.ptr)
            stats["resets"] += int(sim.outputs()["did_reset"].sum())
        cnt, ratio = _check(sim, f"step {t}")
        stats["gt"] += int((cnt > P).sum()); stats["lt"] += int(((cnt > 0) & (cnt < P)).sum()); stats["zero"] += int((cnt == 0).sum())
        stats["ratio"] = max(stats["ratio"], ratio); stats["maxM"] = max(stats["maxM"], int(cnt.max()))
        pose = sim.point_cloud_pose.numpy()
        for i, c in enumerate(cams):
            if c == "wrist":
                stats["wrist"] = max(stats["wrist"], _wrist_pose_distance(sim, pose[i]))
            else:   # 2a: the handle's cameras, bit for bit, in every env
                bad = np.argwhere(pose[i].view(np.uint32) != fixed[c].view(np.uint32)[:, None])
                assert bad.size == 0, (c, t, bad[:6].tolist())
    _check_guards(sim, "after the rollout")
    obs = sim.observations()
    assert [k for k in obs if k.startswith(("image_", "depth_", "segmentation_", "point_"))][-1] == "point_cloud"   # behind the existing image keys
    np.testing.assert_array_equal(obs["point_cloud"], sim.point_cloud.numpy())
    sim.free(act); sim.close()
    print(f"point cloud rollout {case[:4]}: {stats}")
    return stats


@pytest.mark.parametrize("case", ROLLOUTS, ids=ROLLOUT_IDS)
def test_rollout_against_the_model(hip_lib, case):
    """1 (+ 2a, 2c, 6a).  Random actions with the default episode length of 50: the rollouts of 55 steps cross an auto-reset of every env.  After enabling and after every
    step the planes, frames, poses, cloud, count and source are read and held to the model; front and top poses are the scene cameras bit for bit; the wrist pose is
    within its bound of the fp64 chain; the guards are intact at the end."""
    task, n, size, P, cams, ids, colors, steps = case
    st = _rollout(case)
    if steps > 1:
        assert st["resets"] >= n, st
    if (task, P) == ("reach", 128):
        assert st["lt"] > 0, st
    if task == "stack":
        assert st["gt"] == n * (steps + 1) and st["lt"] == 0 and st["zero"] == 0, st
    if task == "push":
        assert st["zero"] == n * (steps + 1), st
    if size == (512, 512):
        assert st["gt"] == n * (steps + 1) and (2 * P - 1) * st["maxM"] > 2 ** 32, st   # the index needs its 64 bits
    assert st["wrist"] <= WRIST_POSE_BOUND, st


def test_the_rollouts_cover_every_regime(hip_lib):
    """1.  Together the cases contain env-steps with M > P, with 0 < M < P and with M = 0 (rollouts already run by the test above are not run again)"""
    tot = {k: sum(_rollout(c)[k] for c in ROLLOUTS) for k in ("gt", "lt", "zero")}
    assert tot["gt"] > 0 and tot["lt"] > 0 and tot["zero"] > 0, tot


def test_reported_poses_with_look_variants(hip_lib):
    """2b.  With variants that move and turn the cameras and change the fovy, redrawn per env at every auto-reset, the reported front / top poses are the cameras of
    tests/look_ref.py for the env's CURRENT variant; the cloud made with them satisfies the invariant"""
    from gym_lowcostrobot_amd import VecSim
    from tests import look_ref

    n, size = 24, (96, 96)
    sim = VecSim("push", n, base_seed=5, max_episode_steps=3, look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 9, "cube": ([0.2, 0, 0], [1, 0.4, 0.4])},
                 point_cloud=_spec(128, ("front", "top"), WITH_FLOOR, True), **_kw(size, False))
    act = sim.alloc_actions()
    seen, worst = set(), 0.0
    for t in range(-1, 7):
        if t >= 0:
            sim.fill_random_actions(act, 3, t); sim.step_device(act.ptr)
        _check(sim, f"step {t}")
        pose, variant = sim.point_cloud_pose.numpy().astype(np.float64), sim.look()["variant"]
        seen |= set(variant.tolist())
        for e in range(n):
            for i, c in enumerate(("front", "top")):
                pos, X, Y, Z, fovy = look_ref.camera("push", "camera_" + c, look_ref.GPU_VARIANTS[variant[e]])
                s = 2.0 * np.tan(np.radians(fovy) / 2) / size[0]
                d = max(np.abs(pose[i, :12, e] - np.concatenate([pos, X, Y, Z])).max(), abs(pose[i, 12, e] - s) / s)
                worst = max(worst, float(d))
                assert d <= LOOK_CAMERA_TOL, (t, e, c, d)
    assert len(seen) > 1   # the envs did change variants
    print(f"look cameras: largest distance of a reported pose from tests/look_ref.py {worst:.3g}")
    sim.free(act); sim.close()


def test_invariant_after_the_entry_points_that_are_not_the_step(hip_lib):
    """3.  After enabling, reset(), a masked reset, set_state followed by the no-op reset, and set_look the invariant holds, and what each call changes shows in the cloud"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 70, (36, 52)
    sim = VecSim("push", n, base_seed=2, look_variants=[{}, {"cam_dpos": [[0.03, 0.0, 0.02], [0.0, 0.04, 0.05]], "fovy_deg": [50.0, 40.0]}],
                 point_cloud=_spec(192, None, ("arm", "cube"), True), **_kw(size, True))
    assert sim.point_cloud_spec["cameras"] == ALL   # cameras 0: every camera the handle has
    rng = np.random.default_rng(4)
    _check(sim, "enabled")
    for t in range(3):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
    _check(sim, "steps")

    before = sim.point_cloud.numpy()
    sim.reset()
    _check(sim, "reset()")
    assert (sim.point_cloud.numpy() != before).any()

    before = sim.point_cloud.numpy()
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    sim.reset(mask=mask, seeds=np.arange(100, 100 + n, dtype=np.uint64))
    _check(sim, "reset(mask)")
    after = sim.point_cloud.numpy()
    np.testing.assert_array_equal(after[mask == 0], before[mask == 0])
    assert (after[mask == 1] != before[mask == 1]).any()

    st = sim.get_state()
    st["qpos"][:5] += rng.uniform(-0.3, 0.3, (5, n))
    sim.set_state(qpos=st["qpos"])
    sim.reset(mask=np.zeros(n, np.uint8))
    _check(sim, "reset(zeros) after set_state")
    assert (sim.point_cloud.numpy() != after).any()

    before, pose_before = sim.point_cloud.numpy(), sim.point_cloud_pose.numpy()
    variant = (np.arange(n) % 2).astype(np.int32)
    sim.set_look(variant=variant, rgb=rng.uniform(0, 1, (9, n)).astype(np.float32))
    _check(sim, "set_look")
    pose = sim.point_cloud_pose.numpy()
    np.testing.assert_array_equal(pose[:, :, variant == 0], pose_before[:, :, variant == 0])
    assert (pose[:2, :, variant == 1] != pose_before[:2, :, variant == 1]).any()      # front and top moved with the variant ...
    np.testing.assert_array_equal(pose[2], pose_before[2])                              # ... the wrist camera did not
    assert (sim.point_cloud.numpy() != before).any()
    _check_guards(sim, "after the entry points")
    sim.close()


def test_cloud_on_the_second_stream_is_the_serial_cloud(hip_lib, monkeypatch):
    """4.  The same seeded rollout with frames and cloud on the caller's stream (LCR_RENDER_OVERLAP=0) and on the second stream: identical bytes after every burst, across
    steps whose auto-resets redraw the looks (the cloud of a step must read the look and pose snapshots its frames were drawn from, not what later steps left)"""
    from gym_lowcostrobot_amd import VecSim
    from tests import look_ref

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=3, max_episode_steps=3, look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 7}, point_cloud=_spec(256, None, WITH_FLOOR, True))
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", n, **kw)
    acts = [(s_, s_.alloc_actions()) for s_ in (ref, ovl)]
    names = ("point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose")

    def same(when):
        for name in names:
            a, b = getattr(ref, name).numpy(), getattr(ovl, name).numpy()
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{name}, {when}")

    same("enabled")
    t, variants = 0, set()
    for burst in (1, 1, 1, 1, 3, 2, 4):          # episodes end every 3 steps: auto-resets fall at the start, in the middle and at the end of bursts
        for _ in range(burst):
            for s_, a in acts:
                s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
            t += 1
        same(f"after step {t - 1}")
        variants |= set(ovl.look()["variant"].tolist())
    assert len(variants) > 1
    _check(ovl, "second stream")
    for s_, a in acts:
        s_.free(a); s_.close()


def test_sharded_cloud_is_the_unsharded_cloud(hip_lib):
    """5.  Two shards of 64 envs on one GPU keep the cloud of the unsharded 128-env handle"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = _kw((16, 16), True, base_seed=9, max_episode_steps=3, point_cloud=_spec(64, None, WITH_FLOOR, True))
    one = VecSim("push", 128, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], **kw)
    assert all(s_.point_cloud.shape == (64, 64, 6) and s_.point_cloud_spec == one.point_cloud_spec for s_ in sh.shards)
    act = one.alloc_actions()
    for t in range(5):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        for name, axis in (("point_cloud", 0), ("point_cloud_count", 0), ("point_cloud_source", 0), ("point_cloud_pose", 2)):
            got = np.concatenate([getattr(s_, name).numpy() for s_ in sh.shards], axis=axis)
            np.testing.assert_array_equal(got.view(np.uint32), getattr(one, name).numpy().view(np.uint32), err_msg=f"{name}, step {t}")
    assert one.point_cloud.numpy().std() > 0.02
    one.free(act); one.close(); sh.close()


def test_nothing_else_moves(hip_lib):
    """6.  A twin handle without the cloud produces identical frames, planes, wrist frames, stack and state over ten steps"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=21, max_episode_steps=4, obs_stack=dict(frames=2, dtype="float16"))
    with_cloud = VecSim("stack", n, point_cloud=_spec(256, None, None, True), **kw)
    twin = VecSim("stack", n, **kw)
    assert twin.point_cloud is None and "point_cloud" not in twin.observations()
    names = ["image_" + c for c in ALL] + ["depth_" + c for c in ALL] + ["seg_" + c for c in ALL] + ["obs_stack"]
    acts = [(s_, s_.alloc_actions()) for s_ in (with_cloud, twin)]
    for t in range(10):
        for s_, a in acts:
            s_.fill_random_actions(a, 11, t); s_.step_device(a.ptr)
        for name in names:
            a, b = getattr(with_cloud, name).numpy(), getattr(twin, name).numpy()
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{name}, step {t}")
        sa, sb = with_cloud.get_state(), twin.get_state()
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{k}, step {t}")
        np.testing.assert_array_equal(with_cloud.outputs()["did_reset"], twin.outputs()["did_reset"])
    _check(with_cloud, "beside the stack")
    _check_guards(with_cloud, "beside the stack")
    for s_, a in acts:
        s_.free(a); s_.close()


def test_life_cycle(hip_lib):
    """7.  Refused without planes, with one plane, and with the wrist bit but no wrist camera; the same spec again is a no-op, another spec is refused; a handle without a
    cloud reports zeros; enabling on a live handle, before the stack, works"""
    from gym_lowcostrobot_amd import VecSim, _capi

    L = hip_lib
    n, size = 5, (16, 16)
    sp = _capi.PointCloudSpec.from_any(128)
    cv = _capi.LcrPointCloudView()
    for planes, what in (((), b"none is enabled"), (("depth",), b"segmentation plane is missing"), (("segmentation",), b"depth plane is missing")):
        sim = VecSim("push", n, observation_mode="both", image_size=size, image_planes=planes)
        assert L.lcr_enable_point_cloud(sim.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID
        assert what in L.lcr_last_error() and b"both image planes" in L.lcr_last_error(), L.lcr_last_error()
        assert L.lcr_get_point_cloud(sim.handle, ctypes.byref(cv)) == 0
        assert bytes(cv) == bytes(ctypes.sizeof(cv))   # all zeros
        assert sim.point_cloud is None and sim.point_cloud_spec is None
        sim.close()
    state = VecSim("push", n, observation_mode="state")
    assert L.lcr_enable_point_cloud(state.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID and b"no image observations" in L.lcr_last_error()
    state.close()

    plain = VecSim("push", n, **_kw(size, False))
    wr = _capi.PointCloudSpec.from_any(dict(points=128, cameras=("front", "wrist")))
    assert L.lcr_enable_point_cloud(plain.handle, ctypes.byref(wr)) == _capi.LCR_ERR_INVALID and b"wrist" in L.lcr_last_error()
    assert L.lcr_enable_point_cloud(plain.handle, ctypes.byref(sp)) == 0          # enabled late, on a live handle
    assert L.lcr_get_point_cloud(plain.handle, ctypes.byref(cv)) == 0
    assert cv.enabled == 1 and cv.spec.cameras == 3 and cv.spec.ids == 0x7FC and cv.spec.points == 128 and cv.spec.colors == 0
    assert (cv.channels, cv.slots, cv.image_height, cv.image_width) == (3, 2) + size and cv.bytes_per_env == 128 * 3 * 4
    assert cv.points and cv.count and cv.source and cv.camera_pose
    first = cv.points
    resolved = _capi.PointCloudSpec(points=128, cameras=3, ids=0x7FC, colors=0)
    for again in (sp, resolved):                                                    # the same spec, as given or resolved: a no-op
        assert L.lcr_enable_point_cloud(plain.handle, ctypes.byref(again)) == 0
        assert L.lcr_get_point_cloud(plain.handle, ctypes.byref(cv)) == 0 and cv.points == first
    for other in (dict(points=192), dict(points=128, colors=True), dict(points=128, cameras=("front",)), dict(points=128, ids=WITH_FLOOR)):
        o = _capi.PointCloudSpec.from_any(other)
        assert L.lcr_enable_point_cloud(plain.handle, ctypes.byref(o)) == _capi.LCR_ERR_INVALID and b"fixed for the life" in L.lcr_last_error()
    assert L.lcr_enable_obs_stack(plain.handle, ctypes.byref(_capi.ObsStackSpec.from_any(2))) == 0   # the stack may come after the cloud
    v = (_capi.LookVariant * 1)(_capi.LookVariant.from_any({}))
    assert L.lcr_enable_look(plain.handle, 1, v, None) == _capi.LCR_ERR_INVALID                       # look and wrist camera come before the planes, so before the cloud
    assert L.lcr_enable_wrist_camera(plain.handle, ctypes.byref(_capi.WristCamera.from_any(True))) == _capi.LCR_ERR_INVALID
    plain.step(np.zeros((n, plain.action_dim), np.float32))
    got = np.empty((n, 128, 3), np.float32)
    assert L.lcr_memcpy_d2h(plain.handle, got.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(cv.points), got.nbytes) == 0
    assert np.isfinite(got).all() and got.std() > 0.01
    plain.close()


def test_torch_view_of_the_cloud(hip_lib):
    """7.  sim.point_cloud.torch(): zero-copy (the same data pointer), float32, and it reads the finished cloud after lcr_get_point_cloud has joined the second stream"""
    import torch

    from gym_lowcostrobot_amd import VecSim, _capi

    n, size, P = 5, (16, 16), 64
    sim = VecSim("push", n, point_cloud=_spec(P, None, WITH_FLOOR, True), **_kw(size, False))
    t = sim.point_cloud.torch()
    assert t.dtype == torch.float32 and tuple(t.shape) == (n, P, 6) and t.is_contiguous() and t.data_ptr() == sim.point_cloud.ptr
    rng = np.random.default_rng(1)
    sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
    cv = _capi.LcrPointCloudView()
    assert hip_lib.lcr_get_point_cloud(sim.handle, ctypes.byref(cv)) == 0 and cv.points == sim.point_cloud.ptr   # joins: the handle's stream now waits for the cloud
    sim.sync()
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), sim.point_cloud.numpy().view(np.uint32))
    _check(sim, "after the step")
    assert sim.point_cloud_count.torch().dtype == torch.int32 and tuple(sim.point_cloud_source.torch().shape) == (n, P) and tuple(sim.point_cloud_pose.torch().shape) == (2, 13, n)
    del t
    sim.close()
