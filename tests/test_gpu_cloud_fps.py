"""The point cloud by farthest-point sampling on the GPU (VecSim(..., point_cloud=dict(points=P, sampling="fps", pool=Q)); lcr_enable_point_cloud_sampled): the greedy
order, bit for bit, against the numpy model of tests/cloud_fps_ref.py.

The twin method.  The pool never leaves the kernel, so handle A asks for P = Q: its output is the whole pool in greedy order, and every pool point is known to the bit.
Sorted by source (the pool is monotone in the candidate number) A's points are the pool in pool order; the model's greedy order of them must reproduce A's output -- sources
and point bits -- exactly.  Handle B, same seeds, asks for P < Q of the same pool: its output must be the first P of A's (the prefix property of the header).  What is exact
and what has a bound is as in tests/test_gpu_cloud.py: count, source and r g b exactly, x y z within cloud_ref.xyz_bound of the fp64 formula at their sources.

Shapes, the smallest at which the kernel can go wrong (a workgroup is one env; its 256 threads own the pool entries tid + 256 e; a wave is 64 entries; the kernel is built
for 2, 4, 8 and 16 entries a thread):
  reach  n 5   16 x 16    Q 128   P 64    front + top                  0 < M < Q (M = 61 .. 64 at reset): duplicates, zero distances, half the threads without an entry
  stack  n 70  36 x 52    Q 320   P 64    all three, + floor, colours  M > Q; Q ragged against 256; colours ride along
  push   n 64  64 x 64    Q 256   P 128   top + wrist, second cube     M = 0 everywhere: zeros and -1, the uniform skip of the loop
  reach  n 3   128 x 128  Q 4096  P 256   all three, + floor           the largest pool, 16 entries a thread
The other tests use Q = 1024 (4 entries a thread) and Q = 2048 (8), so that every build of the kernel runs.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import cloud_fps_ref, cloud_ref

pytestmark = pytest.mark.gpu

ALL = ("front", "top", "wrist")
WITH_FLOOR = ("arm", "cube", "cube2", "floor")
# task, n, size, cameras, ids, colours, Q, B's P, steps
ROLLOUTS = [
    ("reach", 5, (16, 16), ("front", "top"), None, False, 128, 64, 55),
    ("stack", 70, (36, 52), ALL, WITH_FLOOR, True, 320, 64, 55),
    ("push", 64, (64, 64), ("top", "wrist"), ("cube2",), False, 256, 128, 3),
    ("reach", 3, (128, 128), ALL, WITH_FLOOR, False, 4096, 256, 1),
]
ROLLOUT_IDS = [f"{r[0]}-n{r[1]}-{r[2][0]}x{r[2][1]}-Q{r[6]}-P{r[7]}" for r in ROLLOUTS]


def _cloud(P, Q, cams=None, ids=None, colors=False):
    d = dict(points=P, colors=colors, sampling="fps", pool=Q)
    if cams is not None:
        d["cameras"] = cams
    if ids is not None:
        d["ids"] = ids
    return d


def _kw(size, wrist, **more):
    return dict(observation_mode="both", image_size=size, image_planes=("depth", "segmentation"), wrist_camera=True if wrist else None, **more)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_twins(A, B, Q, when):
    """everything the header says of an FPS cloud, for the twins A (P = Q) and B (P < Q) -> count of A"""
    sp = A.point_cloud_spec
    assert sp["points"] == Q and A.point_cloud_sampling == B.point_cloud_sampling == {"mode": "fps", "pool": Q}
    PB = B.point_cloud_spec["points"]
    cams, colors = sp["cameras"], sp["colors"]
    H, W = A.image_size
    depth, seg = [getattr(A, "depth_" + c).numpy() for c in cams], [getattr(A, "seg_" + c).numpy() for c in cams]
    rgb = [getattr(A, "image_" + c).numpy() for c in cams]
    for c, d, s, f in zip(cams, depth, seg, rgb):   # a difference here is not this feature's
        np.testing.assert_array_equal(_bits(d), _bits(getattr(B, "depth_" + c).numpy()), err_msg=f"depth_{c} of the twins, {when}")
        np.testing.assert_array_equal(s, getattr(B, "seg_" + c).numpy(), err_msg=f"seg_{c} of the twins, {when}")
        np.testing.assert_array_equal(f, getattr(B, "image_" + c).numpy(), err_msg=f"image_{c} of the twins, {when}")
    pose = A.point_cloud_pose.numpy()
    np.testing.assert_array_equal(_bits(pose), _bits(B.point_cloud_pose.numpy()), err_msg=f"camera_pose of the twins, {when}")
    pts, cnt, src = A.point_cloud.numpy(), A.point_cloud_count.numpy(), A.point_cloud_source.numpy()
    C = 6 if colors else 3
    assert pts.dtype == np.float32 and pts.shape == (A.n, Q, C) and src.shape == (A.n, Q) and pose.shape == (len(cams), 13, A.n)

    # count and the pool: exact integer decisions on the GPU's own segmentation bytes
    cand = cloud_ref.candidates(seg, cloud_ref.ids_mask(sp["ids"]))
    M = cand.sum(axis=1)
    np.testing.assert_array_equal(cnt, M, err_msg=f"count, {when}")
    np.testing.assert_array_equal(B.point_cloud_count.numpy(), M, err_msg=f"count of B, {when}")
    pool_src = np.stack([cloud_fps_ref.pool_sources(cand[e], Q) for e in range(A.n)])
    by_source = np.argsort(src, axis=1, kind="stable")
    env = np.arange(A.n)[:, None]
    np.testing.assert_array_equal(src[env, by_source], pool_src, err_msg=f"A's sources as a multiset, {when}")

    # the greedy order of the pool A has shown, by the model: sources and point bits exactly
    live = M > 0
    assert not pts[~live].any() and (src[~live] == -1).all()
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

    # the points themselves: the fp64 formula at their sources
    want = cloud_fps_ref.points_at(depth, rgb, pose, src.astype(np.int64), H, W, colors)
    if colors:
        bad = np.argwhere(_bits(pts[..., 3:]) != _bits(want[..., 3:].astype(np.float32)))
        assert bad.size == 0, (when, "rgb", len(bad), bad[:6].tolist())
    bound = cloud_ref.xyz_bound(depth, pose, src.astype(np.int64), H, W)[..., None]
    err = np.abs(pts[..., :3].astype(np.float64) - want[..., :3])
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (when, "xyz", len(bad), bad[:6].tolist(), float((err / bound).max()))
    return cnt


@functools.lru_cache(maxsize=None)
def _rollout(case):
    from gym_lowcostrobot_amd import VecSim
    from tests.test_gpu_cloud import _check_guards, _scene_camera_f32, _wrist_pose_distance

    task, n, size, cams, ids, colors, Q, PB, steps = case
    wrist = "wrist" in cams
    A = VecSim(task, n, base_seed=17, point_cloud=_cloud(Q, Q, cams, ids, colors), **_kw(size, wrist))
    B = VecSim(task, n, base_seed=17, point_cloud=_cloud(PB, Q, cams, ids, colors), **_kw(size, wrist))
    assert A.point_cloud_spec == {"points": Q, "cameras": cams, "ids": tuple(i for i in range(11) if cloud_ref.ids_mask(ids) >> i & 1), "colors": colors}
    acts = [(s_, s_.alloc_actions()) for s_ in (A, B)]
    stats = {"gt": 0, "lt": 0, "zero": 0, "resets": 0, "wrist": 0.0}
    fixed = {c: _scene_camera_f32(task, c, size[0]) for c in cams if c != "wrist"}
    for t in range(-1, steps):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 23, t); s_.step_device(a.ptr)
            stats["resets"] += int(A.outputs()["did_reset"].sum())
        cnt = _check_twins(A, B, Q, f"step {t}")
        stats["gt"] += int((cnt > Q).sum()); stats["lt"] += int(((cnt > 0) & (cnt < Q)).sum()); stats["zero"] += int((cnt == 0).sum())
        pose = A.point_cloud_pose.numpy()
        for i, c in enumerate(cams):
            if c == "wrist":
                stats["wrist"] = max(stats["wrist"], _wrist_pose_distance(A, pose[i]))
            else:
                bad = np.argwhere(_bits(pose[i]) != _bits(fixed[c])[:, None])
                assert bad.size == 0, (c, t, bad[:6].tolist())
    for s_ in (A, B):
        _check_guards(s_, "after the rollout")
    np.testing.assert_array_equal(A.observations()["point_cloud"], A.point_cloud.numpy())
    for s_, a in acts:
        s_.free(a); s_.close()
    print(f"fps rollout {case[0]} n {n} Q {Q}: {stats}, model fallbacks so far {cloud_fps_ref.FALLBACKS[0]}")
    return stats


@pytest.mark.parametrize("case", ROLLOUTS, ids=ROLLOUT_IDS)
def test_greedy_order_bit_for_bit(hip_lib, case):
    """Random actions; after enabling and after every step the twins are held to the header: the pool, the greedy order and B as A's prefix bit for bit, the points within
    their bound, the poses as in the strided cloud's test, the guards intact at the end"""
    from tests.test_gpu_cloud import WRIST_POSE_BOUND

    task, n, size, cams, ids, colors, Q, PB, steps = case
    st = _rollout(case)
    checks = n * (steps + 1)
    if steps >= 55:
        assert st["resets"] >= n, st          # 55 steps cross an auto-reset of every env
    if (task, Q) == ("reach", 128):
        assert st["lt"] > 0, st
    if task == "stack":
        assert st["gt"] == checks, st
    if task == "push":
        assert st["zero"] == checks, st
    if Q == 4096:
        assert st["gt"] == checks, st
    assert st["wrist"] <= WRIST_POSE_BOUND, st


def test_the_rollouts_cover_every_regime(hip_lib):
    """together the cases contain env-steps with M > Q, with 0 < M < Q and with M = 0 (rollouts already run are not run again)"""
    tot = {k: sum(_rollout(c)[k] for c in ROLLOUTS) for k in ("gt", "lt", "zero")}
    assert tot["gt"] > 0 and tot["lt"] > 0 and tot["zero"] > 0, tot


def test_the_entry_points_that_are_not_the_step(hip_lib):
    """After reset(), a masked reset, set_state followed by the all-zero-mask reset, and set_look on a handle with look variants the cloud is the header's function of the
    current frames: the twins at 96 x 96 with two cameras, Q = 1024 (four entries a thread)"""
    from gym_lowcostrobot_amd import VecSim

    n, size, Q, PB = 6, (96, 96), 1024, 128
    variants = [{}, {"cam_dpos": [[0.03, 0.0, 0.02], [0.0, 0.04, 0.05]], "fovy_deg": [50.0, 40.0]}]
    kw = _kw(size, False, base_seed=2, look_variants=variants)
    twins = [VecSim("push", n, point_cloud=_cloud(P, Q, ("front", "top"), ("arm", "cube", "floor"), True), **kw) for P in (Q, PB)]
    A, B = twins
    rng = np.random.default_rng(4)
    _check_twins(A, B, Q, "enabled")
    for t in range(2):
        a = rng.uniform(-1, 1, (n, A.action_dim)).astype(np.float32)
        for s_ in twins:
            s_.step(a)
    cnt = _check_twins(A, B, Q, "steps")
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
        s_.close()


def test_fps_cloud_on_the_second_stream_is_the_serial_cloud(hip_lib, monkeypatch):
    """The same seeded rollout of ten steps with frames and cloud on the caller's stream (LCR_RENDER_OVERLAP=0) and on the second stream: identical points, sources and
    counts, across auto-resets that redraw the looks.  Q = 2048: eight entries a thread"""
    from gym_lowcostrobot_amd import VecSim
    from tests import look_ref

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=3, max_episode_steps=3, look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 7}, point_cloud=_cloud(256, 2048, None, WITH_FLOOR, True))
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
    src = ovl.point_cloud_source.numpy()
    assert (ovl.point_cloud_count.numpy() > 2048).all() and all(len(set(r.tolist())) == 256 for r in src)   # distinct candidates: a real FPS ran
    for s_, a in acts:
        s_.free(a); s_.close()


def test_sharded_fps_cloud_is_the_unsharded_cloud(hip_lib):
    """Two shards of 64 envs (the cut falls on a wave boundary of the step kernels) keep the cloud of the unsharded 128-env handle, bit for bit"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = _kw((16, 16), True, base_seed=9, max_episode_steps=3, point_cloud=_cloud(64, 192, None, WITH_FLOOR, True))
    one = VecSim("push", 128, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], **kw)
    assert all(s_.point_cloud.shape == (64, 64, 6) and s_.point_cloud_spec == one.point_cloud_spec and s_.point_cloud_sampling == {"mode": "fps", "pool": 192} for s_ in sh.shards)
    act = one.alloc_actions()
    for t in range(5):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        for name, axis in (("point_cloud", 0), ("point_cloud_count", 0), ("point_cloud_source", 0), ("point_cloud_pose", 2)):
            got = np.concatenate([getattr(s_, name).numpy() for s_ in sh.shards], axis=axis)
            np.testing.assert_array_equal(_bits(got), _bits(getattr(one, name).numpy()), err_msg=f"{name}, step {t}")
    assert one.point_cloud.numpy().std() > 0.02
    one.free(act); one.close(); sh.close()


def test_life_cycle(hip_lib):
    """The same spec and sampling again is a no-op; another pool, another mode or plain lcr_enable_point_cloud on an FPS handle is refused and the message names both; an FPS
    enable on a strided handle is refused; without planes or images the refusals are those of the strided cloud"""
    from gym_lowcostrobot_amd import VecSim, _capi

    L = hip_lib
    n, size = 5, (16, 16)
    sp = _capi.PointCloudSpec.from_any(64)
    fps = _capi.PointCloudSampling(mode=1, pool=128)
    got = _capi.PointCloudSampling(mode=7, pool=7)
    for planes, what in (((), b"none is enabled"), (("depth",), b"segmentation plane is missing"), (("segmentation",), b"depth plane is missing")):
        sim = VecSim("push", n, observation_mode="both", image_size=size, image_planes=planes)
        assert L.lcr_enable_point_cloud_sampled(sim.handle, ctypes.byref(sp), ctypes.byref(fps)) == _capi.LCR_ERR_INVALID
        assert what in L.lcr_last_error() and b"both image planes" in L.lcr_last_error(), L.lcr_last_error()
        assert L.lcr_get_point_cloud_sampling(sim.handle, ctypes.byref(got)) == 0 and (got.mode, got.pool) == (0, 0)
        assert sim.point_cloud is None and sim.point_cloud_sampling is None
        sim.close()
    state = VecSim("push", n, observation_mode="state")
    assert L.lcr_enable_point_cloud_sampled(state.handle, ctypes.byref(sp), ctypes.byref(fps)) == _capi.LCR_ERR_INVALID and b"no image observations" in L.lcr_last_error()
    state.close()

    sim = VecSim("push", n, **_kw(size, False))
    assert L.lcr_enable_point_cloud_sampled(sim.handle, ctypes.byref(sp), ctypes.byref(fps)) == 0   # enabled late, on a live handle
    assert L.lcr_get_point_cloud_sampling(sim.handle, ctypes.byref(got)) == 0 and (got.mode, got.pool) == (1, 128)
    cv = _capi.LcrPointCloudView()
    assert L.lcr_get_point_cloud(sim.handle, ctypes.byref(cv)) == 0 and cv.enabled == 1 and cv.spec.points == 64 and cv.bytes_per_env == 64 * 3 * 4
    first = cv.points
    assert L.lcr_enable_point_cloud_sampled(sim.handle, ctypes.byref(sp), ctypes.byref(fps)) == 0   # the same again: nothing happens
    assert L.lcr_get_point_cloud(sim.handle, ctypes.byref(cv)) == 0 and cv.points == first
    for other_spec, other in ((sp, _capi.PointCloudSampling(mode=1, pool=192)), (sp, _capi.PointCloudSampling(mode=0, pool=0)), (sp, None),
                              (_capi.PointCloudSpec.from_any(128), fps)):
        assert L.lcr_enable_point_cloud_sampled(sim.handle, ctypes.byref(other_spec), ctypes.byref(other) if other is not None else None) == _capi.LCR_ERR_INVALID
        msg = L.lcr_last_error()
        assert b"fixed for the life" in msg and b"sampling fps, pool 128" in msg, msg   # what is enabled ...
        want = b"sampling stride, pool 0" if other is None or other.mode == 0 else b"sampling fps, pool %d" % other.pool
        assert msg.count(b"sampling") == 2 and want in msg.split(b"asked for")[1] and b"points %d" % other_spec.points in msg.split(b"asked for")[1], msg   # ... and what was asked for
    assert L.lcr_enable_point_cloud(sim.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID and b"sampling fps, pool 128" in L.lcr_last_error()
    sim.step(np.zeros((n, sim.action_dim), np.float32))
    out = np.empty((n, 64, 3), np.float32)
    assert L.lcr_memcpy_d2h(sim.handle, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(cv.points), out.nbytes) == 0
    assert np.isfinite(out).all() and out.std() > 0.01
    sim.close()

    strided = VecSim("push", n, point_cloud=64, **_kw(size, False))
    assert strided.point_cloud_sampling == {"mode": "stride", "pool": 0}
    assert L.lcr_enable_point_cloud_sampled(strided.handle, ctypes.byref(sp), ctypes.byref(fps)) == _capi.LCR_ERR_INVALID
    msg = L.lcr_last_error()
    assert b"fixed for the life" in msg and b"sampling stride, pool 0" in msg and b"sampling fps, pool 128" in msg, msg
    assert L.lcr_enable_point_cloud_sampled(strided.handle, ctypes.byref(sp), None) == 0                                            # the same strided cloud again, either way
    assert L.lcr_enable_point_cloud_sampled(strided.handle, ctypes.byref(sp), ctypes.byref(_capi.PointCloudSampling(mode=0, pool=0))) == 0
    strided.close()


def test_stride_is_untouched(hip_lib):
    """sampling="stride" and the keyword form without a sampling give byte-equal clouds over five steps, and the same spec"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 70, (36, 52)
    kw = _kw(size, True, base_seed=21, max_episode_steps=4)
    spec = dict(points=256, ids=WITH_FLOOR, colors=True)
    named = VecSim("stack", n, point_cloud=dict(spec, sampling="stride"), **kw)
    plain = VecSim("stack", n, point_cloud=spec, **kw)
    assert named.point_cloud_spec == plain.point_cloud_spec and sorted(plain.point_cloud_spec) == ["cameras", "colors", "ids", "points"]
    assert named.point_cloud_sampling == plain.point_cloud_sampling == {"mode": "stride", "pool": 0}
    acts = [(s_, s_.alloc_actions()) for s_ in (named, plain)]
    for t in range(-1, 5):
        if t >= 0:
            for s_, a in acts:
                s_.fill_random_actions(a, 11, t); s_.step_device(a.ptr)
        for name in ("point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose"):
            np.testing.assert_array_equal(_bits(getattr(named, name).numpy()), _bits(getattr(plain, name).numpy()), err_msg=f"{name}, step {t}")
    from tests.test_gpu_cloud import _check

    _check(named, "sampling='stride'")   # and it is the strided cloud of the model
    for s_, a in acts:
        s_.free(a); s_.close()
