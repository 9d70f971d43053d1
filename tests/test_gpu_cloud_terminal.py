"""The point cloud of the terminal observation on the GPU (VecSim.point_cloud_terminal; lcr_point_cloud_terminal), and the vector adapters that expose stack and cloud.

Strided mode: the terminal cloud against the numpy model of tests/cloud_ref.py, fed the terminal planes, frames and wrist frames of the existing terminal calls for the
same envs and the pose the call returns.  The rule is that of tests/test_gpu_cloud.py::_check and no tolerance is new: count and source exact, r g b bit for bit, x y z
within cloud_ref.xyz_bound; the wrist pose within test_gpu_cloud.WRIST_POSE_BOUND of tests/wrist_ref.py on the terminal joint angles.

Farthest-point and cropped modes: bit for bit against the ordinary path.  A twin handle of the same configuration is put into the terminal poses (set_state, then the
no-op reset); the terminal qpos is float32 and converts to double exactly.  Its live cloud, count, source and pose of those envs must equal the terminal ones.

Shapes: 70 envs (a ragged last wave of the step kernel), 16 x 16 and 32 x 36 frames, episode ends staggered with set_state(elapsed = 49 - e % 7)."""
import numpy as np
import pytest

from tests import cloud_ref
from tests.test_gpu_cloud import WRIST_POSE_BOUND

pytestmark = pytest.mark.gpu

N = 70
ALL = ("front", "top", "wrist")
WITH_FLOOR = ("arm", "cube", "cube2", "floor")
SMALL, TAIL = (16, 16), (32, 36)


def _kw(size, wrist, look=False, **more):
    from tests import look_ref

    kw = dict(observation_mode="both", image_size=size, image_planes=("depth", "segmentation"), wrist_camera=True if wrist else None, base_seed=17, **more)
    if look:
        kw.update(look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 9, "cube": ([0.2, 0, 0], [1, 0.4, 0.4])})
    return kw


def _stagger(sim):
    sim.set_state(elapsed=(49 - np.arange(sim.n) % 7).astype(np.int32))


def _terminal_inputs(sim, ids, cams):
    """depth, seg, rgb per camera slot of the listed envs' terminal observations, by the existing terminal calls"""
    front, top = sim.render_terminal(ids)
    pl = sim.render_terminal_planes(ids)
    rgb, depth, seg = {"front": front, "top": top}, {"front": pl["depth_front"], "top": pl["depth_top"]}, {"front": pl["segmentation_front"], "top": pl["segmentation_top"]}
    if "wrist" in cams:
        w = sim.render_terminal_wrist(ids)
        rgb["wrist"], depth["wrist"], seg["wrist"] = w["image_wrist"], w["depth_wrist"], w["segmentation_wrist"]
    return [depth[c] for c in cams], [seg[c] for c in cams], [rgb[c] for c in cams]


def _check(sim, ids, got, when):
    """the rule of tests/test_gpu_cloud.py::_check on the terminal inputs -> (count, largest error / bound)"""
    sp = sim.point_cloud_spec
    H, W = sim.image_size
    depth, seg, rgb = _terminal_inputs(sim, ids, sp["cameras"])
    pts, cnt, src, pose = got["point_cloud"], got["count"], got["source"], got["pose"]
    assert pts.dtype == np.float32 and pts.shape == (ids.size, sp["points"], 6 if sp["colors"] else 3) and pose.shape == (len(sp["cameras"]), 13, ids.size)
    assert cnt.dtype == np.int32 and src.dtype == np.int32 and src.shape == (ids.size, sp["points"])
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


def _wrist_pose_distance(sim, ids, pose_wrist):
    """largest component difference between the returned wrist pose (13, len(ids)) and tests/wrist_ref.py's fp64 pose of the TERMINAL joint angles"""
    from tests import wrist_ref

    w = sim.wrist_camera
    m = wrist_ref.mount(w["link"], w["pos"], w["xyaxes"], w["fovy_deg"])
    q = sim.terminal_obs.numpy()[:6].astype(np.float64)
    s = float(np.float32(2.0 * np.tan(np.radians(m["fovy_deg"]) / 2) / sim.image_size[0]))
    worst = 0.0
    for i, e in enumerate(ids):
        ref = np.concatenate(list(wrist_ref.camera(m, q[:, e])) + [[s]])
        worst = max(worst, float(np.abs(pose_wrist[:, i].astype(np.float64) - ref).max()))
    return worst


# task, size, P, cameras, ids, colours, looks
STRIDED = [
    ("reach", SMALL, 128, ("front", "top"), None, False, False),          # 2 x 16 groups; 0 < M < P
    ("stack", TAIL, 256, ALL, WITH_FLOOR, True, False),                   # the wrist camera, colours, M > P
    ("push", TAIL, 128, ("front", "top"), ("arm", "cube"), True, True),   # looks: the terminal look's cameras and colours
    ("reach", SMALL, 64, ("top", "wrist"), None, False, False),           # the wrist camera without colours
]


@pytest.mark.parametrize("task,size,P,cams,ids_,colors,look", STRIDED, ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-P{c[2]}-{'+'.join(c[3])}{'-rgb' if c[5] else ''}{'-look' if c[6] else ''}" for c in STRIDED])
def test_strided_terminal_cloud_against_the_model(hip_lib, task, size, P, cams, ids_, colors, look):
    """6.  Seven staggered steps: every env ends an episode, on seven different steps.  The terminal clouds of each step's reset envs are held to the model on the terminal
    planes and frames; the live cloud is not touched by the call"""
    from gym_lowcostrobot_amd import VecSim

    spec = dict(points=P, cameras=cams, colors=colors, terminal=True)
    if ids_ is not None:
        spec["ids"] = ids_
    sim = VecSim(task, N, point_cloud=spec, **_kw(size, "wrist" in cams, look))
    assert sim.point_cloud_wants_terminal and "terminal" not in sim.point_cloud_spec
    act = sim.alloc_actions()
    _stagger(sim)
    total, lt, gt, worst_wrist, ratio = 0, 0, 0, 0.0, 0.0
    ended = np.zeros(N, bool)
    for t in range(7):
        sim.fill_random_actions(act, 23, t); sim.step_device(act.ptr)
        ids = np.nonzero(sim.outputs()["did_reset"])[0].astype(np.int32)
        assert ids.size   # (the envs whose time runs out on this step, and any whose episode ended otherwise)
        ended[ids] = True
        live = [getattr(sim, n_).numpy() for n_ in ("point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose")]
        got = sim.point_cloud_terminal(ids)
        cnt, r = _check(sim, ids, got, f"step {t}")
        for n_, a in zip(("point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose"), live):
            np.testing.assert_array_equal(getattr(sim, n_).numpy().view(np.uint32), a.view(np.uint32), err_msg=f"live {n_}, step {t}")
        # the terminal cloud is not the live (reset-state) cloud of those envs
        assert (got["point_cloud"].view(np.uint32) != live[0][ids].view(np.uint32)).any() or not cnt.any()
        total += ids.size; lt += int(((cnt > 0) & (cnt < P)).sum()); gt += int((cnt > P).sum()); ratio = max(ratio, r)
        if "wrist" in cams:
            worst_wrist = max(worst_wrist, _wrist_pose_distance(sim, ids, got["pose"][cams.index("wrist")]))
    print(f"terminal cloud {task} {size} P{P}: {total} clouds, 0 < M < P {lt}, M > P {gt}, largest error / bound {ratio:.3g}, wrist pose distance {worst_wrist:.3g}")
    assert ended.all() and worst_wrist <= WRIST_POSE_BOUND, (total, worst_wrist)
    if (task, P) == ("reach", 128):
        assert lt > 0
    if task == "stack":
        assert gt == total
    sim.free(act); sim.close()


def _terminal_pose(sim):
    """the terminal poses as the library gathers them: qpos (nq, N) and target (3, N), float32 values in float64 / float32 arrays"""
    t, tq = sim.terminal_obs.numpy(), sim.terminal_quat.numpy()
    q = np.zeros((sim.nq, sim.n), np.float64)
    q[0:6], q[6:9], q[9:13] = t[0:6], t[12:15], tq[0:4]
    if sim.task_name == "stack":
        q[13:16], q[16:20] = t[15:18], tq[4:8]
    target = t[15:18].astype(np.float32) if sim.task_name in ("push", "pick_place") else np.zeros((3, sim.n), np.float32)
    return q, target


MODES = [
    ("fps", "stack", TAIL, dict(points=64, sampling="fps", pool=128, cameras=ALL, ids=WITH_FLOOR, colors=True)),
    ("crop", "push", TAIL, dict(points=128, cameras=ALL, ids=WITH_FLOOR, colors=True, crop=((-0.25, -0.05, -0.01), (0.25, 0.45, 0.3)))),
    ("crop-fps", "reach", SMALL, dict(points=64, sampling="fps", pool=64, cameras=("front", "top"), crop=((-0.3, None, 0.0), (0.3, 0.5, None)))),
]


@pytest.mark.parametrize("name,task,size,spec", MODES, ids=[m[0] for m in MODES])
def test_fps_and_crop_terminal_clouds_are_the_twins_live_clouds(hip_lib, name, task, size, spec):
    """7.  Bit for bit against the ordinary path: the twin's live cloud in the terminal poses"""
    from gym_lowcostrobot_amd import VecSim

    wrist = "wrist" in spec["cameras"]
    sim = VecSim(task, N, point_cloud=dict(spec, terminal=True), **_kw(size, wrist))
    twin = VecSim(task, N, point_cloud=spec, **_kw(size, wrist))
    assert sim.point_cloud_sampling == twin.point_cloud_sampling and sim.point_cloud_crop == twin.point_cloud_crop and sim.point_cloud_spec == twin.point_cloud_spec
    act = sim.alloc_actions()
    _stagger(sim)
    total = nonempty = 0
    for t in range(4):
        sim.fill_random_actions(act, 29, t); sim.step_device(act.ptr)
        ids = np.nonzero(sim.outputs()["did_reset"])[0].astype(np.int32)
        got = sim.point_cloud_terminal(ids)
        q, target = _terminal_pose(sim)
        st = twin.get_state()
        st["qpos"][:, ids] = q[:, ids]
        st["target"][:, ids] = target[:, ids]
        twin.set_state(qpos=st["qpos"], target=st["target"])
        twin.reset(mask=np.zeros(N, np.uint8))
        for key, arr, axis in (("point_cloud", twin.point_cloud, 0), ("count", twin.point_cloud_count, 0), ("source", twin.point_cloud_source, 0), ("pose", twin.point_cloud_pose, 2)):
            want = np.take(arr.numpy(), ids, axis=axis)
            bad = np.argwhere(got[key].view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (name, key, t, len(bad), bad[:6].tolist())
        total += ids.size; nonempty += int((got["count"] > 0).sum())
    assert total >= 30 and nonempty > 0, (total, nonempty)
    sim.free(act); sim.close(); twin.close()


def test_second_stream_gives_the_serial_terminal_clouds(hip_lib, monkeypatch):
    """3.  The same rollout with LCR_RENDER_OVERLAP=0 and on the second stream, steps in bursts: the same terminal clouds"""
    from gym_lowcostrobot_amd import VecSim

    kw = _kw(TAIL, True, True, max_episode_steps=3)
    spec = dict(points=128, ids=WITH_FLOOR, colors=True, terminal=True)
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", N, point_cloud=spec, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", N, point_cloud=spec, **kw)
    acts = [(s, s.alloc_actions()) for s in (ref, ovl)]
    t = total = 0
    for burst in (1, 2, 3, 1, 2):
        for _ in range(burst):
            for s, a in acts:
                s.fill_random_actions(a, 5, t); s.step_device(a.ptr)
            t += 1
        ids = np.nonzero(ref.outputs()["did_reset"])[0].astype(np.int32)
        if ids.size:
            a, b = ref.point_cloud_terminal(ids), ovl.point_cloud_terminal(ids)
            for k in a:
                np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=f"{k}, step {t - 1}")
            total += ids.size
    assert total >= N
    for s, a in acts:
        s.free(a); s.close()


def test_calling_the_terminal_cloud_changes_no_later_byte(hip_lib):
    """4.  A handle whose terminal clouds are fetched after every step and one where they never are: identical live cloud, frames, planes, outputs and state"""
    from gym_lowcostrobot_amd import VecSim

    kw = _kw(TAIL, True, True, max_episode_steps=3)
    spec = dict(points=128, colors=True)
    called, quiet = VecSim("push", N, point_cloud=dict(spec, terminal=True), **kw), VecSim("push", N, point_cloud=spec, **kw)
    assert quiet.point_cloud_wants_terminal is False
    acts = [(s, s.alloc_actions()) for s in (called, quiet)]
    names = ["point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose"] + [p + c for p in ("image_", "depth_", "seg_") for c in ALL]
    for t in range(7):
        for s, a in acts:
            s.fill_random_actions(a, 11, t); s.step_device(a.ptr)
        ids = np.nonzero(called.outputs()["did_reset"])[0].astype(np.int32)
        if ids.size:
            called.point_cloud_terminal(ids)
            quiet_got = quiet.point_cloud_terminal(ids) if t == 5 else None   # (the declaration is not needed: any handle with a cloud answers)
            assert quiet_got is None or quiet_got["point_cloud"].shape == (ids.size, 128, 6)
        for n_ in names:
            a, b = getattr(called, n_).numpy(), getattr(quiet, n_).numpy()
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{n_}, step {t}")
        sa, sb = called.get_state(), quiet.get_state()
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{k}, step {t}")
        np.testing.assert_array_equal(called.outputs()["reward"], quiet.outputs()["reward"])
    for s, a in acts:
        s.free(a); s.close()


def test_refusals(hip_lib):
    """8.  An env the last step did not reset, an id out of range, a handle without a cloud; count = 0 and NULL outputs are allowed"""
    import ctypes

    from gym_lowcostrobot_amd import VecSim, _capi

    sim = VecSim("reach", N, point_cloud=dict(points=64, terminal=True), **_kw(SMALL, False))
    _stagger(sim)
    sim.step(np.zeros((N, sim.action_dim), np.float32))
    dres = sim.outputs()["did_reset"]
    done, alive = np.nonzero(dres)[0].astype(np.int32), np.nonzero(~dres)[0]
    assert done.size and alive.size
    full = sim.point_cloud_terminal(done)
    with pytest.raises(ValueError, match="did_reset"):
        sim.point_cloud_terminal([done[0], alive[0]])
    for bad in ([N], [-1]):
        with pytest.raises(ValueError, match="out of range"):
            sim.point_cloud_terminal(bad)
    empty = sim.point_cloud_terminal([])
    assert empty["point_cloud"].shape == (0, 64, 3) and empty["pose"].shape == (2, 13, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert hip_lib.lcr_point_cloud_terminal(sim.handle, None, 0, None, None, None, None) == 0
    assert hip_lib.lcr_point_cloud_terminal(sim.handle, None, 1, None, None, None, None) == _capi.LCR_ERR_INVALID
    assert hip_lib.lcr_point_cloud_terminal(sim.handle, vp(done), int(done.size), None, None, None, None) == 0   # every output may be NULL
    cnt = np.full(done.size, -7, np.int32)
    assert hip_lib.lcr_point_cloud_terminal(sim.handle, vp(done), int(done.size), None, vp(cnt), None, None) == 0
    np.testing.assert_array_equal(cnt, full["count"])
    sim.close()
    none = VecSim("reach", 5, **_kw(SMALL, False))
    ids = np.zeros(1, np.int32)
    assert hip_lib.lcr_point_cloud_terminal(none.handle, vp(ids), 1, None, None, None, None) == _capi.LCR_ERR_INVALID and b"no point cloud" in hip_lib.lcr_last_error()
    with pytest.raises(ValueError, match="no point_cloud"):
        none.point_cloud_terminal([0])
    none.close()


def test_sharded_terminal_clouds_are_the_unsharded_ones(hip_lib):
    """10.  Two shards of 64 envs on one GPU return the terminal clouds of the unsharded 128-env handle, by global env id"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = _kw(SMALL, True, max_episode_steps=3)
    spec = dict(points=64, ids=WITH_FLOOR, colors=True, terminal=True)
    one = VecSim("push", 128, point_cloud=spec, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], point_cloud=spec, **kw)
    act = one.alloc_actions()
    total = 0
    for t in range(4):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        ids = np.nonzero(one.outputs()["did_reset"])[0][::-1].copy()
        if ids.size:
            a, b = one.point_cloud_terminal(ids), sh.point_cloud_terminal(ids)
            for k in a:
                np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=f"{k}, step {t}")
            total += ids.size
    assert total >= 128
    one.free(act); one.close(); sh.close()


# ---- the vector adapters ----

def _adapter_kw():
    kw = dict(obs_stack=dict(frames=4, dtype="float16", reset_fill="zero", terminal=True), point_cloud=dict(points=64, colors=True, terminal=True),
              **_kw(SMALL, True, True, max_episode_steps=3))
    del kw["base_seed"]   # (the adapters pass their `seed`)
    return kw


def _twin_terminals(twin, actions):
    twin.step(actions)
    ids = np.nonzero(twin.outputs()["did_reset"])[0].astype(np.int32)
    if not ids.size:
        return ids, None, None
    return ids, twin.obs_stack_terminal(ids), twin.point_cloud_terminal(ids)["point_cloud"]


def test_the_sb3_adapter_carries_stack_and_cloud(hip_lib):
    """9.  LowCostRobotVecEnv: observation_space gains obs_stack and point_cloud; the live observations are sim.obs_stack / sim.point_cloud; every terminal_observation has
    exactly the keys of observation_space and carries the terminal stack and cloud of a twin VecSim's terminal calls"""
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, VecSim

    n, kw = 6, _adapter_kw()
    env = LowCostRobotVecEnv("push", n, seed=4, **kw)
    twin = VecSim("push", n, base_seed=4, **{k: v for k, v in kw.items() if k != "base_seed"})
    sp = env.observation_space.spaces if hasattr(env.observation_space, "spaces") else env.observation_space
    assert sp["obs_stack"].shape == (4, 9) + SMALL and sp["obs_stack"].dtype == np.float16 and sp["point_cloud"].shape == (64, 6) and sp["point_cloud"].dtype == np.float32
    assert "count" not in sp and "source" not in sp and "pose" not in sp and "image_stack" not in sp
    obs = env.reset(); twin.reset()
    rng = np.random.default_rng(0)
    finished = 0
    for t in range(7):
        a = rng.uniform(-1, 1, (n, env.sim.action_dim)).astype(np.float32)
        obs, rew, dones, infos = env.step(a)
        ids, tstack, tcloud = _twin_terminals(twin, a)
        assert set(obs) == set(sp)
        np.testing.assert_array_equal(obs["obs_stack"].view(np.uint16), env.sim.obs_stack.numpy().view(np.uint16))
        np.testing.assert_array_equal(obs["point_cloud"].view(np.uint32), env.sim.point_cloud.numpy().view(np.uint32))
        np.testing.assert_array_equal(obs["obs_stack"].view(np.uint16), twin.obs_stack.numpy().view(np.uint16))
        np.testing.assert_array_equal(np.nonzero(dones)[0], ids)
        for j, i in enumerate(ids):
            tob = infos[i]["terminal_observation"]
            assert list(tob) == list(sp)
            np.testing.assert_array_equal(tob["obs_stack"].view(np.uint16), tstack[j].view(np.uint16), err_msg=f"step {t}, env {i}")
            np.testing.assert_array_equal(tob["point_cloud"].view(np.uint32), tcloud[j].view(np.uint32), err_msg=f"step {t}, env {i}")
            assert sp["obs_stack"].contains(tob["obs_stack"]) and tob["point_cloud"].shape == (64, 6)
            finished += 1
    assert finished >= 2 * n
    env.close(); twin.close()


def test_the_gymnasium_adapter_carries_stack_and_cloud(hip_lib):
    """9.  LowCostRobotVectorEnv: final_obs has exactly the keys of the observation space, and its rows of the reset envs are the twin's terminal stacks and clouds"""
    from gym_lowcostrobot_amd import LowCostRobotVectorEnv, VecSim

    n, kw = 6, _adapter_kw()
    env = LowCostRobotVectorEnv("push", n, seed=4, **kw)
    twin = VecSim("push", n, base_seed=4, **{k: v for k, v in kw.items() if k != "base_seed"})
    sp = env.single_observation_space.spaces if hasattr(env.single_observation_space, "spaces") else env.single_observation_space
    assert "obs_stack" in sp and "point_cloud" in sp
    obs, _ = env.reset(); twin.reset()
    rng = np.random.default_rng(0)
    finished = 0
    for t in range(7):
        a = rng.uniform(-1, 1, (n, env._v.sim.action_dim)).astype(np.float32)
        obs, rew, term, trunc, infos = env.step(a)
        ids, tstack, tcloud = _twin_terminals(twin, a)
        np.testing.assert_array_equal(obs["obs_stack"].view(np.uint16), twin.obs_stack.numpy().view(np.uint16))
        np.testing.assert_array_equal(obs["point_cloud"].view(np.uint32), twin.point_cloud.numpy().view(np.uint32))
        if ids.size:
            fin = infos["final_obs"]
            assert list(fin) == list(sp)
            np.testing.assert_array_equal(np.nonzero(infos["_final_obs"])[0], ids)
            np.testing.assert_array_equal(fin["obs_stack"][ids].view(np.uint16), tstack.view(np.uint16), err_msg=f"step {t}")
            np.testing.assert_array_equal(fin["point_cloud"][ids].view(np.uint32), tcloud.view(np.uint32), err_msg=f"step {t}")
            finished += ids.size
    assert finished >= 2 * n
    env.close(); twin.close()


def test_without_terminal_the_adapters_are_as_before(hip_lib):
    """9.  A stack without terminal=True is accepted and not exposed"""
    from gym_lowcostrobot_amd import LowCostRobotVecEnv

    env = LowCostRobotVecEnv("reach", 4, obs_stack=4, observation_mode="both", image_size=SMALL, max_episode_steps=2)
    sp = env.observation_space.spaces if hasattr(env.observation_space, "spaces") else env.observation_space
    assert "obs_stack" not in sp and "point_cloud" not in sp
    env.reset()
    for _ in range(2):
        obs, _, dones, infos = env.step(np.zeros((4, env.sim.action_dim), np.float32))
    assert dones.all() and "obs_stack" not in obs and all("obs_stack" not in i["terminal_observation"] for i in infos)
    env.close()
