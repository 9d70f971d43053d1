"""The wrist camera: a third, link-mounted image observation (VecSim(..., wrist_camera=True | dict(link=, pos=, xyaxes=, fovy_deg=)); lcr_enable_wrist_camera).
Definitions: include/lcr.h; tests/wrist_ref.py restates them in numpy.

Bounds -- the project's, imported from the tests that own them, none restated or widened:
  * against wrist_ref (fp64, per pixel): pixels beyond +-2 levels per frame <= test_gpu_image_size._oracle_pixels(H, W) = 0.001 * max(1, 320 / W) * W * H.  The
    reference's own fp32 twin stays at <= 6 pixels for the states and both mounts used here (tests/test_wrist_abi.py: default mount 1 / 1 / 5 at 84 x 84 / 36 x 52 /
    120 x 160, second mount 3 / 1 / 6, against 26.9 / 11.5 / 38.4 allowed), which leaves the bound to fp32 forward kinematics and hardware reciprocals.
  * against the one-ray-per-pixel path of the same library (sim.render(e, "camera_wrist")): <= test_gpu_image_size._raycast_pixels(H, W).
  * planes against wrist_ref: planes_ref.agree at 1e-4 relative depth, disagreeing pixels <= test_gpu_image_planes._ref_pixels(H, W); against the per-pixel path 1e-5.
  * everything called "identical": byte for byte.
"""
import ctypes

import numpy as np
import pytest

from tests import look_ref, planes_ref, wrist_ref
from tests.test_gpu_image_planes import _ref_pixels
from tests.test_gpu_image_size import _oracle_pixels, _random_poses, _raycast_pixels, _terminal_qpos
from tests.test_look_abi import gpu_test_colours

pytestmark = pytest.mark.gpu

BOTH = ("depth", "segmentation")
MOUNTS = {"default": wrist_ref.default_mount(), "other": wrist_ref.OTHER_MOUNT}
SAMPLER = {"seed": 77, "cube": ([0.2, 0.0, 0.0], [1.0, 0.6, 0.3]), "cube2": ([0.0, 0.1, 0.3], [0.4, 0.9, 1.0]), "marker": ([0.0, 0.5, 0.2], [0.3, 0.5, 1.0])}


def _kw(m):
    """a reference mount as the wrist_camera keyword"""
    return {"link": m["link"], "pos": tuple(m["pos"]), "xyaxes": tuple(m["xyaxes"]), "fovy_deg": m["fovy_deg"]}


def _bad_pixels(got, ref):
    d = np.abs(got.astype(int) - ref.astype(int)).max(-1)
    return int((d > 2).sum()), np.argwhere(d > 2)[:5].tolist()


REF_CASES = [(t, w, s) for t in ("push", "stack", "pick_place") for w in ("default", "other") for s in ((84, 84), (36, 52))] + [("stack", "default", (120, 160))]


@pytest.mark.parametrize("task,which,size", REF_CASES, ids=[f"{t}-{w}-{s[0]}x{s[1]}" for t, w, s in REF_CASES])
def test_wrist_frames_and_planes_vs_the_fp64_reference(hip_lib, task, which, size):
    """1. 8 random states (seed 17; state 0 has the default camera below the floor), the default mount and a second one (link 4, other axes, fovy 90): colours and planes.
    120 x 160 runs once (stack, default mount)"""
    from gym_lowcostrobot_amd import VecSim

    H, W = size
    n = 8
    m = MOUNTS[which]
    sim = VecSim(task, n, observation_mode="both", auto_reset=False, image_size=size, wrist_camera=_kw(m), image_planes=BOTH, depth_far=10.0)
    assert sim.image_wrist.shape == (n, H, W, 3) and sim.depth_wrist.shape == (n, H, W) and sim.seg_wrist.dtype == np.uint8
    assert sim.wrist_camera["link"] == m["link"] and sim.wrist_camera["fovy_deg"] == m["fovy_deg"]
    qpos, target = _random_poses(task, n, np.random.default_rng(17), sim.get_state())
    sim.set_state(qpos=qpos, target=target)
    sim.reset(mask=np.zeros(n, np.uint8))            # no env reset, but re-renders frames and planes from the new state
    obs = sim.observations()
    keys = list(obs)
    assert keys[keys.index("image_top") + 1] == "image_wrist" and keys[keys.index("segmentation_top") + 1:keys.index("segmentation_top") + 3] == ["depth_wrist", "segmentation_wrist"]
    if which == "default":
        assert wrist_ref.camera(m, qpos[:, 0])[0][2] < 0     # the floor rule is exercised
    worst, worst_pl, fails = 0, 0, []
    for e in range(n):
        ref = wrist_ref.render(task, qpos[:, e], target[:, e], m, W, H)
        assert ref.shape == (H, W, 3) and ref.std() > 5
        bad, where = _bad_pixels(obs["image_wrist"][e], ref)
        worst = max(worst, bad)
        if bad > _oracle_pixels(H, W):
            fails.append((e, "colour", bad, where))
        dref, sref = wrist_ref.planes(task, qpos[:, e], target[:, e], m, W, H, depth_far=10.0)
        ok = planes_ref.agree(obs["depth_wrist"][e], obs["segmentation_wrist"][e], dref, sref, 1e-4)
        worst_pl = max(worst_pl, int((~ok).sum()))
        if int((~ok).sum()) > _ref_pixels(H, W):
            fails.append((e, "planes", int((~ok).sum()), np.argwhere(~ok)[:5].tolist()))
    print(f"[wrist vs fp64 reference] {task} {which} {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_oracle_pixels(H, W):.1f}), "
          f"worst {worst_pl} disagreeing plane pixels (allowed {_ref_pixels(H, W):.1f})")
    sim.close()
    assert not fails, (task, which, size, fails)


@pytest.mark.parametrize("cam,key", [("camera_front", "image_front"), ("camera_top", "image_top")])
def test_a_world_mount_at_a_scene_camera_draws_that_camera(hip_lib, cam, key):
    """2. the anchor to the committed oracle: link 0 with the pose of a scene camera against oracle.render_oracle.render, and against the two-camera kernel's own frame"""
    from gym_lowcostrobot_amd import VecSim
    from oracle import render_oracle

    task, n = "push", 8
    H, W = size = (84, 84)
    m = wrist_ref.scene_camera_mount(task, cam)
    sim = VecSim(task, n, observation_mode="both", auto_reset=False, image_size=size, wrist_camera=_kw(m))
    qpos, target = _random_poses(task, n, np.random.default_rng(17), sim.get_state())
    sim.set_state(qpos=qpos, target=target)
    sim.reset(mask=np.zeros(n, np.uint8))
    wr, fixed = sim.image_wrist.numpy(), getattr(sim, key).numpy()
    worst = [0, 0]
    for e in range(n):
        ref = render_oracle.render(task, qpos[:, e], target[:, e], cam, W, H)
        assert ref.std() > 5
        bad, where = _bad_pixels(wr[e], ref)
        worst[0] = max(worst[0], bad)
        assert bad <= _oracle_pixels(H, W), (cam, e, bad, where)
        bad, where = _bad_pixels(wr[e], fixed[e])
        worst[1] = max(worst[1], bad)
        assert bad <= _raycast_pixels(H, W), (cam, e, bad, where)
    print(f"[wrist at {cam}] vs oracle: worst {worst[0]} (allowed {_oracle_pixels(H, W):.1f}); vs {key}: worst {worst[1]} (allowed {_raycast_pixels(H, W):.1f})")
    sim.close()


@pytest.mark.parametrize("size,which", [((84, 84), "default"), ((36, 52), "other")], ids=["84x84-default", "36x52-other"])
@pytest.mark.parametrize("n", [24, 25, 1])
@pytest.mark.parametrize("task", ["push", "stack", "pick_place"])
def test_culling_drops_nothing(hip_lib, task, n, size, which):
    """3. the batched frame and planes against the one-ray-per-pixel path of the same env after 15 random steps; n = 25 and n = 1 leave a workgroup partly empty"""
    from gym_lowcostrobot_amd import VecSim

    H, W = size
    sim = VecSim(task, n, observation_mode="both", base_seed=11, image_size=size, wrist_camera=_kw(MOUNTS[which]), image_planes=BOTH)
    rng = np.random.default_rng(5)
    for _ in range(15):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
    wr, dw, sw = sim.image_wrist.numpy(), sim.depth_wrist.numpy(), sim.seg_wrist.numpy()
    worst, worst_pl, fails = 0, 0, []
    for e in range(n):
        ref = sim.render(e, "camera_wrist", W, H)
        assert ref.std() > 5
        bad, where = _bad_pixels(wr[e], ref)
        worst = max(worst, bad)
        if bad > _raycast_pixels(H, W):
            fails.append((e, "colour", bad, where))
        d1, s1 = sim.render_planes(e, "camera_wrist", W, H)
        badpl = int((~planes_ref.agree(dw[e], sw[e], d1, s1, 1e-5)).sum())
        worst_pl = max(worst_pl, badpl)
        if badpl > _raycast_pixels(H, W):
            fails.append((e, "planes", badpl))
    print(f"[wrist tile path] {task} n={n} {H}x{W} {which}: worst {worst} pixels, {worst_pl} plane pixels (allowed {_raycast_pixels(H, W):.1f})")
    sim.close()
    assert not fails, (task, n, size, fails)


def test_the_wrist_camera_moves_nothing_else(hip_lib):
    """4a. two sims, same seed and actions, one with the wrist camera: the two scene cameras' frames and planes, the state, the outputs and the state observations are
    bit-identical over 20 steps with auto-resets (the pattern of test_sized_frames_write_nowhere_else); 4b, the guard bytes, is the next test"""
    from gym_lowcostrobot_amd import VecSim

    n = 67
    kw = dict(observation_mode="both", base_seed=8, max_episode_steps=4, image_size=(36, 52), image_planes=BOTH)
    sims = [VecSim("stack", n, **kw), VecSim("stack", n, wrist_camera=True, **kw)]
    assert sims[0].image_wrist is None and sims[0].wrist_camera is None and "image_wrist" not in sims[0].observations()
    rng = np.random.default_rng(6)
    for t in range(20):
        a = rng.uniform(-1, 1, (n, sims[0].action_dim)).astype(np.float32)
        for s_ in sims:
            s_.step(a)
        if t % 5 == 4:
            for k in ("image_front", "image_top", "depth_front", "depth_top", "seg_front", "seg_top"):
                np.testing.assert_array_equal(getattr(sims[0], k).numpy(), getattr(sims[1], k).numpy(), err_msg=f"step {t} {k}")
    sa, sb = (s_.get_state() for s_ in sims)
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"state {k}")
    oa, ob = (s_.outputs() for s_ in sims)
    for k in oa:
        np.testing.assert_array_equal(oa[k], ob[k], err_msg=f"output {k}")
    for k in ("arm_qpos", "arm_qvel", "cube_pos", "aux_pos", "terminal_obs", "terminal_quat"):
        np.testing.assert_array_equal(getattr(sims[0], k).numpy(), getattr(sims[1], k).numpy(), err_msg=k)
    wr = sims[1].image_wrist.numpy()
    assert all(wr[e].std() > 5 for e in range(n))
    for s_ in sims:
        s_.close()


def _guards(sim, arr):
    """the guard regions around a wrist buffer (include/lcr.h: LCR_WRIST_GUARD): the bytes before it, and from its end over the padding to the end of the region behind it"""
    from gym_lowcostrobot_amd import _capi
    from gym_lowcostrobot_amd.vecsim import DeviceArray

    G = _capi.WRIST_GUARD
    tail = (arr.nbytes + 255) // 256 * 256 - arr.nbytes + G
    return DeviceArray(sim, arr.ptr - G, (G,), np.uint8).numpy(), DeviceArray(sim, arr.ptr + arr.nbytes, (tail,), np.uint8).numpy()


@pytest.mark.parametrize("look", [False, True], ids=["plain", "look"])
@pytest.mark.parametrize("size", [(36, 52), (84, 84), (16, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [25, 24, 1])
def test_guard_bytes_around_the_wrist_buffers_are_untouched(hip_lib, n, size, look):
    """4b. image_wrist, depth_wrist and seg_wrist lie between guard regions filled with LCR_WRIST_GUARD_BYTE when they are allocated.  After the enable calls, steps with
    auto-resets (second stream), a full and a masked reset and a terminal-frame call every guard byte still holds the pattern, while the buffers themselves were drawn.
    n = 25 and n = 1 leave a workgroup of the several-envs mapping partly empty; 52 and 20 wide have a partial last tile column; 16 x 20 is the smallest frame"""
    from gym_lowcostrobot_amd import VecSim, _capi

    kw = dict(look_variants=look_ref.GPU_VARIANTS, look_sampler=SAMPLER) if look else {}
    sim = VecSim("stack", n, observation_mode="both", base_seed=8, max_episode_steps=4, image_size=size, wrist_camera=True, image_planes=BOTH, **kw)
    bufs = {"image_wrist": sim.image_wrist, "depth_wrist": sim.depth_wrist, "seg_wrist": sim.seg_wrist}

    def check(when):
        for k, a in bufs.items():
            for side, g in zip(("before", "behind"), _guards(sim, a)):
                assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (when, k, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())

    check("after the enable calls")
    rng = np.random.default_rng(6)
    for t in range(9):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
        if t in (3, 8):
            check(f"step {t}")
    fin = np.nonzero(sim.outputs()["did_reset"])[0].astype(np.int32)
    if fin.size:
        sim.render_terminal_wrist(fin)
    sim.reset()
    sim.reset(mask=(np.arange(n) % 2).astype(np.uint8))
    sim.render(n - 1, "camera_wrist", size[1], size[0]); sim.render_planes(0, "camera_wrist", size[1], size[0])
    check("after the resets")
    wr, dw, sw = (a.numpy() for a in bufs.values())
    assert all(wr[e].std() > 5 for e in range(n))
    assert (dw > 0).all() and (dw <= 10.0).all() and ((sw & 0x7F) <= 10).all()          # every plane value is a drawn one: none still holds the fill pattern
    sim.close()


def test_wrist_frames_on_the_second_stream_are_the_serial_frames(hip_lib, monkeypatch):
    """5. frames ray-cast on the second stream from the pose snapshot (default) and on the caller's stream after each step kernel (LCR_RENDER_OVERLAP=0): byte-identical"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 192, (84, 84)
    kw = dict(observation_mode="both", base_seed=3, max_episode_steps=7, image_size=size, wrist_camera=True, image_planes=BOTH)
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", n, **kw)
    acts = [(s_, s_.alloc_actions()) for s_ in (ref, ovl)]

    def same():
        for k in ("image_wrist", "depth_wrist", "seg_wrist", "image_front"):
            np.testing.assert_array_equal(getattr(ref, k).numpy(), getattr(ovl, k).numpy(), err_msg=k)

    same()
    t = 0
    for burst in (1, 1, 9, 3, 12):          # episodes end every 7 steps: auto-resets fall inside the bursts
        for _ in range(burst):
            for s_, a in acts:
                s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
            t += 1
        same()
    assert ref.image_wrist.numpy().std() > 5
    for s_, a in acts:
        s_.free(a); s_.close()


@pytest.mark.parametrize("task", ["push", "stack"])
def test_wrist_frames_take_the_look(hip_lib, task):
    """6. four variants that use every field and explicit per-env colours: the wrist frames against the reference drawn with the env's variant's floor, sky, light and arm
    colours and its own colours (the variant's camera offsets do not move the wrist camera); enabling the look after the wrist camera draws the same bytes"""
    from gym_lowcostrobot_amd import VecSim, _capi

    H, W = size = (84, 84)
    n = 8
    m = MOUNTS["default"]
    kw = dict(observation_mode="both", auto_reset=False, image_size=size, wrist_camera=True)
    sim = VecSim(task, n, look_variants=look_ref.GPU_VARIANTS, **kw)
    qpos, target = _random_poses(task, n, np.random.default_rng(17), sim.get_state())
    variant = (np.arange(n) % 4).astype(np.int32)
    rgb = gpu_test_colours(n)
    sim.set_state(qpos=qpos, target=target)
    sim.set_look(variant=variant, rgb=rgb)            # redraws the frames from the new state
    wr = sim.image_wrist.numpy()
    worst = 0
    for e in range(n):
        ref = wrist_ref.render(task, qpos[:, e], target[:, e], m, W, H, v=look_ref.GPU_VARIANTS[variant[e]], rgb=rgb[:, e])
        assert ref.std() > 5
        bad, where = _bad_pixels(wr[e], ref)
        worst = max(worst, bad)
        assert bad <= _oracle_pixels(H, W), (task, e, bad, where)
        bad, _ = _bad_pixels(wr[e], sim.render(e, "camera_wrist", W, H))        # the look-aware per-pixel path
        assert bad <= _raycast_pixels(H, W), (task, e, bad)
    print(f"[wrist looks vs fp64 reference] {task} {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_oracle_pixels(H, W):.1f})")
    # the other order: wrist camera first, look second
    late = VecSim(task, n, **kw)
    arr = (_capi.LookVariant * 4)(*sim.look_variants)
    assert hip_lib.lcr_enable_look(late.handle, 4, arr, None) == 0, hip_lib.lcr_last_error()
    late.look_variants = list(sim.look_variants)
    late.set_state(qpos=qpos, target=target)
    late.set_look(variant=variant, rgb=rgb)
    np.testing.assert_array_equal(late.image_wrist.numpy(), wr)
    sim.close(); late.close()


def test_terminal_wrist_frames_show_the_terminal_look(hip_lib):
    """6b. max_episode_steps = 3 with a sampler: the terminal wrist frames of the envs a step finished are drawn with the look the episode had"""
    from gym_lowcostrobot_amd import VecSim

    task, n = "push", 64
    H, W = size = (84, 84)
    sim = VecSim(task, n, observation_mode="both", base_seed=4, max_episode_steps=3, image_size=size, wrist_camera=True, look_variants=look_ref.GPU_VARIANTS, look_sampler=SAMPLER)
    act = sim.alloc_actions()
    worst, checked = 0, 0
    for t in range(6):
        before = sim.look()
        sim.fill_random_actions(act, 9, t); sim.step_device(act.ptr)
        fin = np.nonzero(sim.outputs()["did_reset"])[0]
        if fin.size == 0:
            continue
        ids = fin[:4].astype(np.int32)
        got = sim.render_terminal_wrist(ids)["image_wrist"]
        tob, tq = sim.terminal_obs.numpy(), sim.terminal_quat.numpy()
        for j, e in enumerate(ids.tolist()):
            qpos, tgt = _terminal_qpos(sim, tob, tq, e)
            ref = wrist_ref.render(task, qpos, tgt, MOUNTS["default"], W, H, v=look_ref.GPU_VARIANTS[before["variant"][e]], rgb=before["rgb"][:, e])
            bad, where = _bad_pixels(got[j], ref)
            worst = max(worst, bad); checked += 1
            assert bad <= _oracle_pixels(H, W), (t, e, bad, where)
    assert checked >= 4
    print(f"[terminal wrist looks vs fp64 reference] {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_oracle_pixels(H, W):.1f})")
    sim.free(act); sim.close()


@pytest.mark.parametrize("task", ["push", "stack"])
def test_terminal_wrist_frames_and_adapters(hip_lib, task, tmp_path):
    """7. batched terminal wrist frames (and planes) against render_state / render_state_planes of the terminal poses; both vector adapters deliver image_wrist and its
    terminal observation; the recorder writes observations/images/wrist"""
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, LowCostRobotVectorEnv, VecSim, recorder
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    H = W = 64
    n = 50
    v = LowCostRobotVecEnv(task, n, observation_mode="both", max_episode_steps=3, seed=5, image_size=(H, W), wrist_camera=True, image_planes=BOTH)
    for k, shape in (("image_wrist", (H, W, 3)), ("depth_wrist", (H, W)), ("segmentation_wrist", (H, W))):
        assert v.observation_space[k].shape == shape, k
    obs = v.reset()
    assert obs["image_wrist"].shape == (n, H, W, 3) and obs["image_wrist"].dtype == np.uint8
    rng = np.random.default_rng(1)
    for _ in range(3):
        obs, rew, dones, infos = v.step(rng.uniform(-1, 1, (n, v.action_space.shape[0])).astype(np.float32))
    assert dones.mean() > 0.5 and obs["image_wrist"].shape == (n, H, W, 3)
    np.testing.assert_array_equal(obs["image_wrist"], v.sim.image_wrist.numpy())
    fin = np.nonzero(dones)[0]
    sim = v.sim
    tob, tq = sim.terminal_obs.numpy(), sim.terminal_quat.numpy()
    term = sim.render_terminal_wrist(fin.astype(np.int32))
    assert list(term) == ["image_wrist", "depth_wrist", "segmentation_wrist"] and term["image_wrist"].shape == (len(fin), H, W, 3)
    worst = 0
    for j, e in enumerate(fin.tolist()):
        qpos, tgt = _terminal_qpos(sim, tob, tq, e)
        ref = sim.render_state(qpos, tgt, "camera_wrist", W, H)
        assert ref.std() > 5
        bad, where = _bad_pixels(term["image_wrist"][j], ref)
        worst = max(worst, bad)
        assert bad <= _raycast_pixels(H, W), (task, e, bad, where)
        d1, s1 = sim.render_state_planes(qpos, tgt, "camera_wrist", W, H)
        assert int((~planes_ref.agree(term["depth_wrist"][j], term["segmentation_wrist"][j], d1, s1, 1e-5)).sum()) <= _raycast_pixels(H, W), (task, e)
        tobs = infos[e]["terminal_observation"]
        for k in ("image_wrist", "depth_wrist", "segmentation_wrist"):
            np.testing.assert_array_equal(tobs[k], term[k][j], err_msg=k)
    print(f"[terminal wrist frames] {task}: worst {worst} pixels beyond +-2 levels (allowed {_raycast_pixels(H, W):.1f})")
    assert np.abs(obs["image_wrist"][fin[0]].astype(int) - term["image_wrist"][0].astype(int)).max() > 20   # the reset frame is not the terminal frame
    if (~dones).any():
        with pytest.raises(ValueError, match="did_reset"):
            sim.render_terminal_wrist(np.nonzero(~dones)[0][:1].astype(np.int32))
    v.close()

    g = LowCostRobotVectorEnv(task, 12, observation_mode="both", max_episode_steps=3, seed=5, image_size=(H, W), wrist_camera=True)
    assert g.single_observation_space["image_wrist"].shape == (H, W, 3)
    o, _ = g.reset(seed=1)
    assert o["image_wrist"].shape == (12, H, W, 3)
    for _ in range(3):
        o, r, te, tr, infos = g.step(rng.uniform(-1, 1, (12, g.single_action_space.shape[0])).astype(np.float32))
    assert (te | tr).all() and infos["_final_obs"].all()
    assert infos["final_obs"]["image_wrist"].shape == (12, H, W, 3) and all(infos["final_obs"]["image_wrist"][e].std() > 5 for e in range(12))
    np.testing.assert_array_equal(infos["final_obs"]["image_wrist"], g._v.sim.render_terminal_wrist(np.arange(12, dtype=np.int32))["image_wrist"])
    assert np.abs(infos["final_obs"]["image_wrist"][0].astype(int) - o["image_wrist"][0].astype(int)).max() > 20      # ... and not the reset frame
    g.close()

    sh = ShardedVecSim(task, 128, [0, 0], observation_mode="both", image_size=(36, 52), wrist_camera={"link": 4})
    assert all(s_.image_wrist.shape == (64, 36, 52, 3) and s_.wrist_camera["link"] == 4 for s_ in sh.shards)
    sh.close()

    sim = VecSim(task, 16, observation_mode="both", max_episode_steps=3, image_size=(H, W), wrist_camera=True)
    rec = recorder.VecRecorder(sim, str(tmp_path), which=(0, 5))
    frames = {0: [], 5: []}
    for t in range(6):
        a = rng.uniform(-1, 1, (16, sim.action_dim)).astype(np.float32)
        sim.step(a)
        rec.after_step(a)
        live, dres = sim.image_wrist.numpy(), sim.outputs()["did_reset"]
        tob, tq = sim.terminal_obs.numpy(), sim.terminal_quat.numpy()
        for e in frames:   # what the episode's file must hold for this step: the live frame, or -- where the step ended the episode -- the frame of the terminal pose
            frames[e].append(sim.render_state(*_terminal_qpos(sim, tob, tq, e), "camera_wrist", W, H) if dres[e] else live[e])
    rec.close()
    assert len(rec.files) >= 4
    first = sorted(rec.files)[0]
    ep = recorder.load_episode(first)
    T = ep["action"].shape[0]
    im = ep["observations/images/wrist"]
    assert 1 <= T <= 3 and im.shape == (T, H, W, 3) and im.dtype == np.uint8 and all(im[i].std() > 5 for i in range(T))
    e0 = 0 if "env0-" in first else 5
    for i in range(T):          # read back equal: the live frames of the steps before the episode's last, then the frame of the terminal pose
        np.testing.assert_array_equal(im[i], frames[e0][i], err_msg=f"frame {i}")
    sim.close()


def test_live_handle_refusals(hip_lib):
    """8. the wrist camera after the planes, a second enable with other arguments, camera 3 on a handle without a wrist camera, a handle without frames"""
    from gym_lowcostrobot_amd import VecSim, _capi

    cam = _capi.WristCamera.from_any(True)
    st = VecSim("reach", 4, observation_mode="state")
    assert hip_lib.lcr_enable_wrist_camera(st.handle, ctypes.byref(cam)) == _capi.LCR_ERR_INVALID and b"observation_mode" in hip_lib.lcr_last_error()
    st.close()
    late = VecSim("reach", 4, observation_mode="both", image_size=(36, 52), image_planes=("depth",))
    assert hip_lib.lcr_enable_wrist_camera(late.handle, ctypes.byref(cam)) == _capi.LCR_ERR_INVALID and b"planes" in hip_lib.lcr_last_error()
    wv = _capi.LcrWristView()
    assert hip_lib.lcr_get_wrist_camera(late.handle, ctypes.byref(wv)) == 0 and wv.enabled == 0 and not wv.image_wrist
    with pytest.raises(ValueError, match="camera"):
        late.render(0, "camera_wrist", 52, 36)
    with pytest.raises(ValueError, match="camera"):
        late.render_planes(0, "camera_wrist", 52, 36)
    with pytest.raises(ValueError, match="camera"):
        late.render_state(np.zeros(late.nq), None, "camera_wrist", 52, 36)
    with pytest.raises(ValueError, match="wrist"):
        late.render_terminal_wrist([0])
    assert hip_lib.lcr_render_terminal_wrist(late.handle, None, 0, None, None, None) == _capi.LCR_ERR_INVALID and b"lcr_enable_wrist_camera" in hip_lib.lcr_last_error()
    late.close()
    sim = VecSim("reach", 4, observation_mode="image", image_size=(36, 52), wrist_camera={"link": 3, "fovy_deg": 75.0})
    before = sim.image_wrist.numpy()
    same = _capi.WristCamera.from_any({"link": 3, "fovy_deg": 75.0})
    assert hip_lib.lcr_enable_wrist_camera(sim.handle, ctypes.byref(same)) == 0
    assert hip_lib.lcr_enable_wrist_camera(sim.handle, ctypes.byref(cam)) == _capi.LCR_ERR_INVALID and b"fixed for the life of the handle" in hip_lib.lcr_last_error()
    np.testing.assert_array_equal(sim.image_wrist.numpy(), before)
    assert hip_lib.lcr_get_wrist_camera(sim.handle, ctypes.byref(wv)) == 0 and wv.enabled == 1 and wv.camera.link == 3 and wv.camera.fovy_deg == 75.0
    assert (wv.image_width, wv.image_height) == (52, 36) and wv.image_wrist == sim.image_wrist.ptr and not wv.depth_wrist and not wv.seg_wrist and wv.depth_far == 0.0
    assert sim.render(0, "camera_wrist", 40, 30).shape == (30, 40, 3)          # any size
    d = np.empty((36, 52), np.float32)
    assert hip_lib.lcr_render_terminal_wrist(sim.handle, None, 0, None, d.ctypes.data_as(ctypes.c_void_p), None) == _capi.LCR_ERR_INVALID     # a plane that is not enabled
    sim.close()
