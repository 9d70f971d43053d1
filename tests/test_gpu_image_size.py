"""Image observations at a caller-chosen frame size (VecSim(..., image_size=(H, W)); lcr_config.image_width / image_height, ABI v7).

Sizes: square and not, W % 16 of 0 and 4 (a partial last tile column), fewer bands than the eight band-rotation phases of the frame kernel (36 rows = 9
bands), the widest row (512), and sizes on both sides of the kernel's several-envs-per-workgroup mapping for small frames.

Bounds.  A pixel agrees when all channels are within +-2 levels (the project's rule for its two fp32 paths and the fp64 oracle).
  * against the CPU oracle (oracle/render_oracle.py, fp64, per pixel): share of agreeing pixels per frame >= 1 - 0.001 * max(1, 320 / W).  The project's 0.999 at
    320 wide allows 76 pixels; the pixels that can fall on the other side of an fp32 edge lie along silhouettes and checker boundaries, so their count scales with the
    linear size while the pixel count scales with its square.  Derived, not measured -- and then checked on the PARENT commit's per-pixel path (sim.render(e, cam, W, H), which
    took any size before this feature) against the oracle for the same states; worst pixels beyond +-2 per frame, the same for all four tasks (they are background pixels):
        64x64: 26 (share 0.00635, derived allowance 0.00500 = 20.5 px)      84x84: 0      36x52: 0      120x160: 5 (0.00026)      128x128: 0      256x512: 5 (0.00004)
        240x320: 2 (0.00003)
    At 64 x 64 the parent's own path misses the derived bound: all 26 pixels lie in row 4 of camera_front, the first row below the horizon: its rays dip by 2e-4 rad and meet the 0.1-m
    checker floor a kilometre away, where fp32 and fp64 disagree about the cell.  The bound there is therefore the parent path's worst count plus one pixel, 27 of 4 096 (_PARENT_PATH_PIXELS);
    every other size keeps the derived bound.  The batched kernel of this feature measures the same 26 at 64 x 64.
  * against the per-pixel ray-caster of lcr_render (fp32, shares box_hit with the frame kernel): pixels beyond +-2 per frame <= max(2, 2e-4 * max(1, 320 / W) * W * H) --
    the existing share of 2e-4 at 320 wide scaled the same way, and at least two pixels so that one edge pixel cannot fail a 36 x 52 frame.  A culled primitive shows as
    tens of pixels.
"""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (84, 84), (36, 52), (120, 160), (128, 128), (256, 512)]   # (H, W)
CAMS = (("camera_front", "image_front"), ("camera_top", "image_top"))


_PARENT_PATH_PIXELS = {(64, 64): 26 + 1}   # (H, W): sizes where the parent's per-pixel path itself exceeds the derived bound -> its worst count plus one pixel (module docstring)


def _oracle_pixels(H, W):
    """pixels of a frame that may differ from the oracle by more than 2 levels"""
    return max(0.001 * max(1.0, 320.0 / W) * W * H, _PARENT_PATH_PIXELS.get((H, W), 0))


def _raycast_pixels(H, W):
    return max(2.0, 2e-4 * max(1.0, 320.0 / W) * W * H)


def _random_poses(task, n, rng, st):
    """the states of test_image_observations_vs_cpu_raycaster (test_gpu_parity.py)"""
    qpos = st["qpos"].copy()
    q, _ = util.random_arm_state(rng, n)
    qpos[:6] = q.T
    for c in range(2 if task == "stack" else 1):
        qpos[6 + 7 * c] = rng.uniform(-0.15, 0.15, n); qpos[7 + 7 * c] = rng.uniform(0.0, 0.3, n); qpos[8 + 7 * c] = rng.uniform(0.015, 0.08, n)
        quat = rng.normal(size=(4, n)); quat /= np.linalg.norm(quat, axis=0)
        qpos[9 + 7 * c: 13 + 7 * c] = quat
    target = np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(0.0, 0.3, n), rng.uniform(0, 0.1, n)]).astype(np.float32)
    return qpos.astype(np.float32).astype(np.float64), target


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", ["push", "stack", "pick_place", "reach"])
def test_sized_frames_vs_cpu_raycaster(hip_lib, task, size):
    """1. the batched frames at every size against the fp64 oracle: 8 random states (seed 17) x 2 cameras"""
    from gym_lowcostrobot_amd import VecSim
    from oracle import render_oracle

    H, W = size
    n = 8
    rng = np.random.default_rng(17)
    sim = VecSim(task, n, observation_mode="both", auto_reset=False, image_size=size)
    assert sim.image_size == (H, W) and sim.image_front.shape == (n, H, W, 3) and sim.image_top.shape == (n, H, W, 3)
    qpos, target = _random_poses(task, n, rng, sim.get_state())
    sim.set_state(qpos=qpos, target=target)
    sim.reset(mask=np.zeros(n, np.uint8))            # no env reset, but re-renders the frames from the new state
    obs = sim.observations()
    assert obs["image_front"].shape == (n, H, W, 3)
    worst, fails = 0, []
    for e in range(n):
        for cam, key in CAMS:
            ref = render_oracle.render(task, qpos[:, e], target[:, e], cam, W, H).astype(int)
            assert ref.shape == (H, W, 3) and ref.std() > 5
            d = np.abs(obs[key][e].astype(int) - ref).max(-1)
            bad = int((d > 2).sum())
            worst = max(worst, bad)
            if bad > _oracle_pixels(H, W):
                fails.append((e, cam, bad, np.argwhere(d > 2)[:5].tolist()))
    print(f"[sized frames vs oracle] {task} {H}x{W}: worst {worst} pixels beyond +-2 levels = share {worst / (W * H):.5f} (allowed {_oracle_pixels(H, W):.1f} pixels)")
    sim.close()
    assert not fails, (task, size, fails)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [24, 25, 1])
@pytest.mark.parametrize("task", ["push", "stack", "pick_place"])
def test_sized_tile_path_matches_per_pixel_raycast(hip_lib, task, n, size):
    """2. culling drops nothing at any size: the batched frames against lcr_render's one-thread-per-pixel ray-cast of the same env and camera after 15 random steps;
    n = 25 and n = 1 leave a workgroup of the several-envs-per-workgroup mapping partly empty"""
    from gym_lowcostrobot_amd import VecSim

    H, W = size
    sim = VecSim(task, n, observation_mode="both", base_seed=11, image_size=size)
    rng = np.random.default_rng(5)
    for _ in range(15):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
    obs = sim.observations()
    worst, fails = 0, []
    for e in range(n):
        for name, key in CAMS:
            ref = sim.render(e, name, W, H).astype(int)
            d = np.abs(obs[key][e].astype(int) - ref).max(-1)
            bad = int((d > 2).sum())
            worst = max(worst, bad)
            if bad > _raycast_pixels(H, W):
                fails.append((e, name, bad, np.argwhere(d > 2)[:5].tolist()))
    print(f"[sized tile path] {task} n={n} {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_raycast_pixels(H, W):.1f})")
    sim.close()
    assert not fails, (task, n, size, fails)


@pytest.mark.parametrize("epw", ["1", "2", "4"])
@pytest.mark.parametrize("size", [(64, 64), (36, 52), (120, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_small_frame_mapping_draws_the_same_bytes(hip_lib, monkeypatch, size, epw):
    """the mappings of the frame kernel for small frames (one, two or four envs per workgroup; chosen from the frame size, LCR_RENDER_EPW pins one for measurements)
    regroup the same arithmetic: byte-identical frames, and a ragged batch (n = 27: 27 = 6 x 4 + 3 = 13 x 2 + 1) writes every env's frames and nothing else"""
    from gym_lowcostrobot_amd import VecSim

    n = 27
    sims = []
    for v in ("1", epw):
        monkeypatch.setenv("LCR_RENDER_EPW", v)
        sims.append(VecSim("stack", n, observation_mode="both", base_seed=4, image_size=size))
    monkeypatch.delenv("LCR_RENDER_EPW")
    acts = [(s_, s_.alloc_actions()) for s_ in sims]
    for t in range(6):
        for s_, a in acts:
            s_.fill_random_actions(a, 9, t); s_.step_device(a.ptr)
    for k in ("image_front", "image_top"):
        a, b = (getattr(s_, k).numpy() for s_ in sims)
        np.testing.assert_array_equal(a, b, err_msg=k)
        assert all(a[e].std() > 5 for e in range(n))
    np.testing.assert_array_equal(sims[0].get_state()["qpos"], sims[1].get_state()["qpos"])
    for s_, a in acts:
        s_.free(a); s_.close()


@pytest.mark.parametrize("task", ["stack", "push"])
def test_the_default_size_did_not_move(hip_lib, task):
    """3. image_size=None and image_size=(240, 320) are the same frames, byte for byte"""
    from gym_lowcostrobot_amd import VecSim

    n = 40
    sims = [VecSim(task, n, observation_mode="both", base_seed=2, image_size=sz) for sz in (None, (240, 320))]
    for s_ in sims:
        assert s_.image_size == (240, 320) and s_.image_front.shape == (n, 240, 320, 3)
    rng = np.random.default_rng(3)
    for _ in range(5):
        a = rng.uniform(-1, 1, (n, sims[0].action_dim)).astype(np.float32)
        for s_ in sims:
            s_.step(a)
    for k in ("image_front", "image_top"):
        a, b = (getattr(s_, k).numpy() for s_ in sims)
        np.testing.assert_array_equal(a, b, err_msg=k)
        assert a.std() > 5
    for s_ in sims:
        s_.close()
    st = VecSim(task, 4, observation_mode="state")
    assert st.image_size == (240, 320) and st.image_front is None
    st.close()


def test_sized_frames_on_the_second_stream_are_the_serial_frames(hip_lib, monkeypatch):
    """4. at 84 x 84: frames ray-cast on the second stream (default) and on the caller's stream after each step kernel (LCR_RENDER_OVERLAP=0) are byte-identical"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 192, (84, 84)
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, observation_mode="both", base_seed=3, max_episode_steps=7, image_size=size)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", n, observation_mode="both", base_seed=3, max_episode_steps=7, image_size=size)
    acts = [(s_, s_.alloc_actions()) for s_ in (ref, ovl)]

    def same():
        for k in ("image_front", "image_top"):
            np.testing.assert_array_equal(getattr(ref, k).numpy(), getattr(ovl, k).numpy(), err_msg=k)
        np.testing.assert_array_equal(ref.get_state()["qpos"], ovl.get_state()["qpos"])

    same()
    t = 0
    for burst in (1, 1, 9, 3, 12):          # episodes end every 7 steps: auto-resets fall inside the bursts
        for _ in range(burst):
            for s_, a in acts:
                s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
            t += 1
        same()
    assert ref.image_front.numpy().std() > 1.0 and ref.image_front.shape == (n, 84, 84, 3)
    for s_, a in acts:
        s_.free(a); s_.close()


def _terminal_qpos(sim, tob, tq, e):
    t = tob[:, e]
    qpos = np.zeros(sim.nq); qpos[0:6] = t[0:6]; qpos[6:9] = t[12:15]; qpos[9:13] = tq[0:4, e]
    if sim.task_name == "stack":
        qpos[13:16] = t[15:18]; qpos[16:20] = tq[4:8, e]
    return qpos, (t[15:18] if sim.task_name in ("push", "pick_place") else None)


@pytest.mark.parametrize("task", ["push", "stack"])
def test_terminal_frames_and_adapters_at_a_small_size(hip_lib, task, tmp_path):
    """5. at 64 x 64 with max_episode_steps=3: batched terminal frames against render_state of the terminal poses; the SB3-style and gymnasium-style adapters report
    (64, 64, 3) image spaces and return observations / terminal observations of that shape; the recorder writes and reads back a (T, 64, 64, 3) episode"""
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, LowCostRobotVectorEnv, VecSim, recorder

    H = W = 64
    n = 50
    v = LowCostRobotVecEnv(task, n, observation_mode="both", max_episode_steps=3, seed=5, image_size=(H, W))
    assert v.observation_space["image_front"].shape == (H, W, 3) and v.observation_space["image_top"].shape == (H, W, 3)
    obs = v.reset()
    assert obs["image_front"].shape == (n, H, W, 3) and obs["image_top"].dtype == np.uint8
    rng = np.random.default_rng(1)
    for _ in range(3):
        obs, rew, dones, infos = v.step(rng.uniform(-1, 1, (n, v.action_space.shape[0])).astype(np.float32))
    assert dones.mean() > 0.5 and obs["image_front"].shape == (n, H, W, 3)
    fin = np.nonzero(dones)[0]
    sim = v.sim
    tob, tq = sim.terminal_obs.numpy(), sim.terminal_quat.numpy()
    fr, tp = sim.render_terminal(fin.astype(np.int32))
    assert fr.shape == (len(fin), H, W, 3) and tp.shape == (len(fin), H, W, 3) and fr.dtype == np.uint8 and tp.std() > 5
    worst = 0
    for j, e in enumerate(fin.tolist()):
        qpos, tgt = _terminal_qpos(sim, tob, tq, e)
        for got, key, cam in ((fr[j], "image_front", "camera_front"), (tp[j], "image_top", "camera_top")):
            ref = sim.render_state(qpos, tgt, cam, W, H).astype(int)
            bad = int((np.abs(ref - got.astype(int)).max(-1) > 2).sum())
            worst = max(worst, bad)
            assert bad <= _raycast_pixels(H, W), (task, e, key, bad)
            tobs = infos[e]["terminal_observation"][key]
            assert tobs.shape == (H, W, 3)
            np.testing.assert_array_equal(tobs, got)
    print(f"[sized terminal frames] {task}: worst {worst} pixels beyond +-2 levels (allowed {_raycast_pixels(H, W):.1f})")
    assert np.abs(obs["image_front"][fin[0]].astype(int) - fr[0].astype(int)).max() > 20   # the reset frame is not the terminal frame
    v.close()

    g = LowCostRobotVectorEnv(task, 12, observation_mode="both", max_episode_steps=3, seed=5, image_size=(H, W))
    assert g.single_observation_space["image_front"].shape == (H, W, 3)
    o, _ = g.reset(seed=1)
    assert o["image_top"].shape == (12, H, W, 3)
    for _ in range(3):
        o, r, term, trunc, infos = g.step(rng.uniform(-1, 1, (12, g.single_action_space.shape[0])).astype(np.float32))
    assert (term | trunc).all() and infos["_final_obs"].all()
    assert infos["final_obs"]["image_front"].shape == (12, H, W, 3) and infos["final_obs"]["image_top"].shape == (12, H, W, 3)
    assert all(infos["final_obs"]["image_front"][e].std() > 5 for e in range(12))
    g.close()

    sim = VecSim(task, 16, observation_mode="both", max_episode_steps=3, image_size=(H, W))
    rec = recorder.VecRecorder(sim, str(tmp_path), which=(0, 5))
    k = sim.action_dim
    for t in range(6):
        a = rng.uniform(-1, 1, (16, k)).astype(np.float32)
        sim.step(a)
        rec.after_step(a)
    rec.close()
    assert len(rec.files) >= 4
    ep = recorder.load_episode(sorted(rec.files)[0])
    T = ep["action"].shape[0]
    assert 1 <= T <= 3
    for cam in ("front", "top"):
        im = ep[f"observations/images/{cam}"]
        assert im.shape == (T, H, W, 3) and im.dtype == np.uint8 and im[-1].std() > 5
    sim.close()


def test_sized_frames_write_nowhere_else(hip_lib):
    """6. n = 67 at 36 x 52: the frame kernel reads poses and writes frames only -- state observations and step outputs after 5 seeded steps are bit-identical
    between observation_mode "state" and "both" (the same holds at the default size, checked here as well)"""
    from gym_lowcostrobot_amd import VecSim

    n = 67
    for size in (None, (36, 52)):
        sims = [VecSim("stack", n, observation_mode=m, base_seed=8, max_episode_steps=4, **({"image_size": size} if m == "both" else {})) for m in ("state", "both")]
        rng = np.random.default_rng(6)
        for _ in range(5):
            a = rng.uniform(-1, 1, (n, sims[0].action_dim)).astype(np.float32)
            for s_ in sims:
                s_.step(a)
        sa, sb = (s_.get_state() for s_ in sims)
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{size} state {k}")
        oa, ob = (s_.outputs() for s_ in sims)
        for k in oa:
            np.testing.assert_array_equal(oa[k], ob[k], err_msg=f"{size} output {k}")
        for k in ("arm_qpos", "arm_qvel", "cube_pos", "aux_pos", "terminal_obs", "terminal_quat"):
            np.testing.assert_array_equal(getattr(sims[0], k).numpy(), getattr(sims[1], k).numpy(), err_msg=f"{size} {k}")
        assert sims[1].image_front.numpy().std() > 5
        for s_ in sims:
            s_.close()
