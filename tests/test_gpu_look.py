"""The look of the batched image observations: visual domain randomisation (VecSim(..., look_variants=[...], look_sampler={...}); lcr_enable_look / lcr_set_look /
lcr_get_look).  Definitions: include/lcr.h; tests/look_ref.py restates them in numpy.

Bounds -- the project's, imported from the tests that own them, none restated or widened:
  * against look_ref (fp64, per pixel): pixels beyond +-2 levels per frame <= test_gpu_image_size._oracle_pixels(H, W) = 0.001 * max(1, 320 / W) * W * H.
  * against the look-aware one-ray-per-pixel path of the same library (sim.render): <= test_gpu_image_size._raycast_pixels(H, W).
  * planes against look_ref: planes_ref.agree at 1e-4 relative depth, disagreeing pixels <= test_gpu_image_planes._ref_pixels(H, W).
  * the default variant without a sampler against a sim without a look, and everything called "identical": byte for byte.

Measured worst counts per frame (MI355X; the lines the tests print, kept in profiles/look.txt), next to the bound they stayed under -- the same for every task:
  looks vs look_ref             84 x 84: 2 (allowed 26.9)    120 x 160: 5 (allowed 38.4)
  terminal looks vs look_ref    84 x 84: 2 (allowed 26.9)
  batched vs per-pixel path     84 x 84: 2 (allowed 5.4)     120 x 160: 7 (allowed 7.7) at n = 24 and 25, 0 at n = 1.  The seven are the same in all three tasks, so they belong
                                to a background, not to a cube or marker; they have not been located pixel by pixel (the suspects are the rows along the horizon of a rolled
                                camera_front, the situation described in tests/test_gpu_image_size.py).  A culled primitive would show as tens
  planes vs look_ref            84 x 84: 0 disagreeing pixels (allowed 26.9)
"""
import ctypes

import numpy as np
import pytest

from tests import look_ref, planes_ref
from tests.test_gpu_image_planes import _ref_pixels
from tests.test_gpu_image_size import _oracle_pixels, _random_poses, _raycast_pixels, _terminal_qpos
from tests.test_look_abi import gpu_test_colours

pytestmark = pytest.mark.gpu

CAMS = (("camera_front", "image_front"), ("camera_top", "image_top"))
BOTH = ("depth", "segmentation")
_ids = lambda s: f"{s[0]}x{s[1]}"   # noqa: E731
SAMPLER = {"seed": 77, "cube": ([0.2, 0.0, 0.0], [1.0, 0.6, 0.3]), "cube2": ([0.0, 0.1, 0.3], [0.4, 0.9, 1.0]), "marker": ([0.0, 0.5, 0.2], [0.3, 0.5, 1.0])}
SAMPLER_LO = np.array(SAMPLER["cube"][0] + SAMPLER["cube2"][0] + SAMPLER["marker"][0], np.float32)
SAMPLER_HI = np.array(SAMPLER["cube"][1] + SAMPLER["cube2"][1] + SAMPLER["marker"][1], np.float32)


def _frames(sim):
    return {k: getattr(sim, k).numpy() for k in ("image_front", "image_top")}


@pytest.mark.parametrize("size", [(84, 84), (36, 52), (120, 160), (240, 320)], ids=_ids)
@pytest.mark.parametrize("n", [24, 25])
@pytest.mark.parametrize("task", ["push", "stack"])
def test_default_variant_draws_the_bytes_of_a_sim_without_a_look(hip_lib, task, n, size):
    """1. identity: one default variant, no sampler, against a sim without a look after 5 random steps"""
    from gym_lowcostrobot_amd import VecSim, default_look_variant

    kw = dict(observation_mode="both", base_seed=2, image_size=size)
    sims = [VecSim(task, n, **kw), VecSim(task, n, look_variants=[default_look_variant()], **kw)]
    for k, a in _frames(sims[0]).items():
        np.testing.assert_array_equal(_frames(sims[1])[k], a, err_msg=f"after lcr_enable_look, {k}")
    rng = np.random.default_rng(3)
    for _ in range(5):
        a = rng.uniform(-1, 1, (n, sims[0].action_dim)).astype(np.float32)
        for s_ in sims:
            s_.step(a)
    fa, fb = (_frames(s_) for s_ in sims)
    for k in fa:
        np.testing.assert_array_equal(fb[k], fa[k], err_msg=k)
        assert fa[k].std() > 5
    for cam, _ in CAMS:   # the look-aware per-pixel path as well
        np.testing.assert_array_equal(sims[1].render(n - 1, cam, size[1], size[0]), sims[0].render(n - 1, cam, size[1], size[0]), err_msg=cam)
    np.testing.assert_array_equal(sims[1].render(0, "camera_vizu", 96, 64), sims[0].render(0, "camera_vizu", 96, 64))
    lk = sims[1].look()
    assert (lk["variant"] == 0).all() and (lk["episode"] == 0).all()
    np.testing.assert_array_equal(lk["rgb"], np.repeat(np.array(look_ref.TASK_RGB, np.float32)[:, None], n, 1))
    for s_ in sims:
        s_.close()


@pytest.mark.parametrize("task", ["push", "stack"])
def test_default_variant_with_planes_draws_the_same_bytes(hip_lib, task):
    """1b. identity with planes on, 84 x 84, n = 25: colours and planes"""
    from gym_lowcostrobot_amd import VecSim

    n = 25
    kw = dict(observation_mode="both", base_seed=2, image_size=(84, 84), image_planes=BOTH, max_episode_steps=3)
    sims = [VecSim(task, n, **kw), VecSim(task, n, look_variants=[{}], **kw)]
    rng = np.random.default_rng(3)
    for _ in range(5):
        a = rng.uniform(-1, 1, (n, sims[0].action_dim)).astype(np.float32)
        for s_ in sims:
            s_.step(a)
    oa, ob = (s_.observations() for s_ in sims)
    assert list(oa) == list(ob)
    for k in oa:
        np.testing.assert_array_equal(ob[k], oa[k], err_msg=k)
    fin = np.nonzero(sims[0].outputs()["did_reset"])[0].astype(np.int32)
    if fin.size:
        for a, b in zip(sims[0].render_terminal(fin), sims[1].render_terminal(fin)):
            np.testing.assert_array_equal(b, a)
        ta, tb = sims[0].render_terminal_planes(fin), sims[1].render_terminal_planes(fin)
        for k in ta:
            np.testing.assert_array_equal(tb[k], ta[k], err_msg=k)
    for s_ in sims:
        s_.close()


@pytest.mark.parametrize("size", [(84, 84), (120, 160)], ids=_ids)
@pytest.mark.parametrize("task", ["push", "stack", "pick_place"])
def test_looks_vs_the_fp64_reference(hip_lib, task, size):
    """2. K = 4 variants that use every field, 8 random poses (seed 17) with explicit per-env colours set by set_look, both cameras; envs 8 and 9 repeat the pose of env 0
    under two other variants: same pose, different variant, different frames -- down to the bands no primitive touches"""
    from gym_lowcostrobot_amd import VecSim

    H, W = size
    n = 10
    sim = VecSim(task, n, observation_mode="both", auto_reset=False, image_size=size, look_variants=look_ref.GPU_VARIANTS)
    qpos, target = _random_poses(task, n, np.random.default_rng(17), sim.get_state())
    qpos[:, 8:] = qpos[:, :1]; target[:, 8:] = target[:, :1]
    variant = (np.arange(n) % 4).astype(np.int32)
    variant[8:] = (1, 2)
    rgb = np.concatenate([gpu_test_colours(8), gpu_test_colours(8)[:, :2]], 1)
    sim.set_state(qpos=qpos, target=target)
    sim.set_look(variant=variant, rgb=rgb)            # redraws the frames from the new state
    lk = sim.look()
    np.testing.assert_array_equal(lk["variant"], variant); np.testing.assert_array_equal(lk["rgb"], rgb)
    obs = sim.observations()
    worst, fails = 0, []
    for e in range(n):
        v = look_ref.GPU_VARIANTS[variant[e]]
        for cam, key in CAMS:
            ref = look_ref.render(task, qpos[:, e], target[:, e], cam, W, H, v=v, rgb=rgb[:, e]).astype(int)
            d = np.abs(obs[key][e].astype(int) - ref).max(-1)
            bad = int((d > 2).sum())
            worst = max(worst, bad)
            if bad > _oracle_pixels(H, W):
                fails.append((e, cam, bad, np.argwhere(d > 2)[:5].tolist()))
    print(f"[looks vs fp64 reference] {task} {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_oracle_pixels(H, W):.1f})")
    assert not fails, (task, size, fails)
    for key in ("image_front", "image_top"):
        for e in (8, 9):
            diff = np.abs(obs[key][e].astype(int) - obs[key][0].astype(int)).max(-1) > 2
            assert diff.mean() > 0.5, (key, e, diff.mean())
    # out-of-range values are refused and leave the looks as they are
    with pytest.raises(ValueError, match="variant"):
        sim.set_look(variant=np.full(n, 4, np.int32))
    with pytest.raises(ValueError, match="rgb"):
        sim.set_look(rgb=np.full((9, n), 1.5, np.float32))
    np.testing.assert_array_equal(sim.look()["variant"], variant)
    sim.close()


@pytest.mark.parametrize("size", [(84, 84), (120, 160)], ids=_ids)
@pytest.mark.parametrize("n", [24, 25, 1])
@pytest.mark.parametrize("task", ["push", "stack", "pick_place"])
def test_culling_under_moved_cameras(hip_lib, task, n, size):
    """3. batched frames against the look-aware per-pixel sim.render of the same env and camera after 15 random steps, variants and colours drawn by the sampler;
    a silhouette built from the wrong camera shows as tens of pixels"""
    from gym_lowcostrobot_amd import VecSim

    H, W = size
    sim = VecSim(task, n, observation_mode="both", base_seed=11, image_size=size, look_variants=look_ref.GPU_VARIANTS, look_sampler=SAMPLER)
    rng = np.random.default_rng(5)
    for _ in range(15):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
    obs = sim.observations()
    if n > 1:
        assert len(set(sim.look()["variant"].tolist())) == 4
    worst, fails = 0, []
    for e in range(n):
        for name, key in CAMS:
            ref = sim.render(e, name, W, H).astype(int)
            d = np.abs(obs[key][e].astype(int) - ref).max(-1)
            bad = int((d > 2).sum())
            worst = max(worst, bad)
            if bad > _raycast_pixels(H, W):
                fails.append((e, name, bad, np.argwhere(d > 2)[:5].tolist()))
    print(f"[look tile path] {task} n={n} {H}x{W}: worst {worst} pixels beyond +-2 levels (allowed {_raycast_pixels(H, W):.1f})")
    sim.close()
    assert not fails, (task, n, size, fails)


def _run_episodes(task, n, steps, size, offset=0, global_envs=None, look=True, record=None):
    from gym_lowcostrobot_amd import VecSim

    kw = dict(observation_mode="both", base_seed=4, max_episode_steps=3, image_size=size, env_id_offset=offset, global_envs=global_envs)
    if look:
        kw.update(look_variants=look_ref.GPU_VARIANTS, look_sampler=SAMPLER)
    sim = VecSim(task, n, **kw)
    act = sim.alloc_actions()
    hist = []
    for t in range(steps):
        before = sim.look() if look else None
        sim.fill_random_actions(act, 9, t); sim.step_device(act.ptr)
        out = sim.outputs()
        rec = {"out": out, "state": sim.get_state(), "frames": _frames(sim), "before": before, "look": sim.look() if look else None}
        if record is not None:
            record(sim, t, rec)
        hist.append(rec)
    sim.free(act); sim.close()
    return hist


@pytest.mark.parametrize("task", ["push", "stack"])
def test_looks_are_redrawn_exactly_where_envs_reset(hip_lib, task):
    """4. max_episode_steps = 3, n = 128, 7 steps with a sampler"""
    H, W = size = (84, 84)
    n = 128
    worst = [0]

    def record(sim, t, rec):   # the terminal frames of (some of) the envs this step finished: the episode as it looked, i.e. with the look recorded before the step
        fin = np.nonzero(rec["out"]["did_reset"])[0]
        if fin.size == 0:
            return
        ids = fin[:4].astype(np.int32)
        fr, tp = sim.render_terminal(ids)
        tob, tq = sim.terminal_obs.numpy(), sim.terminal_quat.numpy()
        for j, e in enumerate(ids.tolist()):
            qpos, tgt = _terminal_qpos(sim, tob, tq, e)
            v = look_ref.GPU_VARIANTS[rec["before"]["variant"][e]]
            for got, cam in ((fr[j], "camera_front"), (tp[j], "camera_top")):
                ref = look_ref.render(task, qpos, tgt, cam, W, H, v=v, rgb=rec["before"]["rgb"][:, e]).astype(int)
                bad = int((np.abs(ref - got.astype(int)).max(-1) > 2).sum())
                worst[0] = max(worst[0], bad)
                assert bad <= _oracle_pixels(H, W), (task, t, e, cam, bad)

    whole = _run_episodes(task, n, 7, size, record=record)
    print(f"[terminal looks vs fp64 reference] {task} {H}x{W}: worst {worst[0]} pixels beyond +-2 levels (allowed {_oracle_pixels(H, W):.1f})")
    resets = np.zeros(n, np.int64)
    for t, rec in enumerate(whole):
        dr = rec["out"]["did_reset"]
        resets += dr
        b, a = rec["before"], rec["look"]
        changed = (b["variant"] != a["variant"]) | (b["rgb"] != a["rgb"]).any(0)
        np.testing.assert_array_equal(changed, dr, err_msg=f"step {t}: the look changes exactly where did_reset is set")
        np.testing.assert_array_equal(a["episode"], resets, err_msg=f"step {t}")
        assert (a["variant"] >= 0).all() and (a["variant"] < 4).all()
        assert (a["rgb"] >= SAMPLER_LO[:, None]).all() and (a["rgb"] <= SAMPLER_HI[:, None]).all()
        assert (a["rgb"][7] == 0.5).all()   # lo == hi pins a channel
    assert resets.min() >= 2
    # the sampler is the generator written down in include/lcr.h
    last = whole[-1]["look"]
    for e in (0, 1, 63, 64, 127):
        var, rgb = look_ref.sample(SAMPLER["seed"], e, int(last["episode"][e]), 4, SAMPLER_LO, SAMPLER_HI)
        assert var == last["variant"][e], e
        np.testing.assert_array_equal(rgb, last["rgb"][:, e], err_msg=f"env {e}")
    # state, reward and flags: bit-identical to a sim without a look
    plain = _run_episodes(task, n, 7, size, look=False)
    for t, (ra, rb) in enumerate(zip(whole, plain)):
        for k in ra["out"]:
            np.testing.assert_array_equal(ra["out"][k], rb["out"][k], err_msg=f"step {t} {k}")
        for k in ra["state"]:
            np.testing.assert_array_equal(ra["state"][k], rb["state"][k], err_msg=f"step {t} state {k}")
    assert any((ra["frames"]["image_front"] != rb["frames"]["image_front"]).any() for ra, rb in zip(whole, plain))
    # two runs are identical; two shards of 64 with global_envs = 128 equal the whole, in looks and in frame bytes
    again = _run_episodes(task, n, 7, size)
    shards = [_run_episodes(task, 64, 7, size, offset=off, global_envs=128) for off in (0, 64)]
    for t in range(7):
        for k in ("variant", "rgb", "episode"):
            np.testing.assert_array_equal(again[t]["look"][k], whole[t]["look"][k], err_msg=f"second run, step {t} {k}")
            np.testing.assert_array_equal(np.concatenate([s_[t]["look"][k] for s_ in shards], -1), whole[t]["look"][k], err_msg=f"shards, step {t} {k}")
        for k in ("image_front", "image_top"):
            np.testing.assert_array_equal(again[t]["frames"][k], whole[t]["frames"][k], err_msg=f"second run, step {t} {k}")
            np.testing.assert_array_equal(np.concatenate([s_[t]["frames"][k] for s_ in shards]), whole[t]["frames"][k], err_msg=f"shards, step {t} {k}")


def test_explicit_resets_count_episodes_and_redraw(hip_lib):
    """4b. lcr_reset, masked or not, raises the episode count of the envs it resets and redraws their looks; a masked no-op reset touches nothing"""
    from gym_lowcostrobot_amd import VecSim

    n = 70
    sim = VecSim("push", n, observation_mode="image", image_size=(36, 52), look_variants=look_ref.GPU_VARIANTS, look_sampler=SAMPLER)
    l0 = sim.look()
    assert (l0["episode"] == 0).all() and len(set(l0["variant"].tolist())) == 4
    for e in (0, 69):
        var, rgb = look_ref.sample(SAMPLER["seed"], e, 0, 4, SAMPLER_LO, SAMPLER_HI)
        assert var == l0["variant"][e]; np.testing.assert_array_equal(rgb, l0["rgb"][:, e])
    sim.reset(mask=np.zeros(n, np.uint8))
    l1 = sim.look()
    for k in ("variant", "rgb", "episode"):
        np.testing.assert_array_equal(l1[k], l0[k])
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    sim.reset(mask=mask)
    l2 = sim.look()
    np.testing.assert_array_equal(l2["episode"], mask)
    np.testing.assert_array_equal((l2["rgb"] != l0["rgb"]).any(0), mask.astype(bool))
    sim.reset(seeds=np.arange(n, dtype=np.uint64))
    np.testing.assert_array_equal(sim.look()["episode"], mask.astype(np.uint32) + 1)
    # look() / set_look() are the checkpoint of the look: restoring the first looks restores the first frames
    f2 = _frames(sim)
    keep = sim.look()
    sim.set_look(variant=l0["variant"], rgb=l0["rgb"])
    assert (_frames(sim)["image_front"] != f2["image_front"]).any()
    sim.set_look(variant=keep["variant"], rgb=keep["rgb"], mask=np.ones(n, np.uint8))
    for k, a in _frames(sim).items():
        np.testing.assert_array_equal(a, f2[k], err_msg=k)
    sim.close()


def test_looks_on_the_second_stream_are_the_serial_looks(hip_lib, monkeypatch):
    """5. episodes of 3 steps in bursts of asynchronous steps: frames ray-cast on the second stream from a snapshot (default) and on the caller's stream after each step
    kernel (LCR_RENDER_OVERLAP=0) are byte-identical -- the snapshot covers the looks"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 192, (84, 84)
    kw = dict(observation_mode="both", base_seed=3, max_episode_steps=3, image_size=size, look_variants=look_ref.GPU_VARIANTS, look_sampler=SAMPLER)
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", n, **kw)
    acts = [(s_, s_.alloc_actions()) for s_ in (ref, ovl)]

    def same():
        for k in ("image_front", "image_top"):
            np.testing.assert_array_equal(getattr(ref, k).numpy(), getattr(ovl, k).numpy(), err_msg=k)
        la, lb = ref.look(), ovl.look()
        for k in ("variant", "rgb", "episode"):
            np.testing.assert_array_equal(la[k], lb[k], err_msg=k)

    same()
    t = 0
    for burst in (1, 1, 1, 2, 3, 4, 5, 7, 9, 12):      # episodes end every 3 steps: the bursts end before, at and after a step that redraws looks
        for _ in range(burst):
            for s_, a in acts:
                s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
            t += 1
        same()
    assert ref.look()["episode"].min() >= 10
    for s_, a in acts:
        s_.free(a); s_.close()


@pytest.mark.parametrize("task", ["push", "stack"])
def test_planes_through_moved_cameras(hip_lib, task):
    """6. depth and segmentation agree with look_ref under the rule of tests/test_gpu_image_planes.py; two sims that differ only in colours and light have identical
    planes; enabling the planes before the look is refused"""
    from gym_lowcostrobot_amd import VecSim, _capi

    H, W = size = (84, 84)
    n = 8
    kw = dict(observation_mode="both", auto_reset=False, image_size=size, image_planes=BOTH, depth_far=10.0)
    sim = VecSim(task, n, look_variants=look_ref.GPU_VARIANTS, **kw)
    recoloured = [dict(v, floor_rgb=v["floor_rgb"][::-1], sky_rgb=[0.9, 0.1, 0.2], ambient=0.1, diffuse=1.2, arm_rgb=[0.1, 0.9, 0.1]) for v in look_ref.GPU_VARIANTS]
    other = VecSim(task, n, look_variants=recoloured, **kw)
    qpos, target = _random_poses(task, n, np.random.default_rng(17), sim.get_state())
    variant = (np.arange(n) % 4).astype(np.int32)
    for s_, rgb in ((sim, gpu_test_colours(n)), (other, gpu_test_colours(n)[::-1].copy())):
        s_.set_state(qpos=qpos, target=target)
        s_.set_look(variant=variant, rgb=rgb)
    pa, pb = sim.plane_arrays(), other.plane_arrays()
    obs = {k: a.numpy() for k, a in pa.items()}
    for k in obs:
        np.testing.assert_array_equal(pb[k].numpy(), obs[k], err_msg=k)
    assert (sim.image_front.numpy() != other.image_front.numpy()).any()
    worst, fails = 0, []
    for e in range(n):
        for cam, c in (("camera_front", "front"), ("camera_top", "top")):
            dref, sref = look_ref.planes(task, qpos[:, e], target[:, e], cam, W, H, v=look_ref.GPU_VARIANTS[variant[e]], depth_far=10.0)
            ok = planes_ref.agree(obs[f"depth_{c}"][e], obs[f"segmentation_{c}"][e], dref, sref, 1e-4)
            bad = int((~ok).sum())
            worst = max(worst, bad)
            if bad > _ref_pixels(H, W):
                fails.append((e, cam, bad, np.argwhere(~ok)[:5].tolist()))
            # the look-aware per-pixel planes look through the same camera
            d1, s1 = sim.render_planes(e, cam, W, H)
            assert int((~planes_ref.agree(obs[f"depth_{c}"][e], obs[f"segmentation_{c}"][e], d1, s1, 1e-5)).sum()) <= _raycast_pixels(H, W), (e, cam)
    print(f"[look planes vs fp64 reference] {task} {H}x{W}: worst {worst} disagreeing pixels per frame (allowed {_ref_pixels(H, W):.1f})")
    assert not fails, (task, fails)
    sim.close(); other.close()

    late = VecSim(task, 4, observation_mode="both", image_size=size, image_planes=("depth",))
    arr = (_capi.LookVariant * 1)(_capi.LookVariant.from_any({}))
    assert hip_lib.lcr_enable_look(late.handle, 1, arr, None) == _capi.LCR_ERR_INVALID
    assert b"planes" in hip_lib.lcr_last_error(), hip_lib.lcr_last_error()
    late.close()


def test_enable_refusals_on_a_live_handle(hip_lib):
    """7. a handle without image observations, a camera pushed to less than 5 cm above the floor and a second call with other arguments are refused; the same arguments
    again do nothing; a handle without a look refuses lcr_get_look / lcr_set_look"""
    from gym_lowcostrobot_amd import VecSim, _capi

    one = (_capi.LookVariant * 1)(_capi.LookVariant.from_any({}))
    st = VecSim("reach", 4, observation_mode="state")
    assert hip_lib.lcr_enable_look(st.handle, 1, one, None) == _capi.LCR_ERR_INVALID and b"observation_mode" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_get_look(st.handle, None, None, None) == _capi.LCR_ERR_INVALID and b"lcr_enable_look" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_set_look(st.handle, None, None, None) == _capi.LCR_ERR_INVALID
    with pytest.raises(ValueError):
        st.look()
    st.close()
    with pytest.raises(ValueError, match="above the floor"):
        VecSim("reach", 4, observation_mode="image", image_size=(36, 52), look_variants=[{"cam_dpos": [[0.0, 0.0, -0.19], [0.0, 0.0, 0.0]]}])   # camera_front: 0.225 - 0.19
    sim = VecSim("reach", 4, observation_mode="image", image_size=(36, 52), look_variants=[{"cam_dpos": [[0.0, 0.0, -0.17], [0.0, 0.0, -0.2]]}], look_sampler={"seed": 5})
    before = _frames(sim)
    arr = (_capi.LookVariant * 1)(sim.look_variants[0])
    assert hip_lib.lcr_enable_look(sim.handle, 1, arr, ctypes.byref(sim.look_sampler)) == 0
    assert hip_lib.lcr_enable_look(sim.handle, 1, arr, None) == _capi.LCR_ERR_INVALID and b"fixed for the life of the handle" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_enable_look(sim.handle, 1, one, ctypes.byref(sim.look_sampler)) == _capi.LCR_ERR_INVALID
    for k, a in _frames(sim).items():
        np.testing.assert_array_equal(a, before[k])
    sim.close()


def test_the_look_reaches_the_sim_through_the_adapters(hip_lib):
    """8. look_variants / look_sampler through LowCostRobotVecEnv, LowCostRobotVectorEnv and ShardedVecSim; set_look / look round-trip"""
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, LowCostRobotVectorEnv, default_look_variant
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = dict(observation_mode="both", max_episode_steps=3, image_size=(36, 52), look_variants=look_ref.GPU_VARIANTS, look_sampler=SAMPLER)
    v = LowCostRobotVecEnv("push", 12, seed=5, **kw)
    g = LowCostRobotVectorEnv("push", 12, seed=5, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], **kw)
    lv, lg, ls = v.sim.look(), g._v.sim.look(), sh.look()
    assert len(lv["variants"]) == 4 and bytes(lv["variants"][1]) != bytes(default_look_variant())
    for k in ("variant", "rgb", "episode"):
        np.testing.assert_array_equal(lv[k], lg[k], err_msg=k)
        np.testing.assert_array_equal(ls[k][..., :12], lv[k], err_msg=k)      # (keyed by the global env id, whatever the shard)
    assert ls["variant"].shape == (128,) and ls["rgb"].shape == (9, 128) and len(set(ls["variant"].tolist())) == 4
    obs = v.reset()
    rng = np.random.default_rng(1)
    for _ in range(3):
        obs, rew, dones, infos = v.step(rng.uniform(-1, 1, (12, v.action_space.shape[0])).astype(np.float32))
    assert dones.any() and (v.sim.look()["episode"] >= 1).all()
    assert infos[int(np.nonzero(dones)[0][0])]["terminal_observation"]["image_front"].shape == (36, 52, 3)
    new_variant = ((lv["variant"] + 1) % 4).astype(np.int32)
    new_rgb = np.full((9, 12), 0.25, np.float32)
    mask = (np.arange(12) < 6).astype(np.uint8)
    cur = v.sim.look()
    v.sim.set_look(variant=new_variant, rgb=new_rgb, mask=mask)
    got = v.sim.look()
    np.testing.assert_array_equal(got["variant"], np.where(mask, new_variant, cur["variant"]))
    np.testing.assert_array_equal(got["rgb"], np.where(mask, new_rgb, cur["rgb"]))
    np.testing.assert_array_equal(got["episode"], cur["episode"])
    v.close(); g.close(); sh.close()
