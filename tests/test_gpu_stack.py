"""The observation stack on the GPU (VecSim(..., obs_stack=...); lcr_enable_obs_stack): the library's device buffer (N, K, C, H, W) against the numpy model of
tests/stack_ref.py, which is fed the library's own uint8 frames and flag bytes.  Everything is compared byte for byte; there is no tolerance in this feature.

Shapes: n = 1 and 5 leave most of the grid to one env (a workgroup never spans envs), 70 crosses a wave of the step kernel; 16 x 16 is the smallest legal frame (one partial
tile of 256 pixels), 36 x 52 is non-square with W no multiple of 16 (1872 pixels: one full tile of 1024 and a partial one of 848)."""
import ctypes

import numpy as np
import pytest

from tests import stack_ref

pytestmark = pytest.mark.gpu

STEPS = 8
QUEUED = (2, 3, 4)   # steps issued back to back with no read in between; with max_episode_steps = 3 step 2 auto-resets the envs (all that have not finished earlier)


def _frames(sim, cameras):
    return [getattr(sim, "image_" + c).numpy() for c in cameras]


def _cameras(sim):
    return sim.obs_stack_spec["cameras"]


def _same(sim, model, when):
    sp = sim.obs_stack_spec
    got = sim.obs_stack.numpy()
    want = model.expected(sp["dtype"], sp["reset_fill"])
    assert got.dtype == want.dtype and got.shape == want.shape, (when, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (when, len(bad), bad[:6].tolist())


def _check_guards(sim, when):
    from gym_lowcostrobot_amd import _capi
    from tests.test_gpu_wrist import _guards

    for side, g in zip(("before", "behind"), _guards(sim, sim.obs_stack)):
        assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (when, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())


def _recorded_rollout(task, n, kw, seed):
    """the seeded rollout on a handle WITHOUT a stack, read after every step: frames of every camera and did_reset per step, plus the initial frames"""
    from gym_lowcostrobot_amd import VecSim

    sim = VecSim(task, n, **kw)
    cams = ("front", "top") + (("wrist",) if sim.image_wrist is not None else ())
    act = sim.alloc_actions()
    rec = [dict(zip(cams, _frames(sim, cams)))]
    for t in range(STEPS):
        sim.fill_random_actions(act, seed, t); sim.step_device(act.ptr)
        rec.append(dict(zip(cams, _frames(sim, cams)), did_reset=sim.outputs()["did_reset"], state=sim.get_state(), reward=sim.outputs()["reward"]))
    sim.free(act); sim.close()
    return rec


ROLLOUTS = [  # task, n, size, K, dtype, fill
    ("push", 1, (16, 16), 1, "uint8", "repeat"),
    ("push", 5, (36, 52), 2, "float16", "zero"),
    ("push", 70, (16, 16), 4, "float32", "repeat"),
    ("push", 70, (36, 52), 2, "uint8", "zero"),
    ("stack", 70, (36, 52), 4, "uint8", "zero"),
    ("stack", 5, (16, 16), 2, "float32", "zero"),
    ("stack", 1, (36, 52), 4, "float16", "repeat"),
    ("stack", 5, (36, 52), 1, "float16", "repeat"),
]


@pytest.mark.parametrize("task,n,size,K,dtype,fill", ROLLOUTS, ids=[f"{r[0]}-n{r[1]}-{r[2][0]}x{r[2][1]}-K{r[3]}-{r[4]}-{r[5]}" for r in ROLLOUTS])
def test_rollout_against_the_model(hip_lib, task, n, size, K, dtype, fill):
    """1 (+ 5, 6).  Eight random steps with max_episode_steps = 3: every env crosses two auto-resets.  The stack is read after the step is issued; steps 2, 3, 4 are issued
    back to back with no read in between, so the stack of step 2 -- the one that refills every env -- is made on the second stream from the did_reset snapshot while the
    step kernels of steps 3 and 4 overwrite the flags.  The frames and flags the model is fed come from the same seeded rollout on a handle without a stack, whose frames,
    states and rewards the handle with the stack must reproduce exactly (nothing else moves).  Both guard regions are read back at the end."""
    from gym_lowcostrobot_amd import VecSim

    kw = dict(observation_mode="both", base_seed=21, max_episode_steps=3, image_size=size, wrist_camera=True if task == "stack" else None)
    rec = _recorded_rollout(task, n, kw, seed=13)
    resets = np.sum([r["did_reset"] for r in rec[1:]], axis=0)
    assert (resets >= 2).all() and rec[1 + QUEUED[0]]["did_reset"].any() and not all(r["did_reset"].all() for r in rec[1:])
    sim = VecSim(task, n, obs_stack=dict(frames=K, dtype=dtype, reset_fill=fill), **kw)
    cams = _cameras(sim)
    assert cams == (("front", "top", "wrist") if task == "stack" else ("front", "top"))
    assert sim.obs_stack.shape == (n, K, 3 * len(cams)) + size and sim.obs_stack.dtype == np.dtype(dtype)
    assert sim.obs_stack_spec == {"frames": K, "cameras": cams, "dtype": dtype, "reset_fill": fill}
    model = stack_ref.StackRef([rec[0][c] for c in cams], K)
    _same(sim, model, "enabled")
    _check_guards(sim, "enabled")
    act = [sim.alloc_actions() for _ in QUEUED]
    for t in range(STEPS):
        sim.fill_random_actions(act[t % len(act)], 13, t); sim.step_device(act[t % len(act)].ptr)
        model.step([rec[t + 1][c] for c in cams], rec[t + 1]["did_reset"])
        if t in QUEUED[:-1]:
            continue
        _same(sim, model, f"step {t}")
        # nothing else moves: frames, state and outputs of the handle with the stack are those of the handle without
        for c in cams:
            np.testing.assert_array_equal(getattr(sim, "image_" + c).numpy(), rec[t + 1][c], err_msg=f"image_{c}, step {t}")
        st = sim.get_state()
        for k, v in rec[t + 1]["state"].items():
            np.testing.assert_array_equal(st[k], v, err_msg=f"{k}, step {t}")
        np.testing.assert_array_equal(sim.outputs()["reward"], rec[t + 1]["reward"]); np.testing.assert_array_equal(sim.outputs()["did_reset"], rec[t + 1]["did_reset"])
    obs = sim.observations()
    assert [k for k in obs if k.startswith(("image_", "depth_", "segmentation_"))][-1] == "image_stack"   # behind the existing image keys
    np.testing.assert_array_equal(obs["image_stack"], sim.obs_stack.numpy())
    if K > 1 and fill == "repeat":   # the stack is not degenerate: a step after the last reset, slots differ
        s = sim.obs_stack.numpy()
        assert (s[:, -1] != s[:, 0]).any()
    _check_guards(sim, "after the rollout")
    for a in act:
        sim.free(a)
    sim.close()


@pytest.mark.parametrize("n,size,K,dtype,fill", [(70, (36, 52), 4, "float16", "zero"), (5, (16, 16), 2, "uint8", "repeat")], ids=["n70-36x52-K4-f16-zero", "n5-16x16-K2-u8-repeat"])
def test_invariant_and_the_entry_points_that_are_not_the_step(hip_lib, n, size, K, dtype, fill):
    """2 (+ 6).  After reset(mask) with a mixed mask, reset(mask = zeros) after set_state, set_look and reset(): slot K - 1 equals the current frames, masked envs are
    refilled, the older slots of the other envs are unchanged"""
    from gym_lowcostrobot_amd import VecSim

    sim = VecSim("push", n, observation_mode="both", base_seed=2, max_episode_steps=50, image_size=size, look_variants=[{}], obs_stack=dict(frames=K, dtype=dtype, reset_fill=fill))
    cams = _cameras(sim)
    model = stack_ref.StackRef(_frames(sim, cams), K)
    rng = np.random.default_rng(4)
    for t in range(K):   # K distinct frames in the stack
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
        model.step(_frames(sim, cams), sim.outputs()["did_reset"])
    _same(sim, model, "steps")

    def invariant(when, refilled):
        s, x = sim.obs_stack.numpy(), stack_ref.convert(stack_ref.channels_first(_frames(sim, cams)), dtype)
        np.testing.assert_array_equal(s[:, -1].view(np.uint8), x.view(np.uint8), err_msg=when)
        keep = ~np.asarray(refilled, bool)
        np.testing.assert_array_equal(s[keep, :-1].view(np.uint8), before[keep, :-1].view(np.uint8), err_msg=when)
        for e in np.nonzero(refilled)[0]:
            want = np.repeat(x[e][None], K - 1, 0) if fill == "repeat" else np.zeros_like(s[e, :-1])
            np.testing.assert_array_equal(s[e, :-1].view(np.uint8), want.view(np.uint8), err_msg=f"{when}, env {e}")
        _same(sim, model, when)

    before = sim.obs_stack.numpy()
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    sim.reset(mask=mask)
    model.reset(_frames(sim, cams), mask)
    invariant("reset(mask)", mask)
    assert (sim.obs_stack.numpy()[mask == 1, -1] != before[mask == 1, -1]).any()

    before = sim.obs_stack.numpy()
    st = sim.get_state()
    st["qpos"][:5] += rng.uniform(-0.3, 0.3, (5, n))
    sim.set_state(qpos=st["qpos"])
    sim.reset(mask=np.zeros(n, np.uint8))
    model.reset(_frames(sim, cams), np.zeros(n, np.uint8))
    invariant("reset(zeros) after set_state", np.zeros(n))
    assert (sim.obs_stack.numpy()[:, -1] != before[:, -1]).any()

    before = sim.obs_stack.numpy()
    sim.set_look(rgb=rng.uniform(0, 1, (9, n)).astype(np.float32))
    model.set_look(_frames(sim, cams))
    invariant("set_look", np.zeros(n))
    assert (sim.obs_stack.numpy()[:, -1] != before[:, -1]).any()

    before = sim.obs_stack.numpy()
    sim.reset()
    model.reset(_frames(sim, cams))
    invariant("reset()", np.ones(n))
    _check_guards(sim, "after the entry points")
    sim.close()


@pytest.mark.parametrize("cams", [("front",), ("wrist",), ("top", "wrist")], ids=lambda c: "+".join(c))
def test_camera_masks_and_the_life_cycle(hip_lib, cams):
    """3.  C and the channel order of a camera selection; the same spec again is a no-op, another spec, lcr_enable_wrist_camera and lcr_enable_look afterwards are refused"""
    from gym_lowcostrobot_amd import VecSim, _capi

    n, size, K = 5, (16, 16), 2
    sim = VecSim("stack", n, observation_mode="both", base_seed=6, max_episode_steps=3, image_size=size, wrist_camera=True, obs_stack=dict(frames=K, cameras=cams[::-1], dtype="uint8"))
    assert _cameras(sim) == cams and sim.obs_stack.shape == (n, K, 3 * len(cams)) + size
    model = stack_ref.StackRef(_frames(sim, cams), K)
    rng = np.random.default_rng(8)
    for t in range(4):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
        model.step(_frames(sim, cams), sim.outputs()["did_reset"])
        _same(sim, model, f"step {t}")
    s = sim.obs_stack.numpy()
    for i, c in enumerate(cams):   # camera i of the selection is channels 3 i .. 3 i + 2, as r, g, b
        np.testing.assert_array_equal(s[:, -1, 3 * i:3 * i + 3], np.moveaxis(getattr(sim, "image_" + c).numpy(), -1, 1))
    L = hip_lib
    sp = _capi.ObsStackSpec.from_any(dict(frames=K, cameras=cams, dtype="uint8"))
    before = sim.obs_stack.numpy()
    assert L.lcr_enable_obs_stack(sim.handle, ctypes.byref(sp)) == 0
    np.testing.assert_array_equal(sim.obs_stack.numpy(), before)
    for other in (dict(frames=K + 1, cameras=cams), dict(frames=K, cameras=cams, dtype="float16"), dict(frames=K, cameras=cams, reset_fill="zero"), dict(frames=K)):
        o = _capi.ObsStackSpec.from_any(other)
        assert L.lcr_enable_obs_stack(sim.handle, ctypes.byref(o)) == _capi.LCR_ERR_INVALID and b"fixed for the life" in L.lcr_last_error()
    sv = _capi.LcrObsStackView()
    assert L.lcr_get_obs_stack(sim.handle, ctypes.byref(sv)) == 0
    assert sv.enabled == 1 and sv.channels == 3 * len(cams) and (sv.image_height, sv.image_width) == size and sv.data == sim.obs_stack.ptr
    assert sv.bytes_per_env == K * 3 * len(cams) * size[0] * size[1] and sv.spec.cameras == sum(_capi.STACK_CAMERAS[c] for c in cams)
    w = _capi.WristCamera.from_any(True)
    assert L.lcr_enable_wrist_camera(sim.handle, ctypes.byref(_capi.WristCamera.from_any({"link": 4}))) == _capi.LCR_ERR_INVALID
    v = (_capi.LookVariant * 1)(_capi.LookVariant.from_any({}))
    assert L.lcr_enable_look(sim.handle, 1, v, None) == _capi.LCR_ERR_INVALID and b"observation stack" in L.lcr_last_error()
    assert L.lcr_enable_wrist_camera(sim.handle, ctypes.byref(w)) == 0   # (the same camera again: still the no-op it was)
    np.testing.assert_array_equal(sim.obs_stack.numpy(), before)
    sim.close()

    plain = VecSim("push", n, observation_mode="both", image_size=size)
    assert plain.obs_stack is None and plain.obs_stack_spec is None and "image_stack" not in plain.observations()
    assert L.lcr_get_obs_stack(plain.handle, ctypes.byref(sv)) == 0 and sv.enabled == 0 and not sv.data
    wr = _capi.ObsStackSpec.from_any(dict(frames=2, cameras=("front", "wrist")))
    assert L.lcr_enable_obs_stack(plain.handle, ctypes.byref(wr)) == _capi.LCR_ERR_INVALID and b"wrist" in L.lcr_last_error()
    assert L.lcr_enable_obs_stack(plain.handle, ctypes.byref(_capi.ObsStackSpec.from_any(2))) == 0       # enabled late, on a live handle
    assert L.lcr_get_obs_stack(plain.handle, ctypes.byref(sv)) == 0 and sv.enabled == 1 and sv.spec.cameras == 3 and sv.channels == 6
    assert L.lcr_enable_wrist_camera(plain.handle, ctypes.byref(w)) == _capi.LCR_ERR_INVALID and b"observation stack" in L.lcr_last_error()
    plain.close()
    state = VecSim("push", n, observation_mode="state")
    assert L.lcr_enable_obs_stack(state.handle, ctypes.byref(_capi.ObsStackSpec.from_any(2))) == _capi.LCR_ERR_INVALID and b"no image observations" in L.lcr_last_error()
    state.close()


def test_stack_on_the_second_stream_is_the_serial_stack(hip_lib, monkeypatch):
    """4.  The same seeded rollout with the frames and the stack on the caller's stream (LCR_RENDER_OVERLAP=0) and on the second stream: identical stacks after every burst"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 70, (36, 52)
    kw = dict(observation_mode="both", base_seed=3, max_episode_steps=3, image_size=size, wrist_camera=True, obs_stack=dict(frames=4, dtype="float16", reset_fill="zero"))
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("stack", n, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("stack", n, **kw)
    acts = [(s_, s_.alloc_actions()) for s_ in (ref, ovl)]
    np.testing.assert_array_equal(ref.obs_stack.numpy().view(np.uint16), ovl.obs_stack.numpy().view(np.uint16))
    t = 0
    for burst in (1, 1, 1, 1, 3, 2, 4):          # episodes end every 3 steps: auto-resets fall at the start, in the middle and at the end of bursts
        for _ in range(burst):
            for s_, a in acts:
                s_.fill_random_actions(a, 5, t); s_.step_device(a.ptr)
            t += 1
        np.testing.assert_array_equal(ref.obs_stack.numpy().view(np.uint16), ovl.obs_stack.numpy().view(np.uint16), err_msg=f"after step {t - 1}")
    s = ref.obs_stack.numpy()
    assert s.astype(np.float32).std() > 0.02 and s.max() <= 1.0
    for s_, a in acts:
        s_.free(a); s_.close()


def test_sharded_stack_is_the_unsharded_stack(hip_lib):
    """7.  Two shards of 64 envs on one GPU keep the stack of the unsharded 128-env handle"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = dict(observation_mode="both", base_seed=9, max_episode_steps=3, image_size=(16, 16), obs_stack=dict(frames=2, dtype="float32"))
    one = VecSim("push", 128, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], **kw)
    assert all(s_.obs_stack.shape == (64, 2, 6, 16, 16) and s_.obs_stack_spec == one.obs_stack_spec for s_ in sh.shards)
    act = one.alloc_actions()
    for t in range(5):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        got = np.concatenate([s_.obs_stack.numpy() for s_ in sh.shards])
        np.testing.assert_array_equal(got.view(np.uint32), one.obs_stack.numpy().view(np.uint32), err_msg=f"step {t}")
    assert one.obs_stack.numpy().std() > 0.02
    one.free(act); one.close(); sh.close()


def test_torch_view_of_the_stack(hip_lib):
    """sim.obs_stack.torch(): zero-copy, the chosen element type (float16 through __cuda_array_interface__), policy-ready by a plain reshape"""
    import torch

    from gym_lowcostrobot_amd import VecSim

    n, size, K = 5, (16, 16), 2
    sim = VecSim("push", n, observation_mode="both", image_size=size, obs_stack=dict(frames=K, dtype="float16"))
    sim.step(np.zeros((n, sim.action_dim), np.float32))
    sim.sync()
    t = sim.obs_stack.torch()
    assert t.dtype == torch.float16 and tuple(t.shape) == (n, K, 6) + size and t.is_contiguous() and t.data_ptr() == sim.obs_stack.ptr
    x = t.reshape(n, K * 6, *size)
    assert x.data_ptr() == t.data_ptr()
    np.testing.assert_array_equal(x.cpu().numpy().reshape(n, K, 6, *size).view(np.uint16), sim.obs_stack.numpy().view(np.uint16))
    del t, x
    sim.close()
