"""The depth channel of the observation stack on the GPU (VecSim(obs_stack=dict(..., planes=("depth",))); lcr_enable_obs_stack_planes): RGB-D stacks, bit for bit.

Definition: include/lcr.h, "The depth channel of the observation stack"; tests/stack_depth_ref.py restates it in numpy -- the colour model of tests/stack_ref.py beside a
stack of the raw depths, and the element rule, which tests/test_stack_depth_abi.py holds against exact rational arithmetic.  The model is fed the library's own frames,
depth planes and did_reset after every call.  Everything is compared byte for byte: there is no tolerance in this feature.

Shapes: 16 x 16 is one partial tile of the stack kernel (256 pixels), 32 x 36 a full tile of 1 024 pixels and a last tile of 128; 6 to 12 envs.  Episode ends are staggered
with set_state(elapsed = 49 - e % 7), so that envs reset on different steps.  depth_far: the top camera looks down on a floor 0.6 m below it, so only a depth_far below that
puts pixels of every camera on both sides of the clamp -- 0.5 m wherever the top camera is stacked (the saturated branch of all three rules then holds the floor, not only
the sky); the front camera alone also runs at 10 m, where the sky saturates."""
import ctypes

import numpy as np
import pytest

from tests import stack_depth_ref as ref

pytestmark = pytest.mark.gpu

ALL = ("front", "top", "wrist")
SMALL, TAIL = (16, 16), (32, 36)


def _kw(size, cams, look=False, far=0.5, planes=("depth",), **more):
    from tests import look_ref

    kw = dict(observation_mode="both", image_size=size, base_seed=11, wrist_camera=True if "wrist" in cams else None, image_planes=planes, depth_far=far, **more)
    if look:
        kw.update(look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 5, "cube": ([0.2, 0, 0], [1, 0.4, 0.4])})
    return kw


def _frames(sim, cams):
    return [getattr(sim, "image_" + c).numpy() for c in cams]


def _depths(sim, cams):
    return [getattr(sim, "depth_" + c).numpy() for c in cams]


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (what, len(bad), bad[:6].tolist())


def _both_sides(sim, cams, what):
    """every selected camera's depth plane holds pixels at depth_far and pixels below it: both branches of the clamp run"""
    far = np.float32(sim.depth_far)
    for c, d in zip(cams, _depths(sim, cams)):
        assert (d == far).any() and (d < far).any() and d.max() <= far and d.min() >= 0, (what, c, float(d.min()), float(d.max()), float(far))


def _stagger(sim, order):
    sim.set_state(elapsed=(49 - order).astype(np.int32))


def _terminal_rgbd(sim, ids, cams, dtype):
    """the terminal frames and terminal depth planes of the listed envs by the existing calls, through the element rule -> (len(ids), 4 ncam, H, W)"""
    front, top = sim.render_terminal(ids)
    fr, dp = {"front": front, "top": top}, dict(sim.render_terminal_planes(ids))
    if "wrist" in cams:
        w = sim.render_terminal_wrist(ids)
        fr["wrist"], dp["depth_wrist"] = w["image_wrist"], w["depth_wrist"]
    return ref.rgbd_elements([fr[c] for c in cams], [dp["depth_" + c] for c in cams], dtype, sim.depth_far)


def _guards_intact(sim, arr, what):
    from gym_lowcostrobot_amd import _capi
    from tests.test_gpu_wrist import _guards

    for g in _guards(sim, arr):
        assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), what


# ---- 5.  every build, live ----

def _shape_of(dtype, K, cams, fill):
    """(task, size, envs, depth_far) of a case: K = 3 runs the frame with a full tile and a last tile of 128 pixels, one K = 8 case StackTwoCubes; the front camera alone
    sees the sky, so it also runs at 10 m (repeat) -- every other case at 0.5 m, where the floor under the top camera saturates"""
    task = "stack" if (dtype, K, cams, fill) == ("float16", 8, ALL, "zero") else "reach"
    far = 10.0 if cams == ("front",) and fill == "repeat" else 0.5
    return task, (TAIL if K == 3 else SMALL), {1: 6, 3: 8, 8: 12}[K], far


@pytest.mark.parametrize("fill", ref.FILLS)
@pytest.mark.parametrize("cams", [("front",), ("top",), ALL], ids="+".join)
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_every_build_live(hip_lib, dtype, K, cams, fill):
    """5.  dtype x K x cameras x reset_fill over 2 K + 1 steps with staggered resets: after enabling and after every step the stack is the model's, fed that step's frames,
    depth planes and did_reset"""
    from gym_lowcostrobot_amd import VecSim

    task, size, n, far = _shape_of(dtype, K, cams, fill)
    sim = VecSim(task, n, obs_stack=dict(frames=K, dtype=dtype, reset_fill=fill, cameras=cams, planes=("depth",)), **_kw(size, cams, far=far))
    assert sim.obs_stack_planes == ("depth",) and sim.obs_stack_spec == {"frames": K, "cameras": cams, "dtype": dtype, "reset_fill": fill}
    inv_far, s255 = ref.constants(sim.depth_far)
    assert sim.obs_stack_depth_scale == {"inv_far": float(inv_far), "s255": float(s255)}
    assert sim.obs_stack.shape == (n, K, 4 * len(cams)) + size and sim.obs_stack.dtype == np.dtype(dtype)
    assert sim.observations()["image_stack"].shape == sim.obs_stack.shape
    model = ref.StackDepthRef(_frames(sim, cams), _depths(sim, cams), K, sim.depth_far)
    _both_sides(sim, cams, "enabling")
    _same_bytes(sim.obs_stack.numpy(), model.expected(dtype, fill), "enabling")
    _stagger(sim, np.arange(n) % 7)
    act = sim.alloc_actions()
    reset_steps, pushed = set(), 0
    for t in range(2 * K + 1):
        sim.fill_random_actions(act, 3, t); sim.step_device(act.ptr)
        dres = sim.outputs()["did_reset"]
        model.step(_frames(sim, cams), _depths(sim, cams), dres)
        _both_sides(sim, cams, f"step {t}")
        _same_bytes(sim.obs_stack.numpy(), model.expected(dtype, fill), f"step {t}")
        if dres.any():
            reset_steps.add(t)
        pushed += int((~dres).sum())
    assert len(reset_steps) >= min(3, 2 * K + 1) and pushed > 0, reset_steps   # envs reset on different steps, and others were pushed
    _guards_intact(sim, sim.obs_stack, "the stack's guards")
    sim.free(act); sim.close()


# ---- 6.  the colour channels are the colour stack's ----

@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_colour_channels_are_those_of_a_twin_without_planes(hip_lib, dtype):
    """6.  channels r g b of every camera equal the stack of a twin handle enabled without planes=, bit for bit, over a rollout with resets"""
    from gym_lowcostrobot_amd import VecSim

    n, K, cams = 8, 3, ALL
    stack = dict(frames=K, dtype=dtype, reset_fill="zero", cameras=cams)
    rgbd = VecSim("reach", n, obs_stack=dict(stack, planes=("depth",)), **_kw(TAIL, cams))
    rgb = VecSim("reach", n, obs_stack=stack, **_kw(TAIL, cams))
    assert rgb.obs_stack_planes == () and rgb.obs_stack_depth_scale is None and rgb.obs_stack.shape == (n, K, 9) + TAIL
    acts = [(s, s.alloc_actions()) for s in (rgbd, rgb)]
    for s, _ in acts:
        _stagger(s, np.arange(n) % 7)
    colour = np.array([4 * c + k for c in range(3) for k in range(3)])
    for t in range(2 * K + 1):
        for s, a in acts:
            s.fill_random_actions(a, 3, t); s.step_device(a.ptr)
        _same_bytes(np.ascontiguousarray(rgbd.obs_stack.numpy()[:, :, colour]), rgb.obs_stack.numpy(), f"step {t}")
    for s, a in acts:
        s.free(a); s.close()


# ---- 7.  reset, redraw, set_look ----

def test_reset_redraw_and_set_look_keep_the_newest_slot_current(hip_lib):
    """7.  lcr_reset with a mask refills the masked envs, the all-zero-mask redraw after set_state and set_look rewrite slot K - 1 -- the depth channel included -- and
    the unmasked envs keep their older slots"""
    from gym_lowcostrobot_amd import VecSim

    n, K, cams, dtype = 9, 4, ("front", "top"), "float16"
    sim = VecSim("reach", n, obs_stack=dict(frames=K, dtype=dtype, reset_fill="repeat", cameras=cams, planes=("depth",)), **_kw(TAIL, cams, look=True))
    model = ref.StackDepthRef(_frames(sim, cams), _depths(sim, cams), K, sim.depth_far)
    rng = np.random.default_rng(0)
    e = np.arange(n)
    depth = np.array([4 * c + 3 for c in range(len(cams))])

    def check(what):
        got = sim.obs_stack.numpy()
        _same_bytes(got, model.expected(dtype, "repeat"), what)
        _same_bytes(np.ascontiguousarray(got[:, -1][:, depth]), ref.depth_elements(np.stack(_depths(sim, cams), axis=1), dtype, sim.depth_far), what + ": slot K - 1, depth")
        return got

    for t in range(K):
        sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
        model.step(_frames(sim, cams), _depths(sim, cams), sim.outputs()["did_reset"])
    before = check("steps")
    assert (before[:, 0, depth] != before[:, -1, depth]).any()   # the arm has moved: the slots differ in the depth channel
    mask = (e % 3 == 1).astype(np.uint8)
    sim.reset(mask=mask, seeds=np.arange(500, 500 + n, dtype=np.uint64))
    model.reset(_frames(sim, cams), _depths(sim, cams), mask)
    after = check("reset(mask)")
    _same_bytes(after[mask == 0, :-1], before[mask == 0, :-1], "older slots of the unmasked envs")
    assert (after[mask == 1, 0] == after[mask == 1, -1]).all() and (after[mask == 1] != before[mask == 1]).any()
    st = sim.get_state()
    st["qpos"][:5] += rng.uniform(-0.2, 0.2, (5, n))
    sim.set_state(qpos=st["qpos"])
    sim.reset(mask=np.zeros(n, np.uint8))
    model.reset(_frames(sim, cams), _depths(sim, cams), np.zeros(n, np.uint8))
    redrawn = check("the all-zero-mask redraw")
    _same_bytes(redrawn[:, :-1], after[:, :-1], "older slots after the redraw")
    assert (redrawn[:, -1, depth] != after[:, -1, depth]).any()
    sim.set_look(variant=((e + 1) % 4).astype(np.int32))   # (other variants: other cameras, other depths)
    model.set_look(_frames(sim, cams), _depths(sim, cams))
    looked = check("set_look")
    _same_bytes(looked[:, :-1], redrawn[:, :-1], "older slots after set_look")
    sim.close()


# ---- 8. / 10.  terminal stacks, the guards ----

@pytest.mark.parametrize("K,dtype,cams,size", [(1, "float32", ("front", "top"), SMALL), (2, "uint8", ALL, TAIL), (4, "float16", ALL, SMALL)], ids=["K1", "K2", "K4"])
def test_terminal_stacks_carry_the_depth_channel(hip_lib, K, dtype, cams, size):
    """8. / 10.  obs_stack_terminal over staggered resets is the model's history, then the terminal frames and terminal depth planes of render_terminal,
    render_terminal_planes and render_terminal_wrist through the element rule; a twin that never calls it has the same stack, history, frames and planes afterwards; the
    guard regions around the stack and the history are intact"""
    from gym_lowcostrobot_amd import VecSim

    n = 10
    kw = _kw(size, cams, look=True, planes=("depth", "segmentation"))
    stack = dict(frames=K, dtype=dtype, reset_fill="zero", cameras=cams, planes=("depth",), terminal=True)
    sim, quiet = VecSim("reach", n, obs_stack=stack, **kw), VecSim("reach", n, obs_stack=stack, **kw)
    assert sim.obs_stack_keeps_terminal and (sim.obs_stack_history is None) == (K == 1)
    if K > 1:
        assert sim.obs_stack_history.shape == (n, K - 1, 4 * len(cams)) + size and sim.obs_stack_history.dtype == np.dtype(dtype)
        assert not sim.obs_stack_history.numpy().view(np.uint8).any()
    model = ref.StackDepthRef(_frames(sim, cams), _depths(sim, cams), K, sim.depth_far)
    acts = [(s, s.alloc_actions()) for s in (sim, quiet)]
    e = np.arange(n)
    for s, _ in acts:
        _stagger(s, e % 7)
    terminals = 0
    for t in range(10):
        if t == 7:
            for s, _ in acts:
                _stagger(s, 6 - e % 7)   # the envs reset on step 6 end their next episode after one step: their reset fill is in the terminal stack
        S = model.expected(dtype, "zero")
        for s, a in acts:
            s.fill_random_actions(a, 3, t); s.step_device(a.ptr)
        dres = sim.outputs()["did_reset"]
        model.step(_frames(sim, cams), _depths(sim, cams), dres)
        ids = np.nonzero(dres)[0][::-1].astype(np.int32).copy()   # (not ascending: the assembly gathers by id)
        if ids.size:
            want = np.concatenate([S[ids, 1:], _terminal_rgbd(sim, ids, cams, dtype)[:, None]], axis=1)
            _same_bytes(sim.obs_stack_terminal(ids), want, f"terminal stacks, step {t}")
            terminals += ids.size
        _same_bytes(sim.obs_stack.numpy(), model.expected(dtype, "zero"), f"live stack, step {t}")
        for name in ["obs_stack"] + ["image_" + c for c in cams] + ["depth_" + c for c in cams] + ["seg_" + c for c in cams]:
            _same_bytes(getattr(quiet, name).numpy(), getattr(sim, name).numpy(), f"{name} of the twin, step {t}")
        if K > 1:
            _same_bytes(quiet.obs_stack_history.numpy(), sim.obs_stack_history.numpy(), f"history of the twin, step {t}")
    assert terminals >= n
    for s, a in acts:
        _guards_intact(s, s.obs_stack, "the stack's guards")
        if K > 1:
            _guards_intact(s, s.obs_stack_history, "the history's guards")
        s.free(a); s.close()


# ---- 9.  the second stream ----

def test_second_stream_gives_the_serial_stacks(hip_lib, monkeypatch):
    """9.  the same rollout with frames, planes and stack on the caller's stream (LCR_RENDER_OVERLAP=0) and on the second stream, stepped in bursts with no read in
    between: the same stacks, histories and terminal stacks"""
    from gym_lowcostrobot_amd import VecSim

    n, cams, K = 12, ALL, 4
    kw = _kw(TAIL, cams, max_episode_steps=3)
    stack = dict(frames=K, dtype="uint8", reset_fill="repeat", cameras=cams, planes=("depth",), terminal=True)
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    serial = VecSim("reach", n, obs_stack=stack, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("reach", n, obs_stack=stack, **kw)
    acts = [(s, s.alloc_actions()) for s in (serial, ovl)]
    t = terminals = 0
    for burst in (1, 1, 1, 2, 3, 1, 2):   # episodes end every 3 steps: auto-resets fall at the start, in the middle and at the end of bursts
        for _ in range(burst):
            for s, a in acts:
                s.fill_random_actions(a, 5, t); s.step_device(a.ptr)
            t += 1
        _same_bytes(ovl.obs_stack.numpy(), serial.obs_stack.numpy(), f"stack after step {t - 1}")
        _same_bytes(ovl.obs_stack_history.numpy(), serial.obs_stack_history.numpy(), f"history after step {t - 1}")
        dres = serial.outputs()["did_reset"]
        np.testing.assert_array_equal(ovl.outputs()["did_reset"], dres)
        ids = np.nonzero(dres)[0].astype(np.int32)
        if ids.size:
            _same_bytes(ovl.obs_stack_terminal(ids), serial.obs_stack_terminal(ids), f"terminal stacks after step {t - 1}")
            terminals += ids.size
    assert terminals >= 2 * n
    # the serial handle's last stack against the element rule: its newest slot is its current frames and depth planes
    _same_bytes(serial.obs_stack.numpy()[:, -1], ref.rgbd_elements(_frames(serial, cams), _depths(serial, cams), "uint8", serial.depth_far), "newest slot")
    for s, a in acts:
        s.free(a); s.close()


# ---- 11.  the vector adapters ----

def _adapter_kw():
    kw = dict(obs_stack=dict(frames=3, dtype="float16", reset_fill="zero", planes=("depth",), terminal=True), **_kw(SMALL, ALL, max_episode_steps=3))
    del kw["base_seed"]   # (the adapters pass their `seed`)
    return kw


def test_the_sb3_adapter_carries_the_rgbd_stack(hip_lib):
    """11.  LowCostRobotVecEnv: observation_space["obs_stack"] has 4 ncam channels, the live observations are sim.obs_stack, every terminal_observation has exactly the keys
    of the space and carries the terminal RGB-D stack of a twin VecSim"""
    from gym_lowcostrobot_amd import LowCostRobotVecEnv, VecSim

    n, kw = 6, _adapter_kw()
    env = LowCostRobotVecEnv("reach", n, seed=4, **kw)
    twin = VecSim("reach", n, base_seed=4, **kw)
    sp = env.observation_space.spaces if hasattr(env.observation_space, "spaces") else env.observation_space
    assert sp["obs_stack"].shape == (3, 12) + SMALL and sp["obs_stack"].dtype == np.float16
    env.reset(); twin.reset()
    rng = np.random.default_rng(0)
    finished = 0
    for t in range(7):
        a = rng.uniform(-1, 1, (n, env.sim.action_dim)).astype(np.float32)
        obs, rew, dones, infos = env.step(a)
        twin.step(a)
        ids = np.nonzero(twin.outputs()["did_reset"])[0].astype(np.int32)
        assert set(obs) == set(sp)
        _same_bytes(obs["obs_stack"], env.sim.obs_stack.numpy(), f"live, step {t}")
        _same_bytes(obs["obs_stack"], twin.obs_stack.numpy(), f"the twin's, step {t}")
        np.testing.assert_array_equal(np.nonzero(dones)[0], ids)
        tstack = twin.obs_stack_terminal(ids) if ids.size else None
        for j, i in enumerate(ids):
            tob = infos[i]["terminal_observation"]
            assert list(tob) == list(sp)
            _same_bytes(tob["obs_stack"], tstack[j], f"step {t}, env {i}")
            assert sp["obs_stack"].contains(tob["obs_stack"])
            finished += 1
    assert finished >= 2 * n
    env.close(); twin.close()


def test_the_gymnasium_adapter_carries_the_rgbd_stack(hip_lib):
    """11.  LowCostRobotVectorEnv: final_obs has exactly the keys of the observation space, and its rows of the reset envs are the twin's terminal RGB-D stacks"""
    from gym_lowcostrobot_amd import LowCostRobotVectorEnv, VecSim

    n, kw = 6, _adapter_kw()
    env = LowCostRobotVectorEnv("reach", n, seed=4, **kw)
    twin = VecSim("reach", n, base_seed=4, **kw)
    sp = env.single_observation_space.spaces if hasattr(env.single_observation_space, "spaces") else env.single_observation_space
    assert sp["obs_stack"].shape == (3, 12) + SMALL and sp["obs_stack"].dtype == np.float16
    env.reset(); twin.reset()
    rng = np.random.default_rng(0)
    finished = 0
    for t in range(7):
        a = rng.uniform(-1, 1, (n, env._v.sim.action_dim)).astype(np.float32)
        obs, rew, term, trunc, infos = env.step(a)
        twin.step(a)
        ids = np.nonzero(twin.outputs()["did_reset"])[0].astype(np.int32)
        _same_bytes(obs["obs_stack"], twin.obs_stack.numpy(), f"live, step {t}")
        if ids.size:
            fin = infos["final_obs"]
            assert list(fin) == list(sp)
            np.testing.assert_array_equal(np.nonzero(infos["_final_obs"])[0], ids)
            _same_bytes(np.ascontiguousarray(fin["obs_stack"][ids]), twin.obs_stack_terminal(ids), f"step {t}")
            finished += ids.size
    assert finished >= 2 * n
    env.close(); twin.close()


def test_without_terminal_the_rgbd_stack_is_accepted_and_not_exposed(hip_lib):
    """11.  without terminal=True the stack is accepted and not exposed, as today"""
    from gym_lowcostrobot_amd import LowCostRobotVecEnv

    env = LowCostRobotVecEnv("reach", 4, obs_stack=dict(frames=2, planes=("depth",)), max_episode_steps=2, **{k: v for k, v in _kw(SMALL, ("front", "top")).items() if k != "base_seed"})
    sp = env.observation_space.spaces if hasattr(env.observation_space, "spaces") else env.observation_space
    assert "obs_stack" not in sp and env.sim.obs_stack.shape == (4, 2, 8) + SMALL and env.sim.obs_stack_planes == ("depth",)
    env.close()


# ---- 12.  shards ----

def test_sharded_rgbd_stacks_are_the_unsharded_ones(hip_lib):
    """12.  two shards of 64 envs on one GPU give the stack and the terminal stacks of the unsharded 128-env handle"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    kw = _kw(SMALL, ALL, max_episode_steps=3)
    stack = dict(frames=4, dtype="float16", reset_fill="zero", planes=("depth",), terminal=True)
    one = VecSim("reach", 128, obs_stack=stack, **kw)
    sh = ShardedVecSim("reach", 128, [0, 0], obs_stack=stack, **kw)
    assert all(s.obs_stack_planes == ("depth",) and s.obs_stack.shape == (64, 4, 12) + SMALL for s in sh.shards)
    act = one.alloc_actions()
    total = 0
    for t in range(7):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        dres = one.outputs()["did_reset"]
        _same_bytes(np.concatenate([s.obs_stack.numpy() for s in sh.shards]), one.obs_stack.numpy(), f"stack, step {t}")
        ids = np.nonzero(dres)[0][::-1].copy()
        if ids.size:
            _same_bytes(sh.obs_stack_terminal(ids), one.obs_stack_terminal(ids), f"terminal stacks, step {t}")
            total += ids.size
    assert total >= 2 * 128
    one.free(act); one.close(); sh.close()


# ---- 13.  refusals on a device ----

def test_refusals_on_a_device(hip_lib):
    """13.  a handle without the depth plane; planes enabled after the stack; a second enable with another mask; another depth_far afterwards"""
    from gym_lowcostrobot_amd import VecSim, _capi

    cams = ("front", "top")
    sp = _capi.ObsStackSpec.from_any(dict(frames=2, cameras=cams))
    enable = lambda s, planes, keep=0: hip_lib.lcr_enable_obs_stack_planes(s.handle, ctypes.byref(sp), keep, planes)   # noqa: E731
    got = lambda s: [v.value for v in _get(hip_lib, s)]                                                                  # noqa: E731

    # no planes at all, and the segmentation plane alone: refused by name, nothing is switched on silently
    for planes in ((), ("segmentation",)):
        none = VecSim("reach", 6, **_kw(SMALL, cams, planes=planes))
        assert enable(none, _capi.PLANE_DEPTH) == _capi.LCR_ERR_INVALID and b"depth plane" in hip_lib.lcr_last_error() and b"lcr_enable_image_planes" in hip_lib.lcr_last_error()
        assert none.depth_front is None and got(none) == [0, 0.0, 0.0]
        # planes enabled after the stack: the colour stack stands, its mask is fixed, and the depth channel cannot be added to it
        assert enable(none, 0) == 0 and got(none) == [0, 0.0, 0.0]
        assert hip_lib.lcr_enable_image_planes(none.handle, _capi.PLANE_DEPTH | _capi.PLANE_SEGMENTATION if planes else _capi.PLANE_DEPTH, ctypes.c_float(0.5)) == (_capi.LCR_ERR_INVALID if planes else 0)
        assert enable(none, _capi.PLANE_DEPTH) == _capi.LCR_ERR_INVALID and (b"planes 0" in hip_lib.lcr_last_error() or b"depth plane" in hip_lib.lcr_last_error())
        view = _capi.LcrObsStackView()
        assert hip_lib.lcr_get_obs_stack(none.handle, ctypes.byref(view)) == 0 and view.channels == 6
        none.close()

    sim = VecSim("reach", 6, obs_stack=dict(frames=2, cameras=cams, planes=("depth",)), **_kw(SMALL, cams))
    inv_far, s255 = ref.constants(0.5)
    assert got(sim) == [_capi.PLANE_DEPTH, float(inv_far), float(s255)]
    assert enable(sim, _capi.PLANE_DEPTH) == 0                                                                     # the same call again: nothing
    assert enable(sim, 0) == _capi.LCR_ERR_INVALID and b"planes" in hip_lib.lcr_last_error()                      # a second enable with another mask
    assert hip_lib.lcr_enable_obs_stack(sim.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID
    assert enable(sim, _capi.PLANE_DEPTH, keep=1) == _capi.LCR_ERR_INVALID and b"keep_terminal" in hip_lib.lcr_last_error()
    assert enable(sim, _capi.PLANE_SEGMENTATION) == _capi.LCR_ERR_UNSUPPORTED
    # depth_far is fixed: the same planes and depth_far again do nothing, another depth_far is refused
    assert hip_lib.lcr_enable_image_planes(sim.handle, _capi.PLANE_DEPTH, ctypes.c_float(0.5)) == 0
    assert hip_lib.lcr_enable_image_planes(sim.handle, _capi.PLANE_DEPTH, ctypes.c_float(0.7)) == _capi.LCR_ERR_INVALID and b"depth_far" in hip_lib.lcr_last_error()
    assert got(sim) == [_capi.PLANE_DEPTH, float(inv_far), float(s255)]
    before = sim.obs_stack.numpy()
    sim.step(np.zeros((6, sim.action_dim), np.float32))
    assert sim.obs_stack.numpy().shape == before.shape == (6, 2, 8) + SMALL
    sim.close()


def _get(hip_lib, sim):
    p, a, b = ctypes.c_uint32(9), ctypes.c_float(9), ctypes.c_float(9)
    assert hip_lib.lcr_get_obs_stack_planes(sim.handle, ctypes.byref(p), ctypes.byref(a), ctypes.byref(b)) == 0
    return p, a, b
