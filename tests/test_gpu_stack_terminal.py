"""Terminal observation stacks on the GPU (VecSim(..., obs_stack=dict(..., terminal=True)); lcr_obs_stack_terminal): the stack of an episode that has ended, bit for bit.

The reference never uses the library's history buffer.  Before every step the whole live stack S is read; after the step, for the envs the step has reset, the terminal
stack must be concat(S[id, 1:], T[id]) with T the terminal frames of render_terminal (and render_terminal_wrist), channels-first, through the header's element rule in numpy:
uint8, np.float32(x) * np.float32(1 / 255), that rounded to float16.  Everything is compared byte for byte; there is no tolerance in this feature.

Shapes: 70 envs leave the step kernel a ragged last wave; 16 x 16 is one partial tile of the stack kernel (256 pixels), 32 x 36 a full tile of 1 024 pixels and a tail of 128.
Episode ends are staggered with set_state(elapsed = 49 - e % 7): the resets of the first seven steps fall on seven different steps; a second staggering in the opposite order
then ends the episodes of the envs that were reset last after ONE step, so that their reset fill is still in the terminal stack."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 70
ALL = ("front", "top", "wrist")
SMALL, TAIL = (16, 16), (32, 36)
# task, size, K, dtype, fill, cameras, looks
CASES = [
    ("reach", SMALL, 1, "uint8", "repeat", ("front",), False),
    ("reach", TAIL, 2, "float16", "zero", ("front", "top"), False),
    ("reach", SMALL, 4, "float32", "repeat", ALL, False),
    ("reach", TAIL, 8, "uint8", "zero", ALL, False),
    ("reach", TAIL, 4, "float16", "repeat", ("front",), True),
    ("reach", SMALL, 8, "float16", "repeat", ("front", "top"), False),
    ("stack", TAIL, 4, "uint8", "repeat", ("front", "top"), False),
    ("push", SMALL, 8, "float32", "zero", ("front", "top"), False),
    ("reach", TAIL, 2, "float32", "repeat", ALL, True),
]
IDS = [f"{c[0]}-{c[1][0]}x{c[1][1]}-K{c[2]}-{c[3]}-{c[4]}-{'+'.join(c[5])}{'-look' if c[6] else ''}" for c in CASES]


def _elements(x, dtype):
    """the header's element rule for source bytes x"""
    if dtype == "uint8":
        return x
    f = np.float32(1) * x.astype(np.float32) * np.float32(1 / 255)
    assert f.dtype == np.float32
    return f if dtype == "float32" else f.astype(np.float16)


def _kw(size, cams, look, **more):
    from tests import look_ref

    kw = dict(observation_mode="both", image_size=size, base_seed=11, wrist_camera=True if "wrist" in cams else None, **more)
    if look:
        kw.update(look_variants=look_ref.GPU_VARIANTS, look_sampler={"seed": 5, "cube": ([0.2, 0, 0], [1, 0.4, 0.4])})
    return kw


def _terminal_frames(sim, ids, cams, dtype):
    """T: the terminal frames of the listed envs by the existing calls, channels-first in the stack's camera order, as elements -> (len(ids), C, H, W)"""
    front, top = sim.render_terminal(ids)
    fr = {"front": front, "top": top}
    if "wrist" in cams:
        fr["wrist"] = sim.render_terminal_wrist(ids)["image_wrist"]
    return _elements(np.concatenate([np.ascontiguousarray(np.moveaxis(fr[c], -1, 1)) for c in cams], axis=1), dtype)


def _stagger(sim, order):
    sim.set_state(elapsed=(49 - order).astype(np.int32))


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (what, len(bad), bad[:6].tolist())


def _rollout(sim, cams, K, dtype, fill, steps=14, act_seed=3):
    """the staggered rollout with the rule of check 1 asserted after every step -> what it contained"""
    e = np.arange(sim.n)
    act = sim.alloc_actions()
    age = np.zeros(sim.n, int)       # steps of the current episode so far
    resets = np.zeros(sim.n, int)
    seen = {"terminals": 0, "short": 0, "first_full": 0, "reset_steps": set()}
    _stagger(sim, e % 7)
    for t in range(steps):
        if t == 7:
            _stagger(sim, 6 - e % 7)   # the envs reset on step 6 end their next episode on step 7, after one step
        S = sim.obs_stack.numpy()
        sim.fill_random_actions(act, act_seed, t); sim.step_device(act.ptr)
        dres = sim.outputs()["did_reset"]
        ids = np.nonzero(dres)[0].astype(np.int32)
        age += 1
        if ids.size:
            T = _terminal_frames(sim, ids, cams, dtype)
            want = np.concatenate([S[ids, 1:], T[:, None]], axis=1)
            got = sim.obs_stack_terminal(ids)
            _same_bytes(got, want, f"terminal stacks, step {t}")
            seen["terminals"] += ids.size
            seen["reset_steps"].add(t)
            for i, env in enumerate(ids):
                L = age[env]                      # the episode's steps, the terminal one included: its frames fill the last L + 1 slots (the reset frame first)
                if L < K - 1 and resets[env] > 0:  # shorter than K - 1 steps: slots 0 .. K - 2 - L still hold the reset fill
                    pad = want[i, :K - 1 - L]
                    if fill == "zero":
                        assert not pad.view(np.uint8).any(), (t, env)
                    else:
                        assert (pad.view(np.uint8) == want[i, K - 1 - L].view(np.uint8)[None]).all(), (t, env)
                    assert want[i, K - 1 - L].any(), (t, env)   # (the reset frame itself)
                    seen["short"] += 1
                if resets[env] == 0 and L >= K - 1:   # a first episode with K - 1 steps behind it: every slot predates any reset of the env
                    seen["first_full"] += 1
        # the live stack is the reset one: its newest slot shows the reset state, not the terminal frame
        age[dres] = 0; resets[dres] += 1
    sim.free(act)
    return seen


@pytest.mark.parametrize("task,size,K,dtype,fill,cams,look", CASES, ids=IDS)
def test_terminal_stacks_bit_for_bit(hip_lib, task, size, K, dtype, fill, cams, look):
    """1.  Over 14 steps every env ends two episodes.  The case must itself contain a terminal stack whose history predates any reset of its env, and -- where one can exist --
    one whose episode was shorter than K - 1 steps, with the reset fill in it.  (An episode has at least one step, so with K <= 2 no terminal stack can show the fill: the
    older slot of K = 2 is the episode's own previous frame.)"""
    from gym_lowcostrobot_amd import VecSim

    sim = VecSim(task, N, obs_stack=dict(frames=K, dtype=dtype, reset_fill=fill, cameras=cams, terminal=True), **_kw(size, cams, look))
    assert sim.obs_stack_keeps_terminal and sim.obs_stack_spec == {"frames": K, "cameras": cams, "dtype": dtype, "reset_fill": fill}
    assert (sim.obs_stack_history is None) == (K == 1)
    if K > 1:
        assert sim.obs_stack_history.shape == (N, K - 1, 3 * len(cams)) + size and sim.obs_stack_history.dtype == np.dtype(dtype)
        assert not sim.obs_stack_history.numpy().view(np.uint8).any()   # zero-filled: enabling saves nothing
    seen = _rollout(sim, cams, K, dtype, fill)
    assert seen["terminals"] >= 2 * N and seen["reset_steps"] == set(range(14)), seen   # (more where an episode also ends by success)
    assert seen["first_full"] > 0, seen
    if K >= 3:
        assert seen["short"] > 0, seen
    sim.close()


def _guard_bytes(sim, arr):
    from tests.test_gpu_wrist import _guards

    return [g.copy() for g in _guards(sim, arr)]


def test_only_step_refills_save(hip_lib):
    """2.  reset(mask), set_look and the no-op reset refill or rewrite the live stack and leave the history and the guards round it alone; the terminal stacks of the last
    step are still returned until the next step"""
    from gym_lowcostrobot_amd import VecSim, _capi

    K, cams = 4, ("front", "top")
    sim = VecSim("reach", N, obs_stack=dict(frames=K, dtype="float16", reset_fill="zero", cameras=cams, terminal=True), **_kw(TAIL, cams, True))
    e = np.arange(N)
    rng = np.random.default_rng(0)
    _stagger(sim, e % 7)
    for t in range(3):
        sim.step(rng.uniform(-1, 1, (N, sim.action_dim)).astype(np.float32))
    ids = np.nonzero(sim.outputs()["did_reset"])[0].astype(np.int32)
    assert 0 < ids.size < N
    hist, guards, term = sim.obs_stack_history.numpy(), _guard_bytes(sim, sim.obs_stack_history), sim.obs_stack_terminal(ids)
    assert hist[ids].any() and all(g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all() for g in guards)
    assert all((g == _capi.WRIST_GUARD_BYTE).all() for g in _guard_bytes(sim, sim.obs_stack))

    def unchanged(when):
        _same_bytes(sim.obs_stack_history.numpy(), hist, f"history after {when}")
        for g, g0 in zip(_guard_bytes(sim, sim.obs_stack_history), guards):
            np.testing.assert_array_equal(g, g0, err_msg=when)
        _same_bytes(sim.obs_stack_terminal(ids), term, f"terminal stacks after {when}")

    live = sim.obs_stack.numpy()
    mask = (e % 3 == 1).astype(np.uint8)
    assert mask[ids].any() and not mask[ids].all()
    sim.reset(mask=mask, seeds=np.arange(500, 500 + N, dtype=np.uint64))
    assert (sim.obs_stack.numpy()[mask == 1] != live[mask == 1]).any()   # the masked envs were refilled ...
    unchanged("reset(mask)")                                             # ... and nothing was saved
    sim.set_look(variant=((e + 1) % 4).astype(np.int32))
    unchanged("set_look")
    st = sim.get_state()
    st["qpos"][:5] += rng.uniform(-0.2, 0.2, (5, N))
    sim.set_state(qpos=st["qpos"])
    sim.reset(mask=np.zeros(N, np.uint8))
    unchanged("the no-op reset")
    # the next step: the envs it resets save again, the history of every other env stands
    S = sim.obs_stack.numpy()
    sim.step(rng.uniform(-1, 1, (N, sim.action_dim)).astype(np.float32))
    dres = sim.outputs()["did_reset"]
    assert dres.any() and not dres.all()
    after = sim.obs_stack_history.numpy()
    _same_bytes(after[~dres], hist[~dres], "history of the envs the step did not reset")
    _same_bytes(after[dres], S[dres, 1:], "history of the envs the step reset")
    sim.close()


def _three_way(task, kw, stack):
    from gym_lowcostrobot_amd import VecSim

    return [VecSim(task, N, obs_stack=dict(stack, **extra), **kw) for extra in (dict(terminal=True), dict(terminal=True), dict())]


def test_nothing_else_moves(hip_lib):
    """4.  A handle with terminal=True whose terminal methods are called after every step, one with terminal=True where they never are, and one without terminal produce
    identical live stacks, frames, outputs and state over the rollout"""
    cams = ALL
    called, quiet, plain = _three_way("push", _kw(TAIL, cams, True), dict(frames=4, dtype="float16", reset_fill="repeat", cameras=cams))
    assert plain.obs_stack_keeps_terminal is False and plain.obs_stack_history is None
    with pytest.raises(ValueError, match="terminal=True"):
        plain.obs_stack_terminal(np.zeros(0, np.int32))
    e = np.arange(N)
    acts = [(s, s.alloc_actions()) for s in (called, quiet, plain)]
    for s, _ in acts:
        _stagger(s, e % 7)
    n_term = 0
    for t in range(9):
        for s, a in acts:
            s.fill_random_actions(a, 7, t); s.step_device(a.ptr)
        ids = np.nonzero(called.outputs()["did_reset"])[0].astype(np.int32)
        if ids.size:
            called.obs_stack_terminal(ids); n_term += ids.size
        ref_state, ref_out = called.get_state(), called.outputs()
        for other in (quiet, plain):
            for name in ["obs_stack"] + ["image_" + c for c in cams]:
                _same_bytes(getattr(other, name).numpy(), getattr(called, name).numpy(), f"{name}, step {t}")
            st, out = other.get_state(), other.outputs()
            for k in ref_state:
                np.testing.assert_array_equal(st[k], ref_state[k], err_msg=f"{k}, step {t}")
            for k in ref_out:
                np.testing.assert_array_equal(out[k], ref_out[k], err_msg=f"{k}, step {t}")
        _same_bytes(quiet.obs_stack_history.numpy(), called.obs_stack_history.numpy(), f"history, step {t}")
    assert n_term >= N
    for s, a in acts:
        s.free(a); s.close()


def test_second_stream_gives_the_serial_terminal_stacks(hip_lib, monkeypatch):
    """3.  The same rollout with frames and stack on the caller's stream (LCR_RENDER_OVERLAP=0) and on the second stream, steps issued in bursts with no read in between:
    the same terminal stacks and the same history (on the second stream the save reads the did_reset snapshot, which the next step kernel cannot overwrite)"""
    from gym_lowcostrobot_amd import VecSim

    cams, K = ALL, 4
    kw = _kw(TAIL, cams, True, max_episode_steps=3)
    stack = dict(frames=K, dtype="uint8", reset_fill="zero", cameras=cams, terminal=True)
    monkeypatch.setenv("LCR_RENDER_OVERLAP", "0")
    ref = VecSim("reach", N, obs_stack=stack, **kw)
    monkeypatch.delenv("LCR_RENDER_OVERLAP")
    ovl = VecSim("reach", N, obs_stack=stack, **kw)
    acts = [(s, s.alloc_actions()) for s in (ref, ovl)]
    t = got_terminals = 0
    for burst in (1, 1, 1, 2, 3, 1, 2):   # episodes end every 3 steps: auto-resets fall at the start, in the middle and at the end of bursts
        for _ in range(burst):
            for s, a in acts:
                s.fill_random_actions(a, 5, t); s.step_device(a.ptr)
            t += 1
        _same_bytes(ovl.obs_stack_history.numpy(), ref.obs_stack_history.numpy(), f"history after step {t - 1}")
        dres = ref.outputs()["did_reset"]
        np.testing.assert_array_equal(ovl.outputs()["did_reset"], dres)
        ids = np.nonzero(dres)[0].astype(np.int32)
        if ids.size:
            _same_bytes(ovl.obs_stack_terminal(ids), ref.obs_stack_terminal(ids), f"terminal stacks after step {t - 1}")
            got_terminals += ids.size
    assert got_terminals >= 2 * N
    for s, a in acts:
        s.free(a); s.close()


def test_several_passes(hip_lib):
    """5.  More envs than one pass of the driver takes: per env the staging holds the three cameras' terminal frames and the terminal stack, and a pass keeps that within
    450 MiB (the budget of the terminal-frame calls).  N is the smallest multiple of 64 beyond it; every env ends on the same step"""
    from gym_lowcostrobot_amd import VecSim

    K, cams, dtype, size = 8, ALL, "float32", SMALL
    px = size[0] * size[1]
    per_env = 3 * (px * 3) + K * 3 * len(cams) * px * 4
    n = ((450 << 20) // per_env // 64 + 1) * 64
    assert n * per_env > (450 << 20) >= (n - 64) * per_env and n == 6208
    sim = VecSim("reach", n, obs_stack=dict(frames=K, dtype=dtype, reset_fill="repeat", cameras=cams, terminal=True), **_kw(size, cams, False))
    act = sim.alloc_actions()
    for t in range(3):
        sim.fill_random_actions(act, 9, t); sim.step_device(act.ptr)
    sim.set_state(elapsed=np.full(n, 49, np.int32))
    S = sim.obs_stack.numpy()
    sim.fill_random_actions(act, 9, 3); sim.step_device(act.ptr)
    assert sim.outputs()["did_reset"].all()
    ids = np.arange(n, dtype=np.int32)[::-1].copy()   # (not the identity: the assembly gathers by id)
    got = sim.obs_stack_terminal(ids)
    T = _terminal_frames(sim, ids, cams, dtype)
    _same_bytes(got[:, -1], T, "newest slot")
    _same_bytes(got[:, :-1], S[ids, 1:], "older slots")
    assert (got[:, 0] != got[:, -1]).any() and (got[0] != got[-1]).any()
    sim.free(act); sim.close()


def test_refusals(hip_lib):
    """8.  An env the last step did not reset, an id out of range, a handle without a stack or without terminal=True; count = 0 is allowed; K = 1 works"""
    from gym_lowcostrobot_amd import VecSim, _capi
    import ctypes

    cams = ("front", "top")
    sim = VecSim("reach", N, obs_stack=dict(frames=2, cameras=cams, terminal=True), **_kw(SMALL, cams, False))
    _stagger(sim, np.arange(N) % 7)
    sim.step(np.zeros((N, sim.action_dim), np.float32))
    dres = sim.outputs()["did_reset"]
    done, alive = np.nonzero(dres)[0], np.nonzero(~dres)[0]
    assert done.size and alive.size
    assert sim.obs_stack_terminal(done).shape == (done.size, 2, 6) + SMALL
    with pytest.raises(ValueError, match="did_reset"):
        sim.obs_stack_terminal([done[0], alive[0]])
    for bad in ([N], [-1], [done[0], N + 5]):
        with pytest.raises(ValueError, match="out of range"):
            sim.obs_stack_terminal(bad)
    assert sim.obs_stack_terminal([]).shape == (0, 2, 6) + SMALL
    assert hip_lib.lcr_obs_stack_terminal(sim.handle, None, 0, None) == 0
    assert hip_lib.lcr_obs_stack_terminal(sim.handle, None, 1, None) == _capi.LCR_ERR_INVALID and hip_lib.lcr_obs_stack_terminal(sim.handle, None, -1, None) == _capi.LCR_ERR_INVALID
    # life: the same spec and keep_terminal again do nothing, another keep_terminal is refused
    sp = _capi.ObsStackSpec.from_any(dict(frames=2, cameras=cams))
    assert hip_lib.lcr_enable_obs_stack_terminal(sim.handle, ctypes.byref(sp), 1) == 0
    assert hip_lib.lcr_enable_obs_stack_terminal(sim.handle, ctypes.byref(sp), 0) == _capi.LCR_ERR_INVALID and b"keep_terminal" in hip_lib.lcr_last_error()
    assert hip_lib.lcr_enable_obs_stack(sim.handle, ctypes.byref(sp)) == _capi.LCR_ERR_INVALID
    sim.close()

    ids, out = np.zeros(1, np.int32), np.zeros(2 * 6 * 256, np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    plain = VecSim("reach", 5, obs_stack=2, **_kw(SMALL, cams, False))
    assert hip_lib.lcr_obs_stack_terminal(plain.handle, vp(ids), 1, vp(out)) == _capi.LCR_ERR_INVALID and b"keep_terminal" in hip_lib.lcr_last_error()
    keep, hist, nbytes = ctypes.c_int32(5), ctypes.c_void_p(1), ctypes.c_uint64(9)
    assert hip_lib.lcr_get_obs_stack_terminal(plain.handle, ctypes.byref(keep), ctypes.byref(hist), ctypes.byref(nbytes)) == 0
    assert (keep.value, hist.value, nbytes.value) == (0, None, 0)
    sp = _capi.ObsStackSpec.from_any(2)
    assert hip_lib.lcr_enable_obs_stack(plain.handle, ctypes.byref(sp)) == 0                       # the same call again: nothing
    assert hip_lib.lcr_enable_obs_stack_terminal(plain.handle, ctypes.byref(sp), 1) == _capi.LCR_ERR_INVALID
    plain.close()
    none = VecSim("reach", 5, **_kw(SMALL, cams, False))
    assert hip_lib.lcr_obs_stack_terminal(none.handle, vp(ids), 1, vp(out)) == _capi.LCR_ERR_INVALID and b"no observation stack" in hip_lib.lcr_last_error()
    with pytest.raises(ValueError, match="no obs_stack"):
        none.obs_stack_terminal([0])
    none.close()
    one = VecSim("reach", 5, max_episode_steps=1, obs_stack=dict(frames=1, dtype="float32", terminal=True), **_kw(SMALL, cams, False))   # K = 1: the terminal frame alone
    assert one.obs_stack_keeps_terminal and one.obs_stack_history is None
    one.step(np.zeros((5, one.action_dim), np.float32))
    ids = np.arange(5, dtype=np.int32)
    _same_bytes(one.obs_stack_terminal(ids)[:, 0], _terminal_frames(one, ids, cams, "float32"), "K = 1")
    one.close()


def test_sharded_terminal_stacks_are_the_unsharded_ones(hip_lib):
    """10.  Two shards of 64 envs on one GPU return the terminal stacks of the unsharded 128-env handle, by global env id"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    cams = ALL
    kw = _kw(SMALL, cams, False, max_episode_steps=3)
    stack = dict(frames=4, dtype="float16", reset_fill="zero", terminal=True)
    one = VecSim("push", 128, obs_stack=stack, **kw)
    sh = ShardedVecSim("push", 128, [0, 0], obs_stack=stack, **kw)
    act = one.alloc_actions()
    total = 0
    for t in range(7):
        one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
        sh.fill_random_actions(7, t); sh.step_device()
        dres = one.outputs()["did_reset"]
        np.testing.assert_array_equal(sh.outputs()["did_reset"], dres)
        ids = np.nonzero(dres)[0][::-1].copy()
        if ids.size:
            _same_bytes(sh.obs_stack_terminal(ids), one.obs_stack_terminal(ids), f"step {t}")
            total += ids.size
    assert total >= 2 * 128
    one.free(act); one.close(); sh.close()
