"""The stream-order contract of the zero-copy image views (include/lcr.h, lcr_step): after an lcr_step the frames, planes, wrist frames and the observation stack are made
on an internal second stream; every entry point that takes the handle -- but lcr_step, lcr_fill_random_actions, lcr_get_outputs, lcr_step_kernel_family -- first makes the
handle's stream wait for them (a "join": an event wait on the device, no host wait).  These tests check that promise from the side it is made to: a consumer on the handle's
stream that never goes through the host.

  the sim under test  frames on the second stream (the default).  The TEST never host-synchronises it inside its loop (entry points that are synchronous by their
                      definition -- lcr_get_look, lcr_reset with a mask, lcr_set_look, lcr_get_state / lcr_set_state -- still are: the cases that call them check values,
                      not ordering).  Its consumer is torch on the handle's stream -- the default stream with nothing set, or a stream of the caller's handed to
                      set_stream --, `view.torch()[idx].clone()` for four envs spread over the batch: tiny kernels that finish in microseconds, so that a missing wait shows
                      as the previous step's bytes.  The clones are kept and compared after the loop, behind ONE final sim.sync().  (The torch views and the index tensor
                      are made once, and the caching allocator is warmed with the loop's own allocations before the loop: a hipMalloc in the loop could wait for the device
                      and hide a missing join.)
  the reference       a second sim with LCR_RENDER_OVERLAP=0 (frames on the handle's stream, after the step kernel), stepped with the same seeded actions
                      (fill_random_actions) and read through lcr_memcpy_d2h (DeviceArray.numpy(), VecSim.read_rows() for the four rows) after every step.  The rollouts of
                      the all-on and of the plain handle are computed once per module and shared.
  arming              The HIP runtime spreads the streams of a process over a few hardware queues (four by default), a new stream going to the queue with the fewest
                      streams; streams that share a queue are executed in the order of their enqueue.  Where the frame stream shares the queue of the handle's stream, the
                      frames are always finished before a read enqueued behind lcr_step runs: no unjoined read is stale, and a missing join could not show.  Which queue a
                      handle's frame stream gets depends on the streams alive in the process, so it differs from one test to the next (profiles/stream_order.txt: the same
                      control reads 331 of 336 or 0 of 336 stale clones, nothing in between, as the caller's stream changes).  Every test therefore ARMS its handle first
                      (_armed): PROBES seeded steps, each followed by clones before and behind wait_frames(); the window is open when they differ.  With a stream of the
                      caller's the probes go through fresh torch streams until one is open; if none is -- always, on the default stream -- the handle is kept alive, so that
                      its frame stream keeps its place in its queue, and the next handle is tried (four at the most: with four queues at most one of four frame streams
                      alive together shares with a given stream).  A handle that cannot be armed fails the test: it would have checked nothing.  The reference makes the
                      same PROBES steps first.
Everything is compared byte for byte; there is no tolerance in this file.

Shapes: preset fast, task push, 84 x 84 frames, max_episode_steps = 5 and 12 steps behind the probes (every env is auto-reset twice inside the loop), N_ENVS = 4 096 envs: the
work behind a step (two-camera kernel, wrist kernel, stack kernel) has to outlast the enqueue of a clone, which the control (test 6) measures on the armed handle: the lines it
prints on an MI355X are kept in profiles/stream_order.txt."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import look_ref

gpu = pytest.mark.gpu

N_ENVS = 4096
PROBES = 8
STEPS = 12
SIZE = (84, 84)
SEED = 5
BUFFERS = ("image_front", "image_top", "image_wrist", "depth_front", "seg_top", "depth_wrist", "obs_stack")
SAMPLER = {"seed": 77, "cube": ([0.2, 0.0, 0.0], [1.0, 0.6, 0.3]), "marker": ([0.0, 0.5, 0.2], [0.3, 0.5, 1.0])}
PLAIN = dict(observation_mode="both", base_seed=3, max_episode_steps=5, image_size=SIZE)
# everything on: a look with a sampler and two variants, the wrist camera, depth and segmentation planes, a stack of K = 2 uint8 frames of all three cameras
ALL_ON = dict(PLAIN, look_variants=look_ref.GPU_VARIANTS[:2], look_sampler=SAMPLER, wrist_camera=True, image_planes=("depth", "segmentation"), obs_stack=dict(frames=2, dtype="uint8"))
STREAMS = ("default", "callers")
LOOP = range(PROBES, PROBES + STEPS)   # the step numbers (the counter of fill_random_actions) of the loop behind the probes


def _idx(n):
    return [0, n // 3, n // 2, n - 1]   # first, one in between, middle, last


@pytest.fixture(autouse=True)
def preset_fast(monkeypatch):
    monkeypatch.setenv("LCR_PRESET", "fast")
    monkeypatch.delenv("LCR_RENDER_OVERLAP", raising=False)


def _serial_sim(mp, task, n, kw, warm=0):
    """the reference: frames, planes, wrist frames and stack on the handle's stream, behind the step kernel; `warm` seeded steps made (the probes of the sim under test)"""
    from gym_lowcostrobot_amd import VecSim

    mp.setenv("LCR_RENDER_OVERLAP", "0")
    try:
        sim = VecSim(task, n, **kw)
    finally:
        mp.delenv("LCR_RENDER_OVERLAP")
    act = sim.alloc_actions()
    for t in range(warm):
        sim.fill_random_actions(act, SEED, t); sim.step_device(act.ptr)
    return sim, act


def _rows(sim, names, idx):
    return {b: sim.read_rows(getattr(sim, b), idx) for b in names}


def _reference_rollout(mp, kw, names):
    """the seeded steps of LOOP on the serial handle, behind the PROBES steps; the sampled rows of `names` after every step"""
    ref, act = _serial_sim(mp, "push", N_ENVS, kw, warm=PROBES)
    rec, resets = [], []
    for t in LOOP:
        ref.fill_random_actions(act, SEED, t); ref.step_device(act.ptr)
        rec.append(_rows(ref, names, _idx(N_ENVS)))
        resets.append(ref.did_reset.numpy()[_idx(N_ENVS)])
    ref.free(act); ref.close()
    assert (np.sum(resets, axis=0) >= 2).all()   # max_episode_steps = 5: every sampled env crosses two auto-resets inside the loop
    return rec


@pytest.fixture(scope="module")
def rollouts(hip_lib):
    """name -> the reference rollout of that handle, computed once and left unchanged"""
    cache = {}
    specs = {"all_on": (ALL_ON, BUFFERS), "plain": (PLAIN, BUFFERS[:2])}

    def get(name):
        if name not in cache:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("LCR_PRESET", "fast")
                kw, names = specs[name]
                rec = _reference_rollout(mp, kw, names)
            for b in names:   # the reference is not degenerate: the sampled rows of every buffer change from step to step, so the bytes of step t - 1 are not those of step t
                changed = sum(bool((rec[t][b] != rec[t - 1][b]).any()) for t in range(1, STEPS))
                assert changed > 0, (name, b)
            cache[name] = rec
        return cache[name]

    return get


def _probe(sim, act, views, idx, t):
    """one seeded step, clones of the sampled rows before and behind wait_frames(): True when they differ -- the unjoined read saw the bytes of the step before"""
    import torch

    sim.fill_random_actions(act, SEED, t); sim.step_device(act.ptr)
    early = [v[idx].clone() for v in views]
    sim.wait_frames()
    late = [v[idx].clone() for v in views]
    sim.sync()
    return any(not torch.equal(a, b) for a, b in zip(early, late))


@contextlib.contextmanager
def _armed(kw, which, names):
    """(sim, act): a handle PROBES seeded steps into its rollout whose frame stream was seen to run beside the handle's stream (module docstring: arming); torch's current
    stream is the handle's stream -- "default": the default stream with nothing set, "callers": a torch stream handed to set_stream.  sim.armed says how it was found"""
    import torch

    from gym_lowcostrobot_amd import VecSim

    kept, found = [], None
    try:
        for handle in range(4):
            sim = VecSim("push", N_ENVS, **kw)
            act = sim.alloc_actions()
            kept.append((sim, act))
            dev = f"cuda:{sim.device}"
            views, idx = [getattr(sim, b).torch() for b in names], torch.tensor(_idx(sim.n), device=dev)
            stream, is_open = None, False
            for t in range(PROBES):   # all PROBES steps are made, also behind the probe that saw the window open: the handle reaches step PROBES, where the reference starts its loop
                if which == "callers" and not is_open:
                    stream = torch.cuda.Stream(device=dev)
                    sim.set_stream(stream.cuda_stream)
                with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                    seen = _probe(sim, act, views, idx, t)
                if seen and not is_open:
                    is_open, sim.armed = True, f"handle {handle + 1}, probe {t + 1}"
            del views
            if is_open:
                found = (sim, act, stream)
                break
        assert found is not None, (f"no handle of 4 had its frames run beside the {which} stream: unjoined reads are never stale here, the test would check nothing.  "
                                   "The runtime put every frame stream on the hardware queue of the handle's stream (or wait_frames() changes nothing): the placement follows "
                                   "GPU_MAX_HW_QUEUES (four queues assumed; with one queue no window can open) and the streams this process made before")
        sim, act, stream = found
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            yield sim, act
            sim.sync()
    finally:
        for s_, a in kept:
            s_.free(a); s_.close()


class _Consumer:
    """`view.torch()[idx].clone()` of the sampled envs of some buffers, on torch's current stream, with no host wait"""

    def __init__(self, sim, names, passes):
        import torch

        self.views = {b: getattr(sim, b).torch() for b in names}
        self.idx = torch.tensor(_idx(sim.n), device=f"cuda:{sim.device}")
        warm = [self.grab() for _ in range(passes)]   # the loop's allocations, made once and handed back to the caching allocator
        torch.cuda.current_stream().synchronize()
        del warm

    def grab(self):
        return {b: v[self.idx].clone() for b, v in self.views.items()}


def _bytes(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def _assert_rows(got, want, when):
    for b, w in want.items():
        g = _bytes(got[b])
        bad = np.argwhere(g != _bytes(w))
        assert g.shape == _bytes(w).shape and bad.size == 0, (when, b, len(bad), bad[:4].tolist())


def _joins(hip_lib, sim):
    from gym_lowcostrobot_amd import _capi

    L = hip_lib

    def raw(fn, view):
        def call():
            assert fn(sim.handle, ctypes.byref(view())) == 0, L.lcr_last_error()
        return call

    return {"wait_frames": sim.wait_frames, "lcr_get_obs": raw(L.lcr_get_obs, _capi.LcrObsView), "lcr_get_image_planes": raw(L.lcr_get_image_planes, _capi.LcrPlanesView),
            "lcr_get_wrist_camera": raw(L.lcr_get_wrist_camera, _capi.LcrWristView), "lcr_get_obs_stack": raw(L.lcr_get_obs_stack, _capi.LcrObsStackView),
            "lcr_get_look": sim.look}   # (lcr_get_look is synchronous: trivially ordered)


def _joined_rollout(sim, act, names, join, unjoined=None):
    """for the steps of LOOP: step_device, [clones with no join -> `unjoined`], join, clones.  One sync at the end.  Returns the joined clones per step"""
    got = []
    con = _Consumer(sim, names, STEPS * (2 if unjoined is not None else 1))
    for t in LOOP:
        sim.fill_random_actions(act, SEED, t); sim.step_device(act.ptr)
        if unjoined is not None:
            unjoined.append(con.grab())
        join()
        got.append(con.grab())
    sim.sync()
    got = [{b: _bytes(a) for b, a in g.items()} for g in got]
    if unjoined is not None:
        unjoined[:] = [{b: _bytes(a) for b, a in g.items()} for g in unjoined]
    return got


JOINS = ("wait_frames", "lcr_get_obs", "lcr_get_image_planes", "lcr_get_wrist_camera", "lcr_get_obs_stack", "lcr_get_look")


@gpu
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("join", JOINS)
def test_reads_behind_a_joining_call_see_the_step(hip_lib, rollouts, join, stream):
    """1. RAW: after step_device and ONE joining call, clones of the sampled envs of every buffer of the all-on handle, enqueued on the handle's stream, are the reference's
    rows of that step -- for each joining call, on the default stream and on a stream of the caller's, over 12 steps with auto-resets in between"""
    want = rollouts("all_on")
    with _armed(ALL_ON, stream, BUFFERS) as (sim, act):
        got = _joined_rollout(sim, act, BUFFERS, _joins(hip_lib, sim)[join])
    for i, t in enumerate(LOOP):
        _assert_rows(got[i], want[i], f"{join}, {stream} stream, step {t}")


@gpu
@pytest.mark.parametrize("stream", STREAMS)
def test_wait_frames_on_a_plain_handle(hip_lib, rollouts, stream):
    """1 (second handle). frames only -- no look, planes, wrist camera or stack --: wait_frames() orders image_front and image_top on both streams"""
    want = rollouts("plain")
    with _armed(PLAIN, stream, BUFFERS[:2]) as (sim, act):
        got = _joined_rollout(sim, act, BUFFERS[:2], sim.wait_frames)
    for i, t in enumerate(LOOP):
        _assert_rows(got[i], want[i], f"plain handle, {stream} stream, step {t}")


@gpu
@pytest.mark.parametrize("stream", STREAMS)
def test_no_join_where_the_library_drew_on_the_handles_stream(hip_lib, monkeypatch, stream):
    """2. a masked reset, set_look, and an all-zero-mask reset behind set_state draw on the handle's stream (they join first): clones taken directly behind them, with no
    joining call in between, are the reference's.  One of the three follows every step, in turn.  (All three wait for the stream before they return: this checks that what
    they drew is what a reader on the handle's stream gets, not an ordering.)"""
    n = N_ENVS
    rng = np.random.default_rng(8)
    masks = [(np.arange(n) % 3 == r).astype(np.uint8) for r in range(3)]
    rgbs = [rng.uniform(0, 1, (9, n)).astype(np.float32) for _ in range(STEPS)]
    dq = [rng.uniform(-0.3, 0.3, (5, n)) for _ in range(STEPS)]

    def entry_point(s_, i):
        if i % 3 == 0:
            s_.reset(mask=masks[(i // 3) % 3])
            return "reset(mask)"
        if i % 3 == 1:
            s_.set_look(rgb=rgbs[i])
            return "set_look"
        st = s_.get_state()
        st["qpos"][:5] += dq[i]
        s_.set_state(qpos=st["qpos"])
        s_.reset(mask=np.zeros(n, np.uint8))
        return "reset(zeros) after set_state"

    want, got, what = [], [], []
    ref, ract = _serial_sim(monkeypatch, "push", n, ALL_ON, warm=PROBES)
    for i, t in enumerate(LOOP):
        ref.fill_random_actions(ract, SEED, t); ref.step_device(ract.ptr)
        entry_point(ref, i)
        want.append(_rows(ref, BUFFERS, _idx(n)))
    ref.free(ract); ref.close()
    with _armed(ALL_ON, stream, BUFFERS) as (sim, act):
        con = _Consumer(sim, BUFFERS, STEPS)
        for i, t in enumerate(LOOP):
            sim.fill_random_actions(act, SEED, t); sim.step_device(act.ptr)
            what.append(entry_point(sim, i))
            got.append(con.grab())
        sim.sync()
        got = [{b: _bytes(a) for b, a in g.items()} for g in got]
        del con
    for i, t in enumerate(LOOP):
        _assert_rows(got[i], want[i], f"{what[i]}, {stream} stream, step {t}")
    for i in range(1, STEPS):   # (each of the three redrew something)
        assert (want[i]["image_front"] != want[i - 1]["image_front"]).any(), i


@gpu
@pytest.mark.parametrize("stream", STREAMS)
def test_a_slow_reader_is_not_overtaken(hip_lib, monkeypatch, stream):
    """3. WAR: behind the join of step k, clones of the WHOLE stack and of all wrist frames (hundreds of MB, milliseconds) are enqueued, then at once two more steps, so that
    both snapshot parities turn over, with no synchronisation in between.  The big clones are the reference's arrays of step k, the buffers at the end those of step k + 2"""
    import torch

    n, k = N_ENVS, PROBES + 6
    ref, ract = _serial_sim(monkeypatch, "push", n, ALL_ON, warm=PROBES)
    for t in range(PROBES, k + 1):
        ref.fill_random_actions(ract, SEED, t); ref.step_device(ract.ptr)
    want_k = {b: getattr(ref, b).numpy() for b in ("obs_stack", "image_wrist")}
    for t in range(k + 1, k + 3):
        ref.fill_random_actions(ract, SEED, t); ref.step_device(ract.ptr)
    want_end = {b: getattr(ref, b).numpy() for b in BUFFERS}
    ref.free(ract); ref.close()
    assert all((want_end[b] != want_k[b]).any() for b in want_k)

    with _armed(ALL_ON, stream, BUFFERS) as (sim, act):
        views = {b: getattr(sim, b).torch() for b in want_k}
        warm = [torch.empty_like(v) for v in views.values()]   # (the big blocks come from the caching allocator inside the loop, not from hipMalloc)
        del warm
        for t in range(PROBES, k + 1):
            sim.fill_random_actions(act, SEED, t); sim.step_device(act.ptr)
            sim.wait_frames()
        big = {b: v.clone() for b, v in views.items()}
        for t in range(k + 1, k + 3):
            sim.fill_random_actions(act, SEED, t); sim.step_device(act.ptr)
        sim.sync()
        for b in want_k:
            assert np.array_equal(_bytes(big[b]), _bytes(want_k[b])), f"{b}: the clone enqueued behind step {k} is not the reference's step {k} ({stream} stream)"
        del big, views
        for b in BUFFERS:
            assert np.array_equal(_bytes(getattr(sim, b).numpy()), _bytes(want_end[b])), f"{b} after step {k + 2} ({stream} stream)"


# ---- 4. the closed loop: a policy whose actions are an exact function of the stack ----
# Features: per env and channel the sum of every fourth pixel of every fourth row, as an integer; quantised to 1/256 of a level by integer division; projected by a fixed
# integer matrix; wrapped into 1 024 buckets (a change of 1/256 level in any channel mean moves the bucket); tanh from a table of float32 values.  Integer arithmetic and
# a table look-up only: torch on the device and numpy on the host give the same float32 actions bit for bit, whatever their reductions and their tanh round like.
_TABLE = np.tanh((np.arange(1024) - 512) / 256.0).astype(np.float32)


def _weights(channels, k):
    w = np.random.default_rng(0).integers(-3, 4, (channels, k))
    w[w == 0] = 1
    return w.astype(np.int64)


def _policy_numpy(stack, w):
    n = stack.shape[0]
    x = stack.reshape(n, -1, *stack.shape[-2:])[:, :, ::4, ::4]
    cnt = x.shape[2] * x.shape[3]
    q = x.sum(axis=(2, 3), dtype=np.int64) * 256 // cnt
    z = (q[:, :, None] * w[None]).sum(axis=1)
    return np.ascontiguousarray(_TABLE[z % 1024].T)   # [k][N]


def _policy_torch(stack, w, table):
    import torch

    n = stack.shape[0]
    x = stack.reshape(n, -1, *stack.shape[-2:])
    assert x.data_ptr() == stack.data_ptr()   # a view: the policy reads the library's buffer
    x = x[:, :, ::4, ::4]
    cnt = x.shape[2] * x.shape[3]
    q = torch.div(x.sum(dim=(2, 3), dtype=torch.int64) * 256, cnt, rounding_mode="floor")
    z = (q[:, :, None] * w[None]).sum(dim=1)
    return table[torch.remainder(z, 1024)].t().contiguous()   # [k][N]


def _routes_agree(dev):
    import torch

    rng = np.random.default_rng(1)
    s = rng.integers(0, 256, (37, 2, 9) + SIZE, dtype=np.uint8)
    s[5] = 255; s[6] = 0; s[3] = np.minimum(s[3], 254)
    w = _weights(18, 5)
    want = _policy_numpy(s, w)
    assert want.shape == (5, 37) and want.dtype == np.float32 and len(np.unique(want)) > 100
    got = _policy_torch(torch.from_numpy(s).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(_TABLE).to(dev))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=dev)
    moved = s.copy(); moved[3, 1, 4, ::4, ::4] += 1   # one level in one channel of one env: that env's actions move, no other's
    diff = (_policy_numpy(moved, w) != want).any(axis=0)
    assert diff[3] and diff.sum() == 1


def test_policy_routes_agree_on_the_cpu():
    """4 (premise, no GPU). random uint8 stacks: the torch route on the CPU and the numpy route give identical float32 actions"""
    _routes_agree("cpu")


@gpu
def test_policy_routes_agree_on_the_device(hip_lib):
    """4 (premise). the torch route on the device and the numpy route give identical float32 actions"""
    import torch

    _routes_agree(f"cuda:{torch.cuda.current_device()}")


@gpu
@pytest.mark.parametrize("stream", STREAMS)
def test_closed_loop_on_the_handles_stream(hip_lib, monkeypatch, stream):
    """4. the loop as a user writes it, 12 times: step_device, wait_frames(), x = stack.reshape(n, K * C, H, W), a torch op makes the next [k][N] action tensor from x, the next
    step_device takes its data_ptr() -- no host wait anywhere.  The reference computes the same actions in numpy from its .numpy() reads.  A stale read changes an action and
    with it the state: final qpos, rng and stack are compared bit for bit"""
    import torch

    n = N_ENVS
    kw = dict(PLAIN, wrist_camera=True, obs_stack=dict(frames=2, dtype="uint8"))
    ref, ract = _serial_sim(monkeypatch, "push", n, kw, warm=PROBES)
    w = _weights(int(np.prod(ref.obs_stack.shape[1:3])), ref.action_dim)
    ref.fill_random_actions(ract, SEED, PROBES); ref.step_device(ract.ptr)
    used = []
    for _ in range(1, STEPS):
        a = _policy_numpy(ref.obs_stack.numpy(), w)
        used.append(a)
        ref.step(a.T)
    want = dict(ref.get_state(), stack=ref.obs_stack.numpy())
    ref.free(ract); ref.close()
    assert all((used[i] != used[i - 1]).mean() > 0.5 for i in range(1, len(used)))   # the actions follow the frames

    with _armed(kw, stream, ("obs_stack", "image_wrist")) as (sim, act):
        dev = f"cuda:{sim.device}"
        wt, table, stack = torch.from_numpy(w).to(dev), torch.from_numpy(_TABLE).to(dev), sim.obs_stack.torch()
        warm = [_policy_torch(stack, wt, table) for _ in range(STEPS)]
        torch.cuda.current_stream().synchronize()
        del warm
        sim.fill_random_actions(act, SEED, PROBES); sim.step_device(act.ptr)
        acts = []
        for _ in range(1, STEPS):
            sim.wait_frames()
            acts.append(_policy_torch(stack, wt, table))   # (kept: the step kernel reads it after this iteration)
            sim.step_device(acts[-1].data_ptr())
        sim.sync()
        got = dict(sim.get_state(), stack=sim.obs_stack.numpy())
        for i, a in enumerate(acts):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), used[i].view(np.uint32)), f"actions of iteration {i + 1} ({stream} stream)"
        del acts, stack
    for key in ("qpos", "rng", "stack"):
        assert np.array_equal(_bytes(got[key]), _bytes(want[key])), f"{key} after the closed loop ({stream} stream)"


@gpu
@pytest.mark.parametrize("mode,n", [("state", 65536), ("both", 2048)])
def test_set_stream_with_work_in_flight(hip_lib, monkeypatch, mode, n):
    """5. lcr_set_stream synchronises the old stream before it switches: fill_random_actions and step_device on stream A, set_stream(B) at once, fill_random_actions (into
    the same action buffer) and step_device on B -- the state is, bit for bit, that of a sim that made the same two steps on one stream.  Default preset, ReachCube: a step
    of 65 536 envs takes milliseconds, the enqueue of the second one microseconds"""
    import torch

    from gym_lowcostrobot_amd import VecSim

    monkeypatch.delenv("LCR_PRESET")
    kw = dict(observation_mode=mode, base_seed=3)
    one = VecSim("reach", n, **kw)
    act = one.alloc_actions()
    for t in range(2):
        one.fill_random_actions(act, SEED, t); one.step_device(act.ptr)
    want = one.get_state()
    want_img = one.image_front.numpy() if mode == "both" else None
    one.free(act); one.close()

    sim = VecSim("reach", n, **kw)
    a, b = torch.cuda.Stream(device=sim.device), torch.cuda.Stream(device=sim.device)
    act = sim.alloc_actions()
    sim.set_stream(a.cuda_stream)
    sim.fill_random_actions(act, SEED, 0); sim.step_device(act.ptr)
    sim.set_stream(b.cuda_stream)
    sim.fill_random_actions(act, SEED, 1); sim.step_device(act.ptr)
    got = sim.get_state()
    for key, v in want.items():
        assert np.array_equal(_bytes(got[key]), _bytes(v)), (mode, key)
    if mode == "both":
        np.testing.assert_array_equal(sim.image_front.numpy(), want_img)
    sim.free(act); sim.close()


@gpu
@pytest.mark.parametrize("stream", STREAMS)
def test_control_unjoined_reads_may_be_stale(hip_lib, rollouts, capsys, stream):
    """6. control, printed and not asserted: on the armed all-on handle the sampled clones are taken once per step WITHOUT a join -- the contract allows them to be stale; they
    read old bytes of the handle's own buffers --, then again behind wait_frames().  Only the joined reads are asserted.  The count of unjoined clones that differ from the
    reference is the evidence that the window the other tests guard is open at N_ENVS = 4 096, on the handles those tests use (armed the same way).  On an MI355X
    (profiles/stream_order.txt): 331 of 336 on either stream -- obs_stack 48 of 48, image_wrist 46 of 48; 4 096 envs are enough, the batch was not raised."""
    want = rollouts("all_on")
    unjoined = []
    with _armed(ALL_ON, stream, BUFFERS) as (sim, act):
        got = _joined_rollout(sim, act, BUFFERS, sim.wait_frames, unjoined=unjoined)
        armed = sim.armed
    rows = len(_idx(N_ENVS))
    stale = {b: sum(int((unjoined[i][b][r] != _bytes(want[i][b])[r]).any()) for i in range(STEPS) for r in range(rows)) for b in BUFFERS}
    total = STEPS * rows
    with capsys.disabled():
        print(f"\n[stream-order] unjoined reads stale: {sum(stale.values())} of {total * len(BUFFERS)} at {N_ENVS} envs, {stream} stream, armed at {armed} ("
              + ", ".join(f"{b} {c} of {total}" for b, c in stale.items()) + ")")
    for i, t in enumerate(LOOP):
        _assert_rows(got[i], want[i], f"joined reads of the control, step {t}")
