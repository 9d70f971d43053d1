"""The depth channel of the observation stack (VecSim(obs_stack=dict(..., planes=("depth",)))): what the RGB-D build of the stack kernel costs beside the colour build, and
beside the torch expression it replaces.
    python tools/obs_stack_depth_times.py [all|parent] [n_envs] [task] [H W]        (default all 32768 stack 84 84; cameras front + top, K = 4, uint8 and float16)
    parent: only the sims a checkout of the parent commit has (no stack, the colour stack) -- run there, in the same session, it re-measures the yardstick.
Frames, planes and stack on the caller's stream (LCR_RENDER_OVERLAP=0), preset fast, image_planes=("depth",) on EVERY sim, the one without a stack included, so that the
frame kernels are the same everywhere.  As in tools/obs_stack_times.py the library has no entry point that launches the stack kernel by itself: a kernel time here is the
DIFFERENCE of the median step time of a sim with the stack and of the one without in the same round, device events, windows of ten steps after a warm-up of twenty.
Bytes of a push from the shapes, per pixel and camera: the colour build reads 3 source bytes and K - 1 slots of 3 elements and writes K slots of 3; the depth build reads
3 + 4 source bytes and moves (2 K - 1) 4 elements.  The ratio of those byte counts is printed beside the measured ratio of the two kernel times, with the run-to-run spread
of the colour stack (the largest window minus the smallest, as a share of the kernel time).
The torch expression: scale, cast, permute, cat, roll and a masked refill from did_reset on the library's own frame and depth tensors, timed in the same windows."""
import os
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

args = sys.argv[1:]
what = args[0] if len(args) > 0 else "all"
n = int(args[1]) if len(args) > 1 else 32768
task = args[2] if len(args) > 2 else "stack"
H, W = (int(args[3]), int(args[4])) if len(args) > 4 else (84, 84)
CAMS, K, FAR = 2, 4, 10.0
WINDOWS, PER = 7, 10
HBM_PEAK = 8.0e12


def make(stack):
    from gym_lowcostrobot_amd import VecSim

    os.environ["LCR_RENDER_OVERLAP"] = "0"
    sim = VecSim(task, n, observation_mode="both", image_size=(H, W), preset="fast", image_planes=("depth",), depth_far=FAR, **({"obs_stack": stack} if stack else {}))
    os.environ.pop("LCR_RENDER_OVERLAP", None)
    act = [sim.alloc_actions() for _ in range(8)]
    for t, a in enumerate(act):
        sim.fill_random_actions(a, 1, t)
    for t in range(20):   # warm: clocks, and a few auto-resets behind
        sim.step_device(act[t % 8].ptr)
    sim.sync()
    return sim, act


def windows(sim, act, extra=None):
    """median (min, max) ms per step over WINDOWS windows of PER steps, device events; `extra(sim)` runs after every step inside the window"""
    w = []
    for _ in range(WINDOWS):
        sim.timer_begin()
        for t in range(PER):
            sim.step_device(act[t % 8].ptr)
            if extra:
                extra(sim)
        w.append(sim.timer_end() / PER)
    return float(np.median(w)), min(w), max(w)


def close(sim, act):
    for a in act:
        sim.free(a)
    sim.close()


def push_bytes(esize, depth):
    cpc, source = (4, 7) if depth else (3, 3)
    return n * CAMS * H * W * (source + (2 * K - 1) * cpc * esize)


def torch_stacker(sim, dtype):
    """the RGB-D stack kept with torch operations on the library's own frame and depth tensors; returns (update(sim), the state dict that holds the stack)"""
    import torch

    half = dtype == "float16"
    inv_far, s255 = float(np.float32(1.0 / sim.depth_far)), float(np.float32(255.0 / sim.depth_far))
    cams = [(sim.image_front.torch(), sim.depth_front.torch()), (sim.image_top.torch(), sim.depth_top.torch())]
    did = sim.did_reset.torch()

    def frame():
        parts = []
        for rgb, d in cams:
            rgb = rgb.permute(0, 3, 1, 2)
            if half:
                parts += [(rgb.to(torch.float32) * (1.0 / 255.0)).to(torch.float16), (d * inv_far).clamp(max=1.0).to(torch.float16).unsqueeze(1)]
            else:
                parts += [rgb, (d * s255 + 0.5).clamp(max=255.0).to(torch.uint8).unsqueeze(1)]
        return torch.cat(parts, dim=1)

    st = {"stack": frame().unsqueeze(1).repeat(1, K, 1, 1, 1).contiguous()}

    def update(sim):
        # (serial streams: the frames of this step are drawn on the handle's stream, which is torch's current stream here -- plain stream order, no synchronisation)
        x = frame()
        s = torch.roll(st["stack"], -1, dims=1)
        s[:, -1] = x
        idx = did.nonzero().squeeze(1)
        if idx.numel():
            s[idx] = x[idx].unsqueeze(1)
        st["stack"] = s

    return update, st


print(f"observation stack with the depth channel: {task}, {n} envs, {H} x {W}, cameras front + top, K = {K}, depth_far {FAR}; mode {what}")
print(f"serial streams, preset fast, depth plane on everywhere; ms per step, median of {WINDOWS} windows of {PER} (min max)")
print("'kernel' = that median minus the median of the sim without a stack in the same round: not a directly timed launch")
for rnd in (1, 2):
    sim, act = make(None)
    b = windows(sim, act)
    close(sim, act)
    print(f"  round {rnd}  no stack (step + frames + depth)  {b[0]:8.3f} ({b[1]:.3f} {b[2]:.3f})", flush=True)
    for dtype in ("uint8", "float16"):
        esize = np.dtype(dtype).itemsize
        res = {}
        for name, depth in (("colour", False),) + ((("rgb-d", True),) if what != "parent" else ()):
            stack = {"frames": K, "dtype": dtype, "cameras": ("front", "top")}
            if depth:
                stack["planes"] = ("depth",)
            sim, act = make(stack)
            m = windows(sim, act)
            close(sim, act)
            kern, nb = m[0] - b[0], push_bytes(esize, depth)
            res[name] = (kern, nb, (m[2] - m[1]) / kern)
            print(f"  round {rnd}  {dtype:8s} {name:7s} stack kernel  {m[0]:8.3f} ({m[1]:.3f} {m[2]:.3f})  kernel {kern:7.3f} ms  {nb / 1e9:7.2f} GB  {nb / kern / 1e9:5.2f} TB/s = "
                  f"{100 * nb / (kern * 1e-3) / HBM_PEAK:4.1f} % of the HBM peak   window spread {100 * res[name][2]:4.1f} % of the kernel", flush=True)
        if what == "parent":
            continue
        (kc, bc, sc), (kd, bd, _) = res["colour"], res["rgb-d"]
        print(f"  round {rnd}  {dtype:8s} rgb-d / colour: bytes x{bd / bc:5.3f}, measured x{kd / kc:5.3f}  (spread of the colour stack {100 * sc:4.1f} %)", flush=True)
        import torch

        sim, act = make(None)
        update, st = torch_stacker(sim, dtype)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        tm = windows(sim, act, extra=update)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - held
        tk = tm[0] - b[0]
        print(f"  round {rnd}  {dtype:8s} rgb-d   torch ops     {tm[0]:8.3f} ({tm[1]:.3f} {tm[2]:.3f})  ops    {tk:7.3f} ms  x{tk / kd:5.2f} of the rgb-d kernel  "
              f"peak extra memory {peak / 1e9:6.2f} GB beside a stack of {st['stack'].numel() * esize / 1e9:.2f} GB", flush=True)
        del update, st
        close(sim, act)
        torch.cuda.empty_cache()
