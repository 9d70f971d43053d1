"""The observation stack (VecSim(obs_stack=...)): what its kernel costs, against the same result made with torch operations, and what it adds to a step.
    python tools/obs_stack_times.py [n_envs] [task] [H W]        (default 32768 stack 84 84; cameras front + top)
(a) the stack kernel alone, K = 1 and K = 4 in uint8 and float16.  Frames and stack on the caller's stream (LCR_RENDER_OVERLAP=0), preset fast (the cheapest step kernel):
    windows of ten steps timed with device events on a sim without the stack and on one with it, in turn, two rounds.  The library has no entry point that launches the
    stack kernel by itself, so the time printed for it is NOT a directly timed launch: it is the difference of the two medians (ms per step = ms per launch, one launch a step).
    Bytes of a push from the shapes: per element of a frame one source byte read, K - 1 elements read, K elements written; GB / ms = TB/s, as a share of the 8 TB/s HBM peak.
(b) the same stack made with torch operations on the library's frame tensors -- cat, permute, cast (* 1/255), roll, masked refill from did_reset -- timed with device
    events in the same windows (no host synchronisation is added; the masked refill's nonzero() is torch's own), and its peak extra device memory (beyond the stack it keeps).
(c) lcr_step per step, open loop, second stream on, default preset: without and with the stack (K = 4 float16), in turn, two rounds.
(d) of profiles/obs_stack.txt is not made here: it is `bench.py --gpus 1 --steps 200 --warmup 50` itself, run in a checkout of the parent commit and in this tree in turn."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 32768
task = args[1] if len(args) > 1 else "stack"
H, W = (int(args[2]), int(args[3])) if len(args) > 3 else (84, 84)
CAMS = 2
WINDOWS, PER = 7, 10
HBM_PEAK = 8.0e12
CASES = [(1, "uint8"), (4, "uint8"), (1, "float16"), (4, "float16")]


def make(stack, preset, overlap):
    from gym_lowcostrobot_amd import VecSim

    if overlap:
        os.environ.pop("LCR_RENDER_OVERLAP", None)
    else:
        os.environ["LCR_RENDER_OVERLAP"] = "0"
    sim = VecSim(task, n, observation_mode="both", image_size=(H, W), preset=preset, **({"obs_stack": stack} if stack else {}))
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


def push_bytes(K, esize):
    return n * CAMS * 3 * H * W * (1 + (K - 1) * esize + K * esize)


def torch_stacker(sim, K, dtype):
    """the stack kept with torch operations on the library's own frame tensors; returns (update(sim), the state dict that holds the stack)"""
    import torch

    tdt = {"uint8": torch.uint8, "float16": torch.float16}[dtype]
    front, top, did = sim.image_front.torch(), sim.image_top.torch(), sim.did_reset.torch()

    def frame():
        x = torch.cat([front, top], dim=-1).permute(0, 3, 1, 2)
        return x.contiguous() if tdt == torch.uint8 else (x.to(torch.float32) * (1.0 / 255.0)).to(tdt)

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


print(f"observation stack: {task}, {n} envs, {H} x {W}, cameras front + top ({CAMS * 3} channels)")
print(f"(a) the stack kernel alone and (b) the torch path: serial streams, preset fast; ms per step, median of {WINDOWS} windows of {PER} (min max)")
print("    'difference' = that median minus the median of the sim without a stack in the same round: not a directly timed launch")
base_rounds = []
for rnd in (1, 2):
    sim, act = make(None, "fast", overlap=False)
    b = windows(sim, act)
    base_rounds.append(b[0])
    print(f"  round {rnd}  no stack (step + frames)      {b[0]:8.3f} ({b[1]:.3f} {b[2]:.3f})", flush=True)
    close(sim, act)
    for K, dtype in CASES:
        esize = np.dtype(dtype).itemsize
        sim, act = make({"frames": K, "dtype": dtype, "cameras": ("front", "top")}, "fast", overlap=False)
        m = windows(sim, act)
        close(sim, act)
        kern = m[0] - b[0]
        nb = push_bytes(K, esize)
        print(f"  round {rnd}  K = {K} {dtype:8s} fused kernel   {m[0]:8.3f} ({m[1]:.3f} {m[2]:.3f})  kernel (difference) {kern:7.3f} ms  {nb / 1e9:7.2f} GB  "
              f"{nb / kern / 1e9:5.2f} TB/s = {100 * nb / (kern * 1e-3) / HBM_PEAK:4.1f} % of the HBM peak", flush=True)
        # (b) the same result with torch operations, on a sim without the stack
        import torch

        sim, act = make(None, "fast", overlap=False)
        update, st = torch_stacker(sim, K, dtype)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        tm = windows(sim, act, extra=update)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - held
        tk = tm[0] - b[0]
        print(f"  round {rnd}  K = {K} {dtype:8s} torch ops      {tm[0]:8.3f} ({tm[1]:.3f} {tm[2]:.3f})  ops (difference)    {tk:7.3f} ms  x{tk / kern:5.2f} of the fused kernel  "
              f"peak extra memory {peak / 1e9:6.2f} GB beside a stack of {st['stack'].numel() * esize / 1e9:.2f} GB", flush=True)
        del update, st
        close(sim, act)
        torch.cuda.empty_cache()

print(f"(c) lcr_step per step, open loop, second stream, default preset: ms per step over {4 * PER} steps enqueued back to back (host clock, one sync at the end)")
for rnd in (1, 2):
    res = {}
    for name, stack in (("no stack", None), ("K = 4 float16", {"frames": 4, "dtype": "float16", "cameras": ("front", "top")})):
        sim, act = make(stack, None, overlap=True)
        w = []
        for _ in range(5):
            sim.sync()
            t0 = time.perf_counter()
            for t in range(4 * PER):
                sim.step_device(act[t % 8].ptr)
            sim.sync()
            w.append((time.perf_counter() - t0) * 1e3 / (4 * PER))
        res[name] = float(np.median(w))
        print(f"  round {rnd}  {name:14s} {res[name]:8.3f} ms per step (min {min(w):.3f} max {max(w):.3f})  {n / res[name] * 1e3:.3e} env-steps/s", flush=True)
        close(sim, act)
    print(f"  round {rnd}  the stack adds {res['K = 4 float16'] - res['no stack']:.3f} ms to the open-loop step ({100 * (res['K = 4 float16'] / res['no stack'] - 1):.1f} %)")
