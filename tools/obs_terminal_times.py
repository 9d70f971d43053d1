"""Terminal observation stacks and clouds (VecSim(obs_stack=dict(..., terminal=True)), obs_stack_terminal(), point_cloud_terminal()): what keeping the history costs the
stack kernel, and what the terminal calls cost beside render_terminal.
    python tools/obs_terminal_times.py [steps|calls|all] [n_envs] [task] [H W]        (default all 32768 stack 84 84; cameras front + top, K = 4)
    LCR_LIB_PATH=<a build of the parent commit> python tools/obs_terminal_times.py parent ...      (the sims the parent has: no stack, the stack)
steps  frames and stack on the caller's stream (LCR_RENDER_OVERLAP=0), preset fast, uint8 and float32.  As in tools/obs_stack_times.py the library has no entry point that
       launches the stack kernel by itself: a kernel time here is the DIFFERENCE of the median step time of a sim with the stack and of one without, device events.
       (a) an ordinary push step: windows of ten steps in which no episode runs out of time (every window starts from elapsed = 0).
       (b) the step on which every env is reset (elapsed = 49 set beforehand): that one step between two events, seven times.
       Bytes from the shapes, per element of a frame: a push reads 1 source byte and K - 1 elements and writes K; a refill reads 1 byte and writes K; the save adds K - 1
       elements read and K - 1 written.
calls  (c) after a step that reset every env: render_terminal, obs_stack_terminal and point_cloud_terminal for all envs, host clock (the calls are synchronous and end in
       host memory), three times each; the float32 stack for the first 8 192 envs only (its terminal stacks of all 32 768 are 22 GB of host memory)."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

args = sys.argv[1:]
what = args[0] if len(args) > 0 else "all"
n = int(args[1]) if len(args) > 1 else 32768
task = args[2] if len(args) > 2 else "stack"
H, W = (int(args[3]), int(args[4])) if len(args) > 4 else (84, 84)
CAMS, K = 2, 4
WINDOWS, PER, RESETS = 5, 10, 7
HBM_PEAK = 8.0e12


def make(stack, **more):
    from gym_lowcostrobot_amd import VecSim

    os.environ["LCR_RENDER_OVERLAP"] = "0"
    sim = VecSim(task, n, observation_mode="both", image_size=(H, W), preset="fast", **({"obs_stack": stack} if stack else {}), **more)
    os.environ.pop("LCR_RENDER_OVERLAP", None)
    act = [sim.alloc_actions() for _ in range(8)]
    for t, a in enumerate(act):
        sim.fill_random_actions(a, 1, t)
    for t in range(20):   # warm
        sim.step_device(act[t % 8].ptr)
    sim.sync()
    return sim, act


def close(sim, act):
    for a in act:
        sim.free(a)
    sim.close()


def push_windows(sim, act):
    w = []
    for _ in range(WINDOWS):
        sim.set_state(elapsed=np.zeros(n, np.int32))
        sim.timer_begin()
        for t in range(PER):
            sim.step_device(act[t % 8].ptr)
        w.append(sim.timer_end() / PER)
    return float(np.median(w)), min(w), max(w)


def reset_steps(sim, act):
    w = []
    for r in range(RESETS):
        for t in range(K):
            sim.step_device(act[t % 8].ptr)
        sim.set_state(elapsed=np.full(n, 49, np.int32))
        sim.timer_begin()
        sim.step_device(act[r % 8].ptr)
        w.append(sim.timer_end())
        assert sim.outputs()["did_reset"].all()
    return float(np.median(w)), min(w), max(w)


def spec(dtype, terminal):
    d = {"frames": K, "dtype": dtype, "cameras": ("front", "top")}
    if terminal:
        d["terminal"] = True
    return d


def gb(elements_read, elements_written, esize, source=1):
    return n * CAMS * 3 * H * W * (source + (elements_read + elements_written) * esize) / 1e9


print(f"terminal observations: {task}, {n} envs, {H} x {W}, cameras front + top, K = {K}; library {os.environ.get('LCR_LIB_PATH', 'of this tree')}")
if what in ("steps", "all", "parent"):
    kinds = [("stack", False)] + ([] if what == "parent" else [("stack, terminal", True)])
    print(f"(a) push step / (b) all-reset step: ms per step, median (min max); kernel = difference to the sim without a stack of the same round")
    for rnd in (1, 2):
        sim, act = make(None)
        bp, br = push_windows(sim, act), reset_steps(sim, act)
        close(sim, act)
        print(f"  round {rnd}  no stack                 push {bp[0]:7.3f} ({bp[1]:.3f} {bp[2]:.3f})   all-reset {br[0]:7.3f} ({br[1]:.3f} {br[2]:.3f})", flush=True)
        for dtype in ("uint8", "float32"):
            es = np.dtype(dtype).itemsize
            for name, term in kinds:
                sim, act = make(spec(dtype, term))
                mp, mr = push_windows(sim, act), reset_steps(sim, act)
                close(sim, act)
                kp, kr = mp[0] - bp[0], mr[0] - br[0]
                pb, rb = gb(K - 1, K, es), gb(K - 1 if term else 0, K + (K - 1 if term else 0), es)
                print(f"  round {rnd}  {dtype:7s} {name:16s} push {mp[0]:7.3f} ({mp[1]:.3f} {mp[2]:.3f}) kernel {kp:6.3f} ms {pb:6.2f} GB {pb / kp:5.2f} TB/s   "
                      f"all-reset {mr[0]:7.3f} ({mr[1]:.3f} {mr[2]:.3f}) kernel {kr:6.3f} ms {rb:6.2f} GB {rb / kr:5.2f} TB/s = {100 * rb * 1e9 / (kr * 1e-3) / HBM_PEAK:4.1f} % of the HBM peak", flush=True)

if what in ("calls", "all"):
    print("(c) the terminal calls after a step that reset every env: seconds, host clock, three calls each (min median max)")

    def timed(f):
        w = []
        for _ in range(3):
            t0 = time.perf_counter()
            f()
            w.append(time.perf_counter() - t0)
        return f"{min(w):7.3f} {float(np.median(w)):7.3f} {max(w):7.3f}"

    for dtype, listed in (("uint8", n), ("float32", min(n, 8192))):
        sim, act = make(spec(dtype, True), image_planes=("depth", "segmentation"), point_cloud=dict(points=512, terminal=True))
        sim.set_state(elapsed=np.full(n, 49, np.int32))
        sim.step_device(act[0].ptr)
        assert sim.outputs()["did_reset"].all()
        ids = np.arange(listed, dtype=np.int32)
        out_gb = listed * K * CAMS * 3 * H * W * np.dtype(dtype).itemsize / 1e9
        print(f"  {dtype}: render_terminal({listed})          {timed(lambda: sim.render_terminal(ids))} s   ({listed * 2 * 3 * H * W / 1e9:.2f} GB to the host)", flush=True)
        print(f"  {dtype}: obs_stack_terminal({listed})       {timed(lambda: sim.obs_stack_terminal(ids))} s   ({out_gb:.2f} GB to the host)", flush=True)
        if dtype == "uint8":
            print(f"  {dtype}: render_terminal_planes({listed})   {timed(lambda: sim.render_terminal_planes(ids))} s   ({listed * 2 * 5 * H * W / 1e9:.2f} GB to the host)", flush=True)
            print(f"  {dtype}: point_cloud_terminal({listed})     {timed(lambda: sim.point_cloud_terminal(ids))} s   (P = 512, x y z: {listed * 512 * 16 / 1e9:.2f} GB to the host)", flush=True)
        close(sim, act)
