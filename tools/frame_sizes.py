"""Image observations at several frame sizes: what the frame kernel and a whole step cost at each.
    python tools/frame_sizes.py [n_envs] [task] [--planes] [--look K[,K...]] [--wrist] [--cloud[=P]] [--cloud-fps=P,Q [--launches]] [--cloud-crop=x0,y0,z0,x1,y1,z1]
For (H, W) in 240x320, 128x128, 84x84, 64x64, default preset, observation_mode "both":
  (i)  the frame kernel alone -- a masked no-op reset re-renders all frames and runs nothing else (tools/render_clocks.py) -- in windows of ten launches after a soak of
       back-to-back launches, timed with device events: median ms, bytes written per launch, TB/s;
  (ii) step + frames, closed loop (a sync after every step, what a policy that reads the frames sees) and open loop (steps enqueued back to back): env-steps/s.
--planes: (i) once more with the depth plane, the segmentation plane and both switched on (VecSim(image_planes=...)): the frame kernel then writes 3 + 4 / 3 + 1 / 3 + 4 + 1 bytes
per pixel, so a store-bound kernel would take 7/3, 4/3 and 8/3 of the plain time; the measured ratio is printed beside that.
--look K[,K...] (e.g. --look 1,8,64): ONLY (i), at 240x320 and 84x84, for the build without a look and with a look of K variants (VecSim(look_variants=...): K different
camera pairs, floors, skies and lights, variants and colours spread over the envs by the sampler): the same bytes are written, what changes is where the untouched bands are copied
from -- K cached background pairs instead of one.
--wrist: ONLY the wrist camera (VecSim(wrist_camera=True), the default mount), at 84x84, 128x128 and 240x320, two rounds of [without, with] in turn: (i) of a sim without it
(the two-camera frame kernel) and of a sim with it (both kernels, back to back on one stream), the wrist kernel's time as the difference of the two, the bytes either kernel
writes per ms; (ii) env-steps/s closed and open loop, without and with the camera.
--cloud[=P]: ONLY the point cloud (VecSim(point_cloud=P), default 1024 points, front + top, arm and cubes, x y z), at the four sizes, two rounds of [without, with] in turn:
(i) of a sim with both planes and no cloud (the frame kernel) and of a sim with the cloud (frame kernel and cloud kernel back to back on one stream), the cloud kernel's
time as the difference of the two, the bytes it reads by the model of DESIGN.md section 3.4 -- one segmentation byte per pixel and camera, and per point the 16 id bytes of
its group again, one depth float (with colours three bytes more) -- and the TB/s that makes.
--cloud-fps=P,Q: ONLY the point cloud by farthest-point sampling (VecSim(point_cloud=dict(points=P, sampling="fps", pool=Q)), front + top, arm and cubes, x y z), at 84x84
and 128x128, two rounds of [without, strided P, FPS P out of Q] in turn: (i) of each, the two cloud kernels' times as differences from the sim without a cloud, the FPS
kernel's N P Q distance updates at ten VALU lane-operations each per second, and that as a share of the VALU peak of 256 CUs x 4 SIMDs x 32 lanes
at 2.4 GHz.  With --launches nothing is timed: per size, twelve steps and forty masked no-op resets on a strided and on an FPS handle -- the launches a kernel trace of
this command is read from.
--cloud-crop=x0,y0,z0,x1,y1,z1 (with --cloud[=P], --cloud-fps=P,Q or both; inf and -inf are open sides): ONLY the cloud inside that crop box of the world frame beside the
cloud without one, at 84x84 and 128x128 -- per mode a handle without a box and one with it, and (i) of each with the cloud kernel's time as the difference from the sim
without a cloud, and the mean M of both: what the box removed.  With --launches nothing is timed, as above: twelve steps and forty masked no-op resets per handle.
LCR_RENDER_EPW=1|2|4 in the environment pins the frame kernel's envs-per-workgroup mapping for the small sizes (A/B of the mappings; default: chosen by frame size)."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

from gym_lowcostrobot_amd import VecSim  # noqa: E402

PLANES = "--planes" in sys.argv
WRIST = "--wrist" in sys.argv
CLOUD = [a for a in sys.argv[1:] if a == "--cloud" or a.startswith("--cloud=")]
CLOUD_FPS = [a for a in sys.argv[1:] if a.startswith("--cloud-fps=")]
CLOUD_CROP = [a for a in sys.argv[1:] if a.startswith("--cloud-crop=")]
CROP = [float(v) for v in CLOUD_CROP[0].split("=")[1].split(",")] if CLOUD_CROP else []
FPS_P, FPS_Q = [int(v) for v in CLOUD_FPS[0].split("=")[1].split(",")] if CLOUD_FPS else (0, 0)
LAUNCHES = "--launches" in sys.argv
CLOUD_P = int(CLOUD[0].split("=")[1]) if CLOUD and "=" in CLOUD[0] else 1024
LOOK = [int(k) for k in sys.argv[sys.argv.index("--look") + 1].split(",")] if "--look" in sys.argv else []
args = [a for i, a in enumerate(sys.argv[1:], 1) if a not in ["--planes", "--look", "--wrist", "--launches"] + CLOUD + CLOUD_FPS + CLOUD_CROP and sys.argv[i - 1] != "--look"]
n = int(args[0]) if len(args) > 0 else 32768
task = args[1] if len(args) > 1 else "stack"
SIZES = [(240, 320), (128, 128), (84, 84), (64, 64)]
SOAK_S, WINDOWS, STEPS = 2.0, 7, 60
print(f"frame sizes: {task}, {n} envs, default preset, LCR_RENDER_EPW={os.environ.get('LCR_RENDER_EPW', '(by frame size)')}")
if not WRIST and not CLOUD and not CLOUD_FPS:
    print(f"{'H x W':>9s} {'frame kernel ms':>16s} {'min':>7s} {'max':>7s} {'GB written':>11s} {'TB/s':>6s} {'closed-loop steps/s':>20s} {'open-loop steps/s':>18s}")
rows = []


def frame_kernel_ms(sim):
    """the frame kernel alone: windows of ten masked no-op resets after a soak -> (median, min, max) ms per launch"""
    mask = np.zeros(n, np.uint8)
    sim.reset(mask=mask); sim.sync()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < SOAK_S:
        for _ in range(20):
            sim.reset(mask=mask)
        sim.sync()
    w = []
    for _ in range(WINDOWS):
        sim.timer_begin()
        for _ in range(10):
            sim.reset(mask=mask)
        w.append(sim.timer_end() / 10)
    return float(np.median(w)), min(w), max(w)


def look_variants(K):
    """K variants, the first the default, the others with cameras, field of view, colours and light of their own (seeded)"""
    rng = np.random.default_rng(1)
    out = [{}]
    for _ in range(K - 1):
        out.append({"cam_dpos": rng.uniform(-0.08, 0.08, (2, 3)), "cam_drot": rng.uniform(-0.1, 0.1, (2, 3)), "fovy_deg": rng.uniform(35.0, 60.0, 2),
                    "floor_rgb": rng.uniform(0.05, 0.6, (2, 3)), "sky_rgb": rng.uniform(0.05, 0.5, 3), "sky_slope": rng.uniform(0.0, 0.4, 3),
                    "ambient": rng.uniform(0.2, 0.5), "diffuse": rng.uniform(0.4, 0.9), "arm_rgb": rng.uniform(0.3, 0.9, 3), "finger_rgb": rng.uniform(0.3, 0.9, 3)})
    return out


if LOOK:
    print(f"frame kernel with a look ({n} envs): ms per launch (median of {WINDOWS} windows of ten), ratio to the build without a look, TB/s written, MB of cached backgrounds")
    for H, W in [(240, 320), (84, 84)]:
        base_ms = None
        for K in [0] + LOOK:
            kw = {} if K == 0 else {"look_variants": look_variants(K), "look_sampler": {"seed": 3, "cube": ([0.1] * 3, [0.9] * 3), "cube2": ([0.1] * 3, [0.9] * 3)}}
            sim = VecSim(task, n, observation_mode="both", image_size=(H, W), **kw)
            act = sim.alloc_actions()
            for t in range(12):   # (the same twelve steps: the same poses under the cameras)
                sim.fill_random_actions(act, 1, t % 8)
                sim.step_device(act.ptr)
            if K:
                assert len(set(sim.look()["variant"].tolist())) == K
            ms, wmin, wmax = frame_kernel_ms(sim)
            base_ms = ms if K == 0 else base_ms
            nbytes = 2 * H * W * 3 * n
            print(f"{H:4d}x{W:<4d} {'no look' if K == 0 else 'K = %2d' % K:>8s} {ms:8.3f} (min {wmin:.3f} max {wmax:.3f})  x{ms / base_ms:.3f}  {nbytes / ms / 1e9:6.2f} TB/s  "
                  f"{max(K, 1) * 2 * H * W * 3 / 1e6:7.2f} MB", flush=True)
            sim.free(act)
            sim.close()
    sys.exit(0)


def loops(sim, act):
    """env-steps/s of step + frames: closed loop (a sync after every step) and open loop (steps enqueued back to back)"""
    sim.sync()
    t0 = time.perf_counter()
    for t in range(STEPS):
        sim.step_device(act[t % 8].ptr)
        sim.sync()
    closed = n * STEPS / (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for t in range(STEPS):
        sim.step_device(act[t % 8].ptr)
    sim.sync()
    return closed, n * STEPS / (time.perf_counter() - t0)


if WRIST:
    print(f"the wrist camera ({n} envs, default mount): ms per launch (median of {WINDOWS} windows of ten; min max), GB / ms = TB/s written, env-steps/s closed / open loop")
    for H, W in [(84, 84), (128, 128), (240, 320)]:
        two = wr = None
        for rnd in (1, 2):
            for on in (False, True):
                sim = VecSim(task, n, observation_mode="both", image_size=(H, W), **({"wrist_camera": True} if on else {}))
                act = [sim.alloc_actions() for _ in range(8)]
                for t, a in enumerate(act):
                    sim.fill_random_actions(a, 1, t)
                for t in range(12):   # (the same twelve steps: the same poses under the cameras)
                    sim.step_device(act[t % 8].ptr)
                ms, wmin, wmax = frame_kernel_ms(sim)
                closed, opened = loops(sim, act)
                nb = 2 * H * W * 3 * n
                if not on:
                    two = ms
                    print(f"{H:4d}x{W:<4d} round {rnd} two-camera kernel        {ms:7.3f} ({wmin:.3f} {wmax:.3f})  {nb / ms / 1e9:5.2f} TB/s   "
                          f"steps/s {closed:.3e} / {opened:.3e}", flush=True)
                else:
                    wr = ms - two
                    print(f"{H:4d}x{W:<4d} round {rnd} two-camera + wrist kernel {ms:7.3f} ({wmin:.3f} {wmax:.3f})  wrist kernel (difference) {wr:6.3f} ms  "
                          f"{nb / 2 / wr / 1e9:5.2f} TB/s   steps/s {closed:.3e} / {opened:.3e}", flush=True)
                for a in act:
                    sim.free(a)
                sim.close()
    sys.exit(0)

if CLOUD_CROP:
    assert len(CROP) == 6 and (CLOUD or CLOUD_FPS), "--cloud-crop takes six numbers and goes with --cloud[=P] and / or --cloud-fps=P,Q"
    box = (tuple(CROP[:3]), tuple(CROP[3:]))
    kinds = [("frame kernel with planes", None)]
    if CLOUD:
        kinds += [(f"+ strided cloud, P {CLOUD_P}", dict(points=CLOUD_P)), (f"+ strided cloud, P {CLOUD_P}, cropped", dict(points=CLOUD_P, crop=box))]
    if CLOUD_FPS:
        fps = dict(points=FPS_P, sampling="fps", pool=FPS_Q)
        kinds += [(f"+ FPS cloud, P {FPS_P} of Q {FPS_Q}", fps), (f"+ FPS cloud, P {FPS_P} of Q {FPS_Q}, cropped", dict(fps, crop=box))]
    print(f"the point cloud inside the crop box {box[0]} .. {box[1]} beside the cloud without one ({n} envs, front + top, arm and cubes, x y z)" +
          ("" if LAUNCHES else f": ms per launch (median of {WINDOWS} windows of ten; min max)"))
    for H, W in [(84, 84), (128, 128)]:
        for rnd in ((1,) if LAUNCHES else (1, 2)):
            base = None
            for name, cloud in kinds[1:] if LAUNCHES else kinds:
                sim = VecSim(task, n, observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"), **({"point_cloud": cloud} if cloud else {}))
                act = sim.alloc_actions()
                for t in range(12):   # (the same twelve steps: the same poses under the cameras)
                    sim.fill_random_actions(act, 1, t % 8)
                    sim.step_device(act.ptr)
                if LAUNCHES:
                    mask = np.zeros(n, np.uint8)
                    for _ in range(40):
                        sim.reset(mask=mask)
                    sim.sync()
                    print(f"{H:4d}x{W:<4d} {name}: 12 steps and 40 masked no-op resets; mean M {float(sim.point_cloud_count.numpy().mean()):.0f}", flush=True)
                else:
                    ms, wmin, wmax = frame_kernel_ms(sim)
                    line = f"{H:4d}x{W:<4d} round {rnd} {name:44s} {ms:8.3f} ({wmin:.3f} {wmax:.3f})"
                    if cloud is None:
                        base = ms
                    else:
                        line += f"  cloud kernel (difference) {ms - base:7.3f} ms; mean M {float(sim.point_cloud_count.numpy().mean()):.0f}"
                    print(line, flush=True)
                sim.free(act)
                sim.close()
    sys.exit(0)

if CLOUD:
    slots, C = 2, 3
    print(f"the point cloud ({n} envs, P = {CLOUD_P}, front + top, arm and cubes, x y z): ms per launch (median of {WINDOWS} windows of ten; min max), GB read by the model, TB/s")
    for H, W in SIZES:
        for rnd in (1, 2):
            base = None
            for on in (False, True):
                sim = VecSim(task, n, observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"), **({"point_cloud": CLOUD_P} if on else {}))
                act = sim.alloc_actions()
                for t in range(12):   # (the same twelve steps: the same poses under the cameras)
                    sim.fill_random_actions(act, 1, t % 8)
                    sim.step_device(act.ptr)
                ms, wmin, wmax = frame_kernel_ms(sim)
                if not on:
                    base = ms
                    print(f"{H:4d}x{W:<4d} round {rnd} frame kernel with planes   {ms:7.3f} ({wmin:.3f} {wmax:.3f})  {2 * H * W * 8 * n / ms / 1e9:5.2f} TB/s written", flush=True)
                else:
                    cl = ms - base
                    mean_m = float(sim.point_cloud_count.numpy().mean())
                    rd = n * (slots * H * W + CLOUD_P * (16 + 4)) + 0.0
                    wr = n * CLOUD_P * (4 * C + 4)
                    print(f"{H:4d}x{W:<4d} round {rnd} frame + cloud kernel       {ms:7.3f} ({wmin:.3f} {wmax:.3f})  cloud kernel (difference) {cl:6.3f} ms = {cl / base:.3f} of the frame kernel  "
                          f"reads {rd / 1e9:6.3f} GB -> {rd / cl / 1e9:5.2f} TB/s read, writes {wr / 1e9:.3f} GB; mean M {mean_m:.0f}", flush=True)
                sim.free(act)
                sim.close()
    sys.exit(0)

if CLOUD_FPS:
    VALU_PEAK = 256 * 4 * 32 * 2.4e9   # lane-operations per second (MI355X_MICROARCH: 157.3 TFLOP/s of fp32 FMAs = 2 x this)
    updates = n * FPS_P * FPS_Q
    kinds = [("frame kernel with planes", None), (f"+ strided cloud, P {FPS_P}", FPS_P), (f"+ FPS cloud, P {FPS_P} of Q {FPS_Q}", dict(points=FPS_P, sampling="fps", pool=FPS_Q))]
    print(f"the point cloud by farthest-point sampling ({n} envs, P = {FPS_P}, Q = {FPS_Q}, front + top, arm and cubes, x y z)" +
          ("" if LAUNCHES else f": ms per launch (median of {WINDOWS} windows of ten; min max)"))
    for H, W in [(84, 84), (128, 128)]:
        for rnd in ((1,) if LAUNCHES else (1, 2)):
            base = None
            for name, cloud in kinds[1:] if LAUNCHES else kinds:
                sim = VecSim(task, n, observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"), **({"point_cloud": cloud} if cloud else {}))
                act = sim.alloc_actions()
                for t in range(12):   # (the same twelve steps: the same poses under the cameras)
                    sim.fill_random_actions(act, 1, t % 8)
                    sim.step_device(act.ptr)
                if LAUNCHES:
                    mask = np.zeros(n, np.uint8)
                    for _ in range(40):
                        sim.reset(mask=mask)
                    sim.sync()
                    print(f"{H:4d}x{W:<4d} {name}: 12 steps and 40 masked no-op resets; mean M {float(sim.point_cloud_count.numpy().mean()):.0f}", flush=True)
                else:
                    ms, wmin, wmax = frame_kernel_ms(sim)
                    line = f"{H:4d}x{W:<4d} round {rnd} {name:34s} {ms:8.3f} ({wmin:.3f} {wmax:.3f})"
                    if cloud is None:
                        base = ms
                    else:
                        line += f"  cloud kernel (difference) {ms - base:7.3f} ms; mean M {float(sim.point_cloud_count.numpy().mean()):.0f}"
                    if isinstance(cloud, dict):
                        line += f"  {updates / 1e9:.1f} G updates x 10 lane-ops -> {10 * updates / (ms - base) / 1e9:.2f} T lane-ops/s = {100 * 10 * updates / ((ms - base) * 1e-3) / VALU_PEAK:.1f} % of the VALU peak"
                    print(line, flush=True)
                sim.free(act)
                sim.close()
    sys.exit(0)

plane_rows = []
for H, W in SIZES:
    sim = VecSim(task, n, observation_mode="both", image_size=(H, W))
    assert sim.image_size == (H, W)
    act = [sim.alloc_actions() for _ in range(8)]
    for t, a in enumerate(act):
        sim.fill_random_actions(a, 1, t)
    for t in range(12):
        sim.step_device(act[t % 8].ptr)
    nbytes = 2 * H * W * 3 * n
    ms, wmin, wmax = frame_kernel_ms(sim)
    w = [wmin, wmax]
    sim.sync()
    t0 = time.perf_counter()
    for t in range(STEPS):
        sim.step_device(act[t % 8].ptr)
        sim.sync()
    closed = n * STEPS / (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for t in range(STEPS):
        sim.step_device(act[t % 8].ptr)
    sim.sync()
    opened = n * STEPS / (time.perf_counter() - t0)
    rows.append((H, W, ms))
    print(f"{H:4d}x{W:<4d} {ms:16.3f} {min(w):7.3f} {max(w):7.3f} {nbytes / 1e9:11.3f} {nbytes / ms / 1e9:6.2f} {closed:20.3e} {opened:18.3e}", flush=True)
    for a in act:
        sim.free(a)
    sim.close()
    for planes, bpp in ((("depth",), 7), (("segmentation",), 4), (("depth", "segmentation"), 8)) if PLANES else ():
        sim = VecSim(task, n, observation_mode="both", image_size=(H, W), image_planes=planes)
        act = sim.alloc_actions()
        for t in range(12):   # (the same twelve steps: the same poses under the cameras)
            sim.fill_random_actions(act, 1, t % 8)
            sim.step_device(act.ptr)
        pms, pmin, pmax = frame_kernel_ms(sim)
        plane_rows.append((H, W, "+".join(planes), pms, pmin, pmax, pms / ms, bpp / 3, 2 * H * W * bpp * n, 2 * H * W * (bpp - 3)))
        sim.free(act)
        sim.close()
base = rows[0][2]
for H, W, ms in rows[1:]:
    print(f"  {H}x{W}: {ms / base:.3f} of the 240x320 kernel's time for {H * W / (240 * 320):.3f} of its bytes" + ("" if ms < base else "   <-- NOT faster than 240x320"))
if PLANES:
    print(f"frame kernel with planes ({n} envs): ms per launch, ratio to the plain kernel of the same size beside the ratio of the bytes written, TB/s, plane bytes per env")
    for H, W, name, pms, pmin, pmax, ratio, bytes_ratio, nb, per_env in plane_rows:
        print(f"{H:4d}x{W:<4d} {name:>19s} {pms:8.3f} (min {pmin:.3f} max {pmax:.3f})  x{ratio:.2f} of plain (bytes x{bytes_ratio:.2f})  {nb / pms / 1e9:6.2f} TB/s  {per_env:8d} B/env of planes")
