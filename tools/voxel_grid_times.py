"""What the voxel-grid kernel costs (profiles/voxel_grid.txt): one configuration per process, so that a kernel trace of the process holds one build of one kernel.

    rocprofv3 --kernel-trace --output-format csv -d OUT/<tag> -o t -- python tools/voxel_grid_times.py run N H W grid16|grid32|cloud
    python tools/voxel_grid_times.py report OUT

`run`: StackTwoCubes, N envs, H x W frames, both planes, front + top, default ids; the grid over BOX as uint8 occupancy + rgb at 16^3 or 32^3 (LCR_VOXEL_LDS=big|slab in the
environment chooses how 32^3 is held), or -- the yardstick, which reads the same planes -- the strided cloud inside BOX with P = 1024 and colours.  Three steps of random
actions, then LAUNCHES masked no-op resets: each launches the frame kernel and the handle's grid (cloud) kernel on the handle's stream.  Prints one JSON line with the bytes the
kernel reads and writes per launch, counted on the host from the planes of the first SAMPLE envs: the segmentation bytes, 64 B of depth per 16-pixel group that holds a
candidate by id, 3 B of colour per occupied voxel, the grid itself (a z-slab build reads the planes once per slab).
`report`: median (min max) of the last LAUNCHES dispatches of the grid / cloud kernel of every trace under OUT, and bytes over time against the achievable HBM rate."""
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = ((-0.25, -0.125, 0.0), (0.25, 0.375, 0.5))
LAUNCHES, SAMPLE = 40, 64
HBM_ACHIEVABLE = 6.3e12   # bytes / s (MI355X: 8 TB/s peak, about 6.3 achievable with a streaming copy)


def run(n, H, W, what):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecsim import DeviceArray

    kw = dict(observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"))
    D = {"grid16": 16, "grid32": 32}.get(what)
    if D:
        kw["voxel_grid"] = dict(box=BOX, dims=(D, D, D), cameras=("front", "top"), features=("occupancy", "rgb"))
    else:
        kw["point_cloud"] = dict(points=1024, cameras=("front", "top"), colors=True, crop=BOX)
    sim = VecSim("stack", n, **kw)
    act = sim.alloc_actions()
    for t in range(3):
        sim.fill_random_actions(act, 1, t)
        sim.step_device(act.ptr)
    sim.sync()
    mask = np.zeros(n, np.uint8)
    for _ in range(LAUNCHES):
        sim.reset(mask=mask)
    sim.sync()
    m = min(SAMPLE, n)
    groups = 0.0
    for cam in ("front", "top"):
        seg = DeviceArray(sim, getattr(sim, "seg_" + cam).ptr, (m, H * W // 16, 16), np.uint8).numpy() & 0x7F
        groups += float(((seg >= 2) & (seg <= 10)).any(axis=2).sum()) / m
    out = {"what": what, "n": n, "H": H, "W": W, "lds": os.environ.get("LCR_VOXEL_LDS", "default"), "groups_with_candidates_per_env": groups}
    if D:
        occ = float(DeviceArray(sim, sim.voxel_grid_occupied.ptr, (m,), np.int32).numpy().mean())
        passes = 2 if D == 32 and out["lds"] == "slab" else 1
        out.update(occupied_per_env=occ, count_per_env=float(DeviceArray(sim, sim.voxel_grid_count.ptr, (m,), np.int32).numpy().mean()), passes=passes,
                   read_bytes_per_env=passes * (2 * H * W + 64 * groups) + 3 * occ, written_bytes_per_env=4 * D ** 3 + 8 + 2 * 13 * 4)
    else:
        P = 1024
        out.update(count_per_env=float(DeviceArray(sim, sim.point_cloud_count.ptr, (m,), np.int32).numpy().mean()),
                   read_bytes_per_env=2 * H * W + 64 * groups + P * (16 + 64 + 3), written_bytes_per_env=P * (24 + 4) + 4 + 2 * 13 * 4)
    print(json.dumps(out), flush=True)
    sim.free(act)
    sim.close()


def report(out_dir):
    for tag in sorted(os.listdir(out_dir)):
        traces = glob.glob(os.path.join(out_dir, tag, "**", "*kernel_trace.csv"), recursive=True)
        line = os.path.join(out_dir, tag, "line.json")
        if not traces or not os.path.exists(line):
            continue
        with open(line) as f:
            info = json.loads([l for l in f if l.startswith("{")][-1])
        rows = {}
        with open(traces[0]) as f:
            for r in csv.DictReader(f):
                rows.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        for name, spans in sorted(rows.items()):
            if "voxel" not in name and "point_cloud" not in name and "render_obs" not in name:
                continue
            ms = [(b - a) * 1e-6 for a, b in sorted(spans)[-LAUNCHES:]]
            med = statistics.median(ms)
            text = f"{tag:28s} {name[:78]:78s} {len(spans):4d} launches   {med:7.3f} ({min(ms):7.3f} {max(ms):7.3f}) ms"
            if "render_obs" not in name:
                rd, wr = info["read_bytes_per_env"] * info["n"], info["written_bytes_per_env"] * info["n"]
                rate = (rd + wr) / (med * 1e-3)
                text += f"   read {rd / 1e9:6.3f} GB  written {wr / 1e9:6.3f} GB   {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_ACHIEVABLE:4.1f} % of {HBM_ACHIEVABLE / 1e12:.1f}"
            print(text)
        print(f"{tag:28s} {json.dumps(info)}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        report(sys.argv[2])
