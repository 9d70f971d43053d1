"""What the heightmap kernel costs (profiles/heightmap.txt): every configuration in ONE process, one after the other, so that the map and the voxel grid it is compared
with are timed in the same run, on the same frames, cameras and ids.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python tools/heightmap_times.py run N H W OUT/lines.json
    python tools/heightmap_times.py report OUT
    rocprofv3 --pmc COUNTERS --output-format csv -d OUT2 -o c -- python tools/heightmap_times.py run N H W OUT2/lines.json 64
    python tools/heightmap_times.py counters OUT2

`run`: for every entry of CONFIGS a StackTwoCubes handle of N envs, H x W frames, both planes, front + top, default ids, over BOX: the map at 64 x 64 and 128 x 128 cells,
height only and with rgb, with one and with four rounds of the scan in flight (LCR_HEIGHTMAP_ROUNDS, set here before the handle is made) and as the launcher chooses, and
the voxel grid at 16^3 (the cell count of 64 x 64), float32, occupancy only and with rgb.  Three steps of random actions, then LAUNCHES masked no-op resets: each launches the
frame kernel and the handle's map (grid) kernel on the handle's stream.  Writes one JSON line per configuration, in order, with the bytes the kernel reads and writes per
launch, counted on the host from the planes of the first SAMPLE envs: the segmentation bytes, 64 B of depth per 16-pixel group that holds a candidate by id (a map in slabs
reads the planes once per slab), 3 B of colour per filled cell, and the output.
`report`: the trace's map and grid dispatches in time order are 1 (enabling) + 3 (steps) + LAUNCHES per configuration; median (min max) of the last LAUNCHES of each, and
bytes over time against the achievable HBM rate.
A trailing `64` restricts `run` to the grid and the 64 x 64 map as the launcher builds them (the comparison at an equal cell count), for a run that collects counters:
`counters` prints the mean of every counter per dispatch for each kernel of such a run (a kernel's name tells grid from map and height only from rgb)."""
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
PER_CONFIG = 1 + 3 + LAUNCHES
HBM_ACHIEVABLE = 6.3e12   # bytes / s (MI355X: 8 TB/s peak, about 6.3 achievable with a streaming copy)
# what, cells a side (the map) or voxels a side (the grid), rgb, rounds in flight (None: the launcher's choice)
CONFIGS = [("grid", 16, False, None), ("grid", 16, True, None)]
CONFIGS += [("map", d, rgb, r) for d in (64, 128) for rgb in (False, True) for r in (None, 1, 4)]


def run(n, H, W, path, only=None):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecsim import DeviceArray

    lines = []
    for what, d, rgb, rounds in CONFIGS:
        if only and (rounds or (what == "map" and d != only)):
            continue
        kw = dict(observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"))
        os.environ.pop("LCR_HEIGHTMAP_ROUNDS", None)
        if what == "grid":
            kw["voxel_grid"] = dict(box=BOX, dims=(d, d, d), cameras=("front", "top"), features=("occupancy", "rgb") if rgb else ("occupancy",), dtype="float32")
        else:
            if rounds:
                os.environ["LCR_HEIGHTMAP_ROUNDS"] = str(rounds)
            kw["heightmap"] = dict(box=BOX, dims=(d, d), cameras=("front", "top"), features=("height", "rgb") if rgb else ("height",))
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
        C = 4 if rgb else 1
        out = {"what": what, "cells_a_side": d, "rgb": rgb, "rounds": rounds or "auto", "n": n, "H": H, "W": W, "groups_with_candidates_per_env": groups}
        if what == "grid":
            filled = float(DeviceArray(sim, sim.voxel_grid_occupied.ptr, (m,), np.int32).numpy().mean())
            count = float(DeviceArray(sim, sim.voxel_grid_count.ptr, (m,), np.int32).numpy().mean())
            passes, cells = 1, d ** 3
        else:
            filled = float(DeviceArray(sim, sim.heightmap_filled.ptr, (m,), np.int32).numpy().mean())
            count = float(DeviceArray(sim, sim.heightmap_count.ptr, (m,), np.int32).numpy().mean())
            passes, cells = -(-d * d // 8192), d * d
        out.update(filled_per_env=filled, count_per_env=count, passes=passes, read_bytes_per_env=passes * (2 * H * W + 64 * groups) + (3 * filled if rgb else 0),
                   written_bytes_per_env=4 * C * cells + 8 + 2 * 13 * 4)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        sim.free(act)
        sim.close()
    os.environ.pop("LCR_HEIGHTMAP_ROUNDS", None)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def report(out_dir):
    traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    with open(os.path.join(out_dir, "lines.json")) as f:
        infos = [json.loads(l) for l in f if l.startswith("{")]
    spans = []
    with open(traces[0]) as f:
        for r in csv.DictReader(f):
            if "heightmap" in r["Kernel_Name"] or "voxel_grid" in r["Kernel_Name"]:
                spans.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    spans.sort()
    assert len(spans) == PER_CONFIG * len(infos), (len(spans), len(infos))
    for i, info in enumerate(infos):
        mine = spans[i * PER_CONFIG:(i + 1) * PER_CONFIG]
        names = {s[2] for s in mine}
        assert len(names) == 1, names
        ms = [(b - a) * 1e-6 for a, b, _ in mine[-LAUNCHES:]]
        med = statistics.median(ms)
        rd, wr = info["read_bytes_per_env"] * info["n"], info["written_bytes_per_env"] * info["n"]
        rate = (rd + wr) / (med * 1e-3)
        tag = f"{info['what']} {info['cells_a_side']:3d} {'rgb' if info['rgb'] else 'h  '} rounds {info['rounds']}"
        print(f"{tag:26s} {names.pop()[:70]:70s} {med:7.3f} ({min(ms):7.3f} {max(ms):7.3f}) ms   read {rd / 1e9:6.3f} GB  written {wr / 1e9:6.3f} GB   "
              f"{rate / 1e12:5.2f} TB/s = {100 * rate / HBM_ACHIEVABLE:4.1f} % of {HBM_ACHIEVABLE / 1e12:.1f}")
        print(f"{'':26s} {json.dumps(info)}")


def counters(out_dir):
    found = glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True)
    vals = {}
    with open(found[0]) as f:
        for r in csv.DictReader(f):
            if "heightmap" in r["Kernel_Name"] or "voxel_grid" in r["Kernel_Name"]:
                vals.setdefault((r["Kernel_Name"], r["Counter_Name"]), []).append(float(r["Counter_Value"]))
    for (name, counter), v in sorted(vals.items()):
        v = v[-LAUNCHES:]
        print(f"{name[:70]:70s} {counter:28s} {len(v):3d} dispatches   mean {statistics.mean(v):16.1f}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], int(sys.argv[6]) if len(sys.argv) > 6 else None)
    elif sys.argv[1] == "counters":
        counters(sys.argv[2])
    else:
        report(sys.argv[2])
