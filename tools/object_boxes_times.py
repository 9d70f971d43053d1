"""What the object-boxes kernel costs (profiles/object_boxes.txt): every configuration in ONE process, one after the other, so that the kernel and the frame kernel that
feeds it are timed in the same run, on the same frames.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python tools/object_boxes_times.py run N OUT/lines.json
    python tools/object_boxes_times.py report OUT
    rocprofv3 --pmc COUNTERS --kernel-trace --output-format csv -d OUT2 -o c -- python tools/object_boxes_times.py run N OUT2/lines.json
    python tools/object_boxes_times.py counters OUT2

`run`: for every entry of CONFIGS a StackTwoCubes handle of N envs, H x W frames, both planes, front + top, the default objects (arm, cube, cube2, marker), with and without
`depth`.  Three steps of random actions, then LAUNCHES masked no-op resets: each launches the frame kernel and the boxes kernel behind it on the handle's stream.  Writes one
JSON line per configuration, in order, with the bytes the kernel must read per launch -- 1 B per pixel of the two segmentation planes and, with depth, 4 B per pixel that
matches one of the objects -- and the bytes it does load for them (64 B of depth per 16-pixel chunk with a matching pixel), counted on the host from the planes of the first
SAMPLE envs.
`report`: the trace's boxes dispatches in time order are 1 (enabling) + 3 (steps) + LAUNCHES per configuration; the frame kernel of a launch is the last one that started
before its boxes kernel.  Median (min max) of the last LAUNCHES of each, the frame kernel's achieved rate over the 16 B per pixel it writes (two cameras: 3 B of colour, 4 B
of depth, 1 B of segmentation) as the yardstick, and the boxes kernel's rate over the bytes it must read as a share of it.
`counters`: the mean of every counter per boxes dispatch, per configuration, over the last LAUNCHES (a run of its own: counters are not collected in the timed run)."""
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAUNCHES, SAMPLE = 40, 64
PER_CONFIG = 1 + 3 + LAUNCHES
# H, W, depth
CONFIGS = [(240, 320, False), (240, 320, True), (84, 84, False), (84, 84, True)]


def run(n, path):
    from gym_lowcostrobot_amd import VecSim, _capi
    from gym_lowcostrobot_amd.vecsim import DeviceArray

    lines = []
    for H, W, depth in CONFIGS:
        sim = VecSim("stack", n, observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"),
                     object_boxes=dict(cameras=("front", "top"), depth=depth))
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
        union = 0
        for o in sim.object_boxes_spec["masks"]:
            union |= o
        matching = chunks = 0.0
        for cam in ("front", "top"):
            seg = DeviceArray(sim, getattr(sim, "seg_" + cam).ptr, (m, H * W // 16, 16), np.uint8).numpy()
            hit = ((union >> (seg & 0x7F).astype(np.int64)) & 1).astype(bool) | (bool(union & _capi.BOXES_MARKER) & ((seg & 0x80) != 0))
            matching += float(hit.sum()) / m
            chunks += float(hit.any(axis=2).sum()) / m
        rec = DeviceArray(sim, sim.object_boxes.ptr, (m, 2, 4, 8), np.int32).numpy()
        out = {"H": H, "W": W, "depth": depth, "n": n, "matching_pixels_per_env": matching, "chunks_with_a_match_per_env": chunks, "chunks_per_env": 2 * H * W // 16,
               "nonempty_records_per_env": float((rec[..., 4] > 0).sum()) / m, "must_read_bytes_per_env": 2 * H * W + (4 * matching if depth else 0),
               "loaded_bytes_per_env": 2 * H * W + (64 * chunks if depth else 0), "written_bytes_per_env": 2 * 4 * 8 * 4, "frame_written_bytes_per_env": 16 * H * W}
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        sim.free(act)
        sim.close()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def report(out_dir):
    traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    with open(os.path.join(out_dir, "lines.json")) as f:
        infos = [json.loads(l) for l in f if l.startswith("{")]
    boxes, frames = [], []
    with open(traces[0]) as f:
        for r in csv.DictReader(f):
            span = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
            if "lcr_object_boxes_kernel" in r["Kernel_Name"]:
                boxes.append(span)
            elif "lcr_render_obs_kernel" in r["Kernel_Name"]:
                frames.append(span)
    boxes.sort(); frames.sort()
    assert len(boxes) == PER_CONFIG * len(infos), (len(boxes), len(infos))
    for i, info in enumerate(infos):
        mine = boxes[i * PER_CONFIG:(i + 1) * PER_CONFIG][-LAUNCHES:]
        # the frame kernel of a launch: the last one that started before the boxes kernel did
        feed = [max(f for f in frames if f[0] < b[0]) for b in mine]
        assert len(set(feed)) == LAUNCHES
        bms = [(b - a) * 1e-6 for a, b, _ in mine]
        fms = [(b - a) * 1e-6 for a, b, _ in feed]
        bmed, fmed = statistics.median(bms), statistics.median(fms)
        n = info["n"]
        frate = info["frame_written_bytes_per_env"] * n / (fmed * 1e-3)
        brate = info["must_read_bytes_per_env"] * n / (bmed * 1e-3)
        lrate = info["loaded_bytes_per_env"] * n / (bmed * 1e-3)
        print(f"{info['H']:3d} x {info['W']:3d} depth {int(info['depth'])}   frame kernel {fmed:7.3f} ({min(fms):7.3f} {max(fms):7.3f}) ms  {info['frame_written_bytes_per_env'] * n / 1e9:7.3f} GB "
              f"written  {frate / 1e12:5.2f} TB/s   |   boxes kernel {bmed:7.3f} ({min(bms):7.3f} {max(bms):7.3f}) ms  must read {info['must_read_bytes_per_env'] * n / 1e9:6.3f} GB "
              f"{brate / 1e12:5.2f} TB/s = {brate / frate:5.2f} of the frame kernel's rate (loads {info['loaded_bytes_per_env'] * n / 1e9:6.3f} GB: {lrate / 1e12:5.2f} TB/s)   "
              f"time {bmed / fmed:5.3f} of the frame kernel's")
        print(f"{'':24s}{json.dumps(info)}")


def counters(out_dir):
    found = glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True)
    with open(os.path.join(out_dir, "lines.json")) as f:
        infos = [json.loads(l) for l in f if l.startswith("{")]
    vals = {}
    with open(found[0]) as f:
        for r in csv.DictReader(f):
            if "lcr_object_boxes_kernel" in r["Kernel_Name"]:
                vals.setdefault(r["Counter_Name"], {}).setdefault(int(r["Dispatch_Id"]), 0.0)
                vals[r["Counter_Name"]][int(r["Dispatch_Id"])] += float(r["Counter_Value"])
    for counter, by_dispatch in sorted(vals.items()):
        v = [by_dispatch[d] for d in sorted(by_dispatch)]
        assert len(v) == PER_CONFIG * len(infos), (counter, len(v))
        means = [statistics.mean(v[i * PER_CONFIG:(i + 1) * PER_CONFIG][-LAUNCHES:]) for i in range(len(infos))]
        print(f"{counter:24s} " + "  ".join(f"{i['H']}x{i['W']} d{int(i['depth'])} {m:15.1f}" for i, m in zip(infos, means)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), sys.argv[3])
    elif sys.argv[1] == "counters":
        counters(sys.argv[2])
    else:
        report(sys.argv[2])
