"""What the surface-normals kernel costs (profiles/surface_normals.txt): every configuration in ONE process, one after the other, so that the kernel, the frame kernel that
feeds it and the object-boxes kernel beside it are timed in the same run, on the same frames.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python tools/surface_normals_times.py run N OUT/lines.json
    python tools/surface_normals_times.py report OUT

`run`: for every entry of CONFIGS a StackTwoCubes handle of N envs, H x W frames, both planes, front + top, world-frame normals and the default object boxes.  Three
steps of random actions, then LAUNCHES masked no-op resets: each launches the frame kernel, the boxes kernel and the normals kernel behind it on the handle's stream.
Writes one JSON line per configuration, in order, with the bytes the normals kernel moves per launch -- 1 B read per pixel of the two segmentation planes, 16 B of depth read per quad of four pixels that holds a box
pixel, 4 B written per pixel -- counted on the host from the planes of the first SAMPLE envs.
`report`: the trace's normals dispatches in time order are 1 (enabling) + 3 (steps) + LAUNCHES per configuration; the frame kernel and the boxes kernel of a launch are
the last ones that started before its normals kernel.  Median (min max) of the last LAUNCHES of each, and each kernel's achieved rate over the bytes it moves (the frame
kernel: the 16 B per pixel it writes for two cameras -- 3 B of colour, 4 B of depth, 1 B of segmentation each; the boxes kernel: the 1 B per pixel it reads)."""
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
# H, W
CONFIGS = [(240, 320), (84, 84)]


def run(n, path):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecsim import DeviceArray

    lines = []
    for H, W in CONFIGS:
        sim = VecSim("stack", n, observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"),
                     object_boxes=dict(cameras=("front", "top")), surface_normals=dict(cameras=("front", "top")))
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
        box_pixels = box_quads = 0.0
        for cam in ("front", "top"):
            ids = DeviceArray(sim, getattr(sim, "seg_" + cam).ptr, (m, H * W // 4, 4), np.uint8).numpy() & 0x7F
            box = (ids >= 2) & (ids <= 10)
            box_pixels += float(box.sum()) / m
            box_quads += float(box.any(axis=2).sum()) / m
        out = {"H": H, "W": W, "n": n, "box_pixels_per_env": box_pixels, "quads_with_a_box_pixel_per_env": box_quads, "quads_per_env": 2 * H * W // 4,
               "read_bytes_per_env": 2 * H * W + 16 * box_quads, "written_bytes_per_env": 2 * H * W * 4, "frame_written_bytes_per_env": 16 * H * W,
               "boxes_read_bytes_per_env": 2 * H * W}
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
    normals, boxes, frames = [], [], []
    with open(traces[0]) as f:
        for r in csv.DictReader(f):
            span = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
            if "lcr_normals_kernel" in r["Kernel_Name"]:
                normals.append(span)
            elif "lcr_object_boxes_kernel" in r["Kernel_Name"]:
                boxes.append(span)
            elif "lcr_render_obs_kernel" in r["Kernel_Name"]:
                frames.append(span)
    normals.sort(); boxes.sort(); frames.sort()
    assert len(normals) == PER_CONFIG * len(infos), (len(normals), len(infos))
    for i, info in enumerate(infos):
        mine = normals[i * PER_CONFIG:(i + 1) * PER_CONFIG][-LAUNCHES:]
        # the frame and the boxes kernel of a launch: the last ones that started before the normals kernel did
        feed = [max(f for f in frames if f[0] < b[0]) for b in mine]
        beside = [max(f for f in boxes if f[0] < b[0]) for b in mine]
        assert len(set(feed)) == LAUNCHES and len(set(beside)) == LAUNCHES
        n = info["n"]
        moved = (info["read_bytes_per_env"] + info["written_bytes_per_env"]) * n

        def med(spans):
            ms = [(b - a) * 1e-6 for a, b, _ in spans]
            return statistics.median(ms), min(ms), max(ms)

        nm, fm, bm = med(mine), med(feed), med(beside)
        nrate, frate, brate = moved / (nm[0] * 1e-3), info["frame_written_bytes_per_env"] * n / (fm[0] * 1e-3), info["boxes_read_bytes_per_env"] * n / (bm[0] * 1e-3)
        print(f"{info['H']:3d} x {info['W']:3d}   normals kernel {nm[0]:7.3f} ({nm[1]:7.3f} {nm[2]:7.3f}) ms  moves {moved / 1e9:7.3f} GB  {nrate / 1e12:5.2f} TB/s "
              f"= {nrate / frate:5.2f} of the frame kernel's rate   |   frame kernel {fm[0]:7.3f} ({fm[1]:7.3f} {fm[2]:7.3f}) ms  writes "
              f"{info['frame_written_bytes_per_env'] * n / 1e9:7.3f} GB  {frate / 1e12:5.2f} TB/s   |   boxes kernel {bm[0]:7.3f} ({bm[1]:7.3f} {bm[2]:7.3f}) ms  reads "
              f"{info['boxes_read_bytes_per_env'] * n / 1e9:6.3f} GB  {brate / 1e12:5.2f} TB/s")
        print(f"{'':16s}{json.dumps(info)}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), sys.argv[3])
    else:
        report(sys.argv[2])
