"""What the motion-vector kernel costs beside the normals kernel (profiles/motion_vectors.txt): both on ONE handle, under random actions, in one process, so that the two
kernels stream the same planes of the same steps.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python tools/motion_vectors_times.py run OUT/lines.json
    python tools/motion_vectors_times.py report OUT

`run`: for every entry of CONFIGS a StackTwoCubes handle of n envs, H x W frames, both planes, front + top, world-frame normals and motion vectors.  WARM + STEPS steps of
random actions; only a step measures, so every one of them runs the chain on the pixels of whatever moved.  Writes one JSON line per configuration with the bytes each
kernel moves per launch -- 1 B read per pixel of the two segmentation planes, 16 B of depth per quad of four pixels that holds a box pixel (normals) or a pixel that runs the
chain (motion vectors), 4 B written per pixel -- counted on the host from the planes and the history of the first SAMPLE envs after the last step.
`report`: each kernel's dispatches in time order are 1 (enabling) + WARM + STEPS per configuration; median (min max) of the last STEPS."""
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, STEPS, SAMPLE = 3, 20, 64
PER_CONFIG = 1 + WARM + STEPS
# n, H, W
CONFIGS = [(32768, 84, 84), (4096, 240, 320)]


def run(path):
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.vecsim import DeviceArray
    from tests import flow_ref

    lines = []
    for n, H, W in CONFIGS:
        sim = VecSim("stack", n, observation_mode="both", image_size=(H, W), image_planes=("depth", "segmentation"),
                     surface_normals=dict(cameras=("front", "top")), motion_vectors=dict(cameras=("front", "top")))
        act = sim.alloc_actions()
        for t in range(WARM + STEPS):
            sim.fill_random_actions(act, 1, t)
            sim.step_device(act.ptr)
        sim.sync()
        m = min(SAMPLE, n)
        boxes = sim.flow_boxes.numpy()[..., :m]
        poses = sim.flow_pose.numpy()[..., :m]
        valid = sim.flow_valid.numpy()[:m].astype(bool)
        box_quads = chain_quads = chain_pixels = box_pixels = 0.0
        for slot, cam in enumerate(("front", "top")):
            ids = DeviceArray(sim, getattr(sim, "seg_" + cam).ptr, (m, H * W // 4, 4), np.uint8).numpy() & 0x7F
            box = (ids >= 2) & (ids <= 10)
            box_static, cam_static = flow_ref.static(boxes, poses[:, slot])
            b = np.clip(ids.astype(np.int64) - 2, 0, 8)
            env = np.arange(m)[:, None, None]
            runs = valid[:, None, None] & (((ids == 1) & ~cam_static[env]) | (box & ~(box_static[b, env] & cam_static[env])))
            box_pixels += float(box.sum()) / m; box_quads += float(box.any(axis=2).sum()) / m
            chain_pixels += float(runs.sum()) / m; chain_quads += float(runs.any(axis=2).sum()) / m
        out = {"H": H, "W": W, "n": n, "valid_share": float(valid.mean()), "box_pixels_per_env": box_pixels, "chain_pixels_per_env": chain_pixels,
               "quads_with_a_box_pixel_per_env": box_quads, "quads_with_a_chain_pixel_per_env": chain_quads, "quads_per_env": 2 * H * W // 4,
               "normals_bytes_per_env": 2 * H * W + 16 * box_quads + 2 * H * W * 4, "flow_bytes_per_env": 2 * H * W + 16 * chain_quads + 2 * H * W * 4}
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
    spans = {"lcr_normals_kernel": [], "lcr_flow_kernel": [], "lcr_render_obs": []}
    with open(traces[0]) as f:
        for r in csv.DictReader(f):
            for key in spans:
                if key in r["Kernel_Name"]:
                    spans[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for v in spans.values():
        v.sort()
    assert len(spans["lcr_normals_kernel"]) == len(spans["lcr_flow_kernel"]) == PER_CONFIG * len(infos), {k: len(v) for k, v in spans.items()}

    def med(s):
        ms = [(b - a) * 1e-6 for a, b in s]
        return statistics.median(ms), min(ms), max(ms)

    for i, info in enumerate(infos):
        nm = med(spans["lcr_normals_kernel"][i * PER_CONFIG:(i + 1) * PER_CONFIG][-STEPS:])
        fm = med(spans["lcr_flow_kernel"][i * PER_CONFIG:(i + 1) * PER_CONFIG][-STEPS:])
        nb, fb = info["normals_bytes_per_env"] * info["n"], info["flow_bytes_per_env"] * info["n"]
        print(f"{info['n']:6d} x {info['H']:3d} x {info['W']:3d}   normals kernel {nm[0]:7.3f} ({nm[1]:7.3f} {nm[2]:7.3f}) ms  moves {nb / 1e9:7.3f} GB  {nb / nm[0] / 1e9:5.2f} TB/s   |   "
              f"motion-vector kernel {fm[0]:7.3f} ({fm[1]:7.3f} {fm[2]:7.3f}) ms  moves {fb / 1e9:7.3f} GB  {fb / fm[0] / 1e9:5.2f} TB/s   |   ratio {fm[0] / nm[0]:5.2f}")
        print(f"{'':16s}{json.dumps(info)}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        report(sys.argv[2])
