"""Is the window between lcr_step and the end of its frames visible to a reader on the handle's stream?  (GPU box)   python tools/stream_order_window.py [--envs 4096] [--streams 8]
The control of tests/test_gpu_stream_order.py WITHOUT its arming: a fresh all-on handle per line, the seeded rollout of that file, clones of four envs of every buffer taken
behind each step with no join, counted stale when they differ from the LCR_RENDER_OVERLAP=0 reference.  First on the default stream, then on --streams fresh torch streams in
turn.  The count is all or nothing per line: it follows which hardware queue the runtime gave the handle's frame stream and the caller's stream (profiles/stream_order.txt)."""
import argparse
import os
import sys

sys.path.insert(0, ".")
os.environ["LCR_PRESET"] = "fast"
import pytest  # noqa: E402
import torch  # noqa: E402

import tests.test_gpu_stream_order as m  # noqa: E402
from gym_lowcostrobot_amd import VecSim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=m.N_ENVS)
ap.add_argument("--streams", type=int, default=8)
args = ap.parse_args()
m.N_ENVS = args.envs
with pytest.MonkeyPatch.context() as mp:
    want = m._reference_rollout(mp, m.ALL_ON, m.BUFFERS)
rows = len(m._idx(args.envs))
for i in range(1 + args.streams):
    sim = VecSim("push", args.envs, **m.ALL_ON)
    act = sim.alloc_actions()
    stream = torch.cuda.Stream(device=sim.device) if i else None
    if stream is not None:
        sim.set_stream(stream.cuda_stream)
    for t in range(m.PROBES):   # (the steps the tests spend on their probes)
        sim.fill_random_actions(act, m.SEED, t); sim.step_device(act.ptr)
    unjoined = []
    sim.timer_begin()
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(None):
        got = m._joined_rollout(sim, act, m.BUFFERS, sim.wait_frames, unjoined=unjoined)
    ms = sim.timer_end()
    stale = {b: sum(int((unjoined[s][b][r] != m._bytes(want[s][b])[r]).any()) for s in range(m.STEPS) for r in range(rows)) for b in m.BUFFERS}
    wrong = sum(int((got[s][b][r] != m._bytes(want[s][b])[r]).any()) for s in range(m.STEPS) for r in range(rows) for b in m.BUFFERS)
    name = "default stream" if stream is None else f"torch stream {i}"
    print(f"{args.envs} envs, {name}: unjoined reads stale {sum(stale.values())} of {m.STEPS * rows * len(m.BUFFERS)} (obs_stack {stale['obs_stack']}, image_wrist {stale['image_wrist']}, "
          f"image_front {stale['image_front']}), joined reads wrong {wrong}; {m.STEPS} steps with their reads {ms:.2f} ms on the device", flush=True)
    sim.free(act); sim.close()
