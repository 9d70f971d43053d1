"""The second and later passes of the three terminal-frame calls (lcr_render_terminal, lcr_render_terminal_planes, lcr_render_terminal_wrist; lcr_capi.hip:
render_terminal_passes).  The calls draw the listed envs in passes of at most `cap` envs, as many as keep the frame staging of one pass within 450 MiB, and use the same
staging again for every pass; a frame must be 512 x 512 before a few hundred ids exceed one pass.  At that size the cases list cap + 1 ids (two passes, the last of one
env) and 2 cap + 1 ids (three passes): what can go wrong there -- the pass loop, a shorter last pass in the staging of a longer one, the host pointer `done * frame` -- shows
as a frame in the wrong slot, a stale frame or a torn one.

One handle serves all cases: push, four envs, look (two variants and a sampler), wrist camera, both planes, max_episode_steps = 3 and three seeded steps, so that every env
has just been reset.  The ids alternate between two finished envs a and b whose terminal frames differ, and every pass starts with the other env than the pass before it
did (the caps of two of the three calls are even: a plain a, b, a, b would put into every slot of the staging the env the pass before had left there, and a pass that
returned what it found would go unnoticed).  Every frame of every array a call returns must equal, byte for byte, the slot of its env in what the same call returns for
[a, b] on the same handle: the frame kernels cast one ray per pixel, one env per workgroup at this size, and what
they draw of an env does not depend on its place in the batch.  The references are computed once and left unchanged.

Host memory: the arrays of one case take 0.5 GB (two passes) to 1 GB (three passes); the cases run one after another and each frees its arrays."""
import numpy as np
import pytest

from tests import look_ref
from tests.test_gpu_wrist import BOTH, SAMPLER

pytestmark = pytest.mark.gpu

H, W = SIZE = (512, 512)
N = 4
BUDGET = 450 << 20   # bytes of frame staging per pass (lcr_capi.hip: render_terminal_passes, the driver of the three lcr_render_terminal* calls) -- stated here, not imported
PX = H * W
# bytes of staging per env: front and top colours / colours, depth and segmentation of front and top (the colours are drawn in the same launch) / wrist colours, depth, segmentation
PER_ENV = {"render_terminal": 2 * PX * 3, "render_terminal_planes": 2 * (PX * 3 + PX * 4 + PX), "render_terminal_wrist": PX * 3 + PX * 4 + PX}
CAP = {call: BUDGET // b for call, b in PER_ENV.items()}
KEYS = {"render_terminal": ("front", "top"), "render_terminal_planes": ("depth_front", "depth_top", "segmentation_front", "segmentation_top"),
        "render_terminal_wrist": ("image_wrist", "depth_wrist", "segmentation_wrist")}


def test_the_caps_of_the_three_calls():
    """the arithmetic of the library, at this frame size (needs no device; the marker of the file keeps it with the tests it serves)"""
    assert CAP == {"render_terminal": 300, "render_terminal_planes": 112, "render_terminal_wrist": 225}


def _call(sim, call, ids):
    """every array `call` returns for `ids`, by name"""
    out = getattr(sim, call)(ids)
    if call == "render_terminal":
        out = dict(zip(KEYS[call], out))
    assert tuple(out) == KEYS[call], (call, tuple(out))
    return out


def _raw(a):
    """the bytes of an array as unsigned integers of its element size: float planes are compared as bits"""
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def finished(hip_lib):
    """(sim, a, b, {call: its arrays for [a, b]}): the handle with every env just reset, two envs whose terminal frames differ, the references"""
    from gym_lowcostrobot_amd import VecSim

    sim = VecSim("push", N, observation_mode="both", base_seed=6, max_episode_steps=3, image_size=SIZE, wrist_camera=True, look_variants=look_ref.GPU_VARIANTS[:2],
                 look_sampler=SAMPLER, image_planes=BOTH)
    act = sim.alloc_actions()
    for t in range(3):
        sim.fill_random_actions(act, 9, t); sim.step_device(act.ptr)
    assert sim.did_reset.numpy().all()
    front = sim.render_terminal(np.arange(N, dtype=np.int32))[0]
    pairs = [(a, b) for a in range(N) for b in range(a + 1, N) if (front[a] != front[b]).any()]
    assert pairs, "the terminal front frames of all envs are the same: the alternation below would check nothing"
    a, b = pairs[0]
    ref = {call: _call(sim, call, np.array([a, b], np.int32)) for call in KEYS}
    for call, arrays in ref.items():
        for key, arr in arrays.items():
            assert arr.shape[:3] == (2, H, W), (call, key, arr.shape)
            arr.setflags(write=False)
    yield sim, a, b, ref
    sim.free(act); sim.close()


@pytest.mark.parametrize("passes", (2, 3))
@pytest.mark.parametrize("call", tuple(KEYS))
def test_later_passes_return_the_frames_of_one_pass(finished, call, passes):
    """cap + 1 ids: two passes, the last of one env; 2 cap + 1 ids: three"""
    sim, a, b, ref = finished
    cap = CAP[call]
    count = (passes - 1) * cap + 1
    i = np.arange(count)
    which = (i % cap + i // cap) % 2   # 0: env a, 1: env b -- alternating inside a pass, and slot j of the staging holds the other env in the next pass
    ids = np.where(which == 0, a, b).astype(np.int32)
    got = _call(sim, call, ids)
    for key in KEYS[call]:
        out, want = _raw(got[key]), _raw(ref[call][key])
        assert out.shape == (count,) + want.shape[1:], (call, key, out.shape)
        for slot in (0, 1):
            at = np.nonzero(which == slot)[0]
            same = (out[at] == want[slot]).reshape(len(at), -1).all(axis=1)
            wrong = at[~same].tolist()
            assert not wrong, f"{call}[{key}], {count} ids in passes of {cap}: frames {wrong[:8]} ({len(wrong)} in all) are not the frame of env {(a, b)[slot]}"
    del got
