"""The far end of workload-size observation buffers: every observation unit at a batch whose device buffer crosses 2^31 and 2^32 bytes (or 2^31 elements), compared byte
for byte at the envs on both sides of each crossing.

Why.  The product runs with buffers far beyond 4 GiB (32 768 envs of 240 x 320 frames are 7.5 GB a colour array), while every content test of these units runs at
n <= 128.  A kernel, an .inc.h pass, a C-ABI staging path or a carve-out that formed `env * pixels`, `env * P * C` or an offset in 32 bits would pass all of them.

Method, the same for every unit (_far_end):
  1. a big sim of n envs (a multiple of 64) whose buffer under test crosses the stated boundaries;
  2. probe envs: env 0, the env whose slice holds the first byte (element) past each boundary -- it straddles the boundary or starts at it --, its predecessor, env n - 1;
  3. twins for the expected bytes: for every 64-env block with a probe env, VecSim(task, 64, env_id_offset=block, global_envs=n, **the same keywords), stepped with the same
     fill_random_actions(buf, seed, t) over a few steps with an auto-reset (max_episode_steps = 2).  First the twins' get_state() must equal the big sim's slices bit for bit
     (a failure there is a PHYSICS failure: shard invariance is pinned elsewhere); then every device buffer of the probe envs is compared byte for byte, the big sim read
     with VecSim.read_rows, the twin whole after the last step (before it, its larger arrays by rows: the copies are what a test here costs).  The twins run the same
     kernels at low offsets, where the unit tests pin them to the numpy models and the fp64 ray-caster: no new tolerance;
  4. on the colour and plane paths an independent check of the env index: the per-pixel path (render / render_planes of the same far env) against the batched frame, by the
     rule of tests/test_gpu_image_size.py (_raycast_pixels), imported;
  5. the guard regions before and behind the unit's buffer on the big sim still hold their pattern after the rollout;
  6. the terminal passes with the ids [n - 1, 0, the boundary envs] against the twins with the matching local ids, byte for byte.

Memory.  A test needs the sum of nbytes of the observation arrays of its big sim (the stack's history included), computed from the first twin's arrays; it skips, with both
numbers in the reason, only when the device has less than 1.1 x that + 4 GiB free.  No test needs more than 64 GiB.

Not built: the tier at which the ELEMENT index of the depth words crosses 2^32 (n = 16 448 at 512 x 512 with both planes: 70 - 105 GB).  The depth consumers run at n = 8 256,
where the element index crosses 2^31 and the byte offset 2^32 and 2^33.
"""
import time

import numpy as np
import pytest

from tests import look_ref, planes_ref
from tests.test_gpu_cloud import _check_guards as _check_cloud_guards
from tests.test_gpu_image_size import _raycast_pixels
from tests.test_gpu_wrist import SAMPLER, _guards

pytestmark = pytest.mark.gpu

GIB = 1 << 30
CAP = 64 * GIB            # no test may need more
BOTH = ("depth", "segmentation")
WITH_FLOOR = ("arm", "cube", "cube2", "floor")
BIG = (512, 512)          # the largest frame: 2^18 pixels per env and plane
BIG_BOX = ((-0.25, -0.125, 0.0), (0.25, 0.375, 0.5))
CROP_BOX = ((-0.1, -0.05, 0.0), (0.1, 0.2, None))
ENV_LAST = ("point_cloud_pose", "voxel_grid_pose", "heightmap_pose", "normals_boxes", "normals_pose",
            "arm_qpos", "arm_qvel", "cube_pos", "aux_pos", "terminal_obs", "terminal_quat")   # [...][N]: small arrays, read whole
GUARDED = ("image_wrist", "depth_wrist", "segmentation_wrist", "obs_stack", "obs_stack_history", "point_cloud", "voxel_grid", "heightmap", "object_boxes",
           "normals_front", "normals_top", "normals_wrist")


def _obs_arrays(sim):
    """every observation buffer of the sim as {name: DeviceArray}: the frames, planes and every unit's arrays"""
    out = {k: getattr(sim, k) for k in ("image_front", "image_top", "image_wrist") if getattr(sim, k) is not None}
    out.update(sim.plane_arrays())
    names = ["obs_stack", "obs_stack_history", "point_cloud", "point_cloud_count", "point_cloud_source", "point_cloud_pose", "voxel_grid", "voxel_grid_source",
             "voxel_grid_count", "voxel_grid_occupied", "voxel_grid_pose", "heightmap", "heightmap_source", "heightmap_count", "heightmap_filled", "heightmap_pose",
             "object_boxes"]
    if hasattr(sim, "normals_spec"):
        names += ["normals_" + c for c in sim.normals_spec["cameras"]] + ["normals_boxes", "normals_pose"]
    out.update({k: getattr(sim, k) for k in names if getattr(sim, k) is not None})
    return out


def _small_arrays(sim):
    """the state observations and the outputs: (., N) or (N,)"""
    names = ("arm_qpos", "arm_qvel", "cube_pos", "aux_pos", "terminal_obs", "terminal_quat", "reward", "terminated", "truncated", "is_success", "did_reset")
    return {k: getattr(sim, k) for k in names if getattr(sim, k) is not None}


def _room(need, what):
    """the memory rule of the module docstring"""
    import torch

    assert need <= CAP, (what, need)
    free = torch.cuda.mem_get_info(0)[0]
    if free < need * 1.1 + 4 * GIB:
        pytest.skip(f"{what}: needs {need} bytes of device memory (x 1.1 + 4 GiB), the device has {free} free")


def _same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
    assert bad.size == 0, (what, f"{bad.size} bytes differ", bad[:6].tolist())


def _assert_guards(sim, arr, what):
    from gym_lowcostrobot_amd import _capi

    for side, g in zip(("before", "behind"), _guards(sim, arr)):
        assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (what, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())


def _terminal_calls(sim):
    """the terminal passes the sim has, each as ids -> {name: array with the listed envs on axis 0}"""
    calls = {"render_terminal": lambda ids: dict(zip(("front", "top"), sim.render_terminal(ids)))}
    if sim.image_planes:
        calls["render_terminal_planes"] = sim.render_terminal_planes
    if sim.wrist_camera is not None:
        calls["render_terminal_wrist"] = sim.render_terminal_wrist
    if sim.obs_stack is not None and sim.obs_stack_keeps_terminal:
        calls["obs_stack_terminal"] = lambda ids: {"stack": sim.obs_stack_terminal(ids)}
    if sim.point_cloud is not None:
        def cloud(ids):
            out = sim.point_cloud_terminal(ids)
            out["pose"] = np.ascontiguousarray(np.moveaxis(out["pose"], -1, 0))   # (slots, 13, len(ids)) -> the envs first
            return out
        calls["point_cloud_terminal"] = cloud
    return calls


def _per_pixel(big, e, H, W):
    """4. the batched frames and planes of env e against the one-ray-per-pixel path of the same env -> the failures"""
    fails = []
    cams = [("camera_front", "front"), ("camera_top", "top")] + ([("camera_wrist", "wrist")] if big.wrist_camera is not None else [])
    for cam, c in cams:
        got = big.read_rows(getattr(big, "image_" + c), [e])[0]
        ref = big.render(e, cam, W, H)
        assert ref.std() > 5, (e, cam)
        bad = int((np.abs(got.astype(int) - ref.astype(int)).max(-1) > 2).sum())
        if bad > _raycast_pixels(H, W):
            fails.append((e, cam, "colour", bad))
        dep, seg = getattr(big, "depth_" + c), getattr(big, "seg_" + c)
        if dep is None and seg is None:
            continue
        d1, s1 = big.render_planes(e, cam, W, H)
        d = big.read_rows(dep, [e])[0] if dep is not None else d1
        s = big.read_rows(seg, [e])[0] if seg is not None else s1
        bad = int((~planes_ref.agree(d, s, d1, s1, 1e-5)).sum())
        if bad > _raycast_pixels(H, W):
            fails.append((e, cam, "planes", bad))
    return fails


def _far_end(n, kw, crossings, *, steps=3, seed=21, per_pixel=False, look=False, whole=None, task="stack"):
    """the method of the module docstring.  `crossings`: (array name, "bytes" | "elements", boundary), each of which the big sim's array must cross; the probe envs follow
    from them.  `whole`: the name of the one array that is also read whole.  -> what the run contained, for the caller's assertions"""
    from gym_lowcostrobot_amd import VecSim

    assert n % 64 == 0
    kw = dict(observation_mode="both", base_seed=7, max_episode_steps=2, **kw)
    H, W = kw["image_size"]
    sims, seen = [], {"terminals": 0, "resets": 0}

    def twin(block):
        sims.append(VecSim(task, 64, env_id_offset=block, global_envs=n, **kw))
        return sims[-1]

    try:
        twins = {0: twin(0)}
        per_env = {k: a.nbytes // 64 for k, a in _obs_arrays(twins[0]).items()}
        need = sum(per_env.values()) * n
        _room(need, f"n = {n}")
        probes, boundary = {0, n - 1}, []
        for name, unit, bound in crossings:
            a = _obs_arrays(twins[0])[name]
            per = per_env[name] // (a.dtype.itemsize if unit == "elements" else 1)
            e = bound // per           # the env that holds the first byte (element) past the boundary: it straddles the boundary or starts at it
            assert 0 < e < n - 1 and per * n > bound, (name, unit, bound, per, n)
            probes |= {e - 1, e}
            boundary.append(e)
        probes = sorted(probes)
        t0 = time.perf_counter()
        big = VecSim(task, n, **kw)
        sims.append(big)
        seen["build_s"] = time.perf_counter() - t0   # (printed: allocating tens of GiB is where a run of these tests can stall)
        arrays = _obs_arrays(big)
        assert sum(a.nbytes for a in arrays.values()) == need and list(arrays) == list(per_env)
        for name, unit, bound in crossings:
            assert arrays[name].nbytes // (arrays[name].dtype.itemsize if unit == "elements" else 1) > bound, (name, unit, bound)
        for b in sorted({e // 64 * 64 for e in probes} - {0}):
            twins[b] = twin(b)
        print(f"[far end] n {n}, {H}x{W}: {need / GIB:.1f} GiB of observation arrays, built in {seen['build_s']:.2f} s; probe envs {probes}; "
              + "; ".join(f"{name} crosses {bound:#x} {unit} at env {e}" for (name, unit, bound), e in zip(crossings, boundary)))
        acts = [(s_, s_.alloc_actions()) for s_ in sims]
        term_ids = [n - 1, 0] + sorted(set(boundary))
        guarded = [k for k in GUARDED if k in arrays]

        for t in range(steps):
            for s_, a in acts:
                s_.fill_random_actions(a, seed, t); s_.step_device(a.ptr)
            when = f"step {t}"
            # 3a. the physics: state, state observations and outputs of every twin are the big sim's slices
            st, small = big.get_state(), {k: a.numpy() for k, a in _small_arrays(big).items()}
            for b, tw in twins.items():
                for k, v in tw.get_state().items():
                    _same_bytes(st[k][..., b:b + 64], v, f"PHYSICS, not an observation: state {k} of block {b}, {when}")
                for k, a in _small_arrays(tw).items():
                    _same_bytes(small[k][..., b:b + 64], a.numpy(), f"PHYSICS, not an observation: {k} of block {b}, {when}")
            # 3b. every observation buffer of the probe envs
            last = {k: arrays[k].numpy() for k in arrays if k in ENV_LAST}
            looks = big.look() if look else None
            for b, tw in twins.items():
                es = [e for e in probes if b <= e < b + 64]
                local = [e - b for e in es]
                for k, a in _obs_arrays(tw).items():
                    if k in ENV_LAST:
                        _same_bytes(last[k][..., es], a.numpy()[..., local], f"{k} of envs {es}, {when}")
                        continue
                    # the twin is read whole after the last step; before it, arrays of more than 16 MiB by rows (the same bytes, a tenth of the copies)
                    want = a.numpy()[local] if t == steps - 1 or a.nbytes <= 16 << 20 else tw.read_rows(a, local)
                    got = big.read_rows(arrays[k], es)
                    for i, e in enumerate(es):
                        _same_bytes(got[i], want[i], f"{k} of env {e}, {when}")
                if look:   # the sampler is keyed by the global env id
                    lt = tw.look()
                    for k in ("variant", "rgb", "episode"):
                        _same_bytes(looks[k][..., b:b + 64], lt[k], f"look {k} of block {b}, {when}")
            # 6. the terminal passes, after a step that ended the episodes of the listed envs
            if big.did_reset.numpy()[term_ids].all():
                seen["resets"] += 1
                got = {name: call(np.asarray(term_ids, np.int32)) for name, call in _terminal_calls(big).items()}
                for b, tw in twins.items():
                    at = [i for i, e in enumerate(term_ids) if b <= e < b + 64]
                    for name, call in _terminal_calls(tw).items() if at else ():
                        want = call(np.asarray([term_ids[i] - b for i in at], np.int32))
                        assert want.keys() == got[name].keys()
                        for k, v in want.items():
                            for j, i in enumerate(at):
                                _same_bytes(got[name][k][i], v[j], f"{name} {k} of env {term_ids[i]}, {when}")
                                seen["terminals"] += 1
                seen["terminal_calls"] = sorted(got)

        # 4. the env index, independently: the per-pixel path of the same far env
        if per_pixel:
            fails = [f for e in probes for f in _per_pixel(big, e, H, W)]
            assert not fails, (f"allowed {_raycast_pixels(H, W):.1f} pixels", fails)
        # the one whole-array copy of the module: a single device-to-host copy of more than 4 GiB
        if whole is not None:
            assert arrays[whole].nbytes > 4 * GIB
            host = arrays[whole].numpy()
            rows = big.read_rows(arrays[whole], probes)
            for i, e in enumerate(probes):
                _same_bytes(host[e], rows[i], f"{whole} of env {e}, read whole against read_rows")
            del host
        # 5. nothing else was written
        for k in guarded:
            _assert_guards(big, arrays[k], f"{k} after the rollout")
        if big.point_cloud is not None:
            _check_cloud_guards(big, "after the rollout")
        seen.update(probes=probes, need=need, guarded=guarded, arrays=list(arrays))
        for s_, a in acts:
            s_.free(a)
    finally:
        for s_ in sims:   # (every sim is closed before the next test builds one)
            s_.close()
    assert seen["resets"] >= 1 and seen["terminals"] > 0, seen
    return seen


@pytest.mark.parametrize("look", [False, True], ids=["plain", "look"])
def test_colour_frames_past_4_gib(hip_lib, look):
    """n = 5 504 at 512 x 512: a colour frame array is 3 x 2^18 B an env, 4.3 GB; env 2 730 straddles 2^31 B and env 5 461 2^32 B.  Front, top and wrist frames, once plain and
    once with two look variants and a sampler (another frame kernel); render_terminal and render_terminal_wrist; the per-pixel path of the far envs"""
    kw = dict(image_size=BIG, wrist_camera=True)
    if look:
        kw.update(look_variants=look_ref.GPU_VARIANTS[:2], look_sampler=SAMPLER)
    seen = _far_end(5504, kw, [(k, "bytes", b) for k in ("image_front", "image_top", "image_wrist") for b in (1 << 31, 1 << 32)], per_pixel=True, look=look)
    assert seen["probes"] == [0, 2729, 2730, 5460, 5461, 5503] and seen["terminal_calls"] == ["render_terminal", "render_terminal_wrist"]


def test_planes_and_wrist_camera_past_4_gib(hip_lib):
    """n = 4 160 at 512 x 512, both planes, wrist camera: a depth plane is 2^20 B an env, 4.4 GB; env 2 048 starts at 2^31 B and env 4 096 at 2^32 B (the segmentation planes
    and the colour frames cross nothing new here).  All three terminal passes of the frames and planes; the guards of the wrist buffers"""
    seen = _far_end(4160, dict(image_size=BIG, image_planes=BOTH, wrist_camera=True),
                    [(k, "bytes", b) for k in ("depth_front", "depth_top", "depth_wrist") for b in (1 << 31, 1 << 32)], per_pixel=True)
    assert seen["probes"] == [0, 2047, 2048, 4095, 4096, 4159] and seen["guarded"] == ["image_wrist", "depth_wrist", "segmentation_wrist"]
    assert seen["terminal_calls"] == ["render_terminal", "render_terminal_planes", "render_terminal_wrist"]


def test_object_boxes_from_segmentation_past_2_32_pixels(hip_lib):
    """n = 16 448 at 512 x 512, the segmentation plane alone, object boxes without depth: a segmentation plane is 2^18 B an env, 4.3 GB, and the kernels' `env * pixels`
    crosses 2^32 at env 16 384.  seg_front is also read whole, in one device-to-host copy of more than 4 GiB.  That copy is most of this test's time, so it runs two steps and
    probes the 2^32 crossing alone: the 2^31 crossing of a segmentation plane, at env 8 192, is probed by every case of test_depth_consumers_past_2_31_elements, with boxes
    in its voxel-boxes case"""
    seen = _far_end(16448, dict(image_size=BIG, image_planes=("segmentation",), object_boxes=dict(depth=False)),
                    [(k, "bytes", 1 << 32) for k in ("segmentation_front", "segmentation_top")], steps=2, per_pixel=True, whole="segmentation_front")
    assert seen["probes"] == [0, 16383, 16384, 16447] and seen["guarded"] == ["object_boxes"]


DEPTH_CONSUMERS = {
    # surface normals of both scene cameras in the camera frame: two more arrays of 4 B a pixel
    "normals": dict(surface_normals=dict(cameras=("front", "top"), frame="camera")),
    # the heightmap beside each kind of cloud (a sim has one cloud): strided, farthest-point sampled, cropped
    "heightmap-cloud": dict(heightmap=dict(box=BIG_BOX, dims=(64, 64), ids=WITH_FLOOR, features=("height", "rgb"), source=True),
                            point_cloud=dict(points=8192, ids=WITH_FLOOR, colors=True, terminal=True)),
    "heightmap-cloud-fps": dict(heightmap=dict(box=BIG_BOX, dims=(64, 64), ids=WITH_FLOOR, features=("height", "rgb"), source=True),
                                point_cloud=dict(points=1024, ids=WITH_FLOOR, colors=True, sampling="fps", pool=4096, terminal=True)),
    "heightmap-cloud-crop": dict(heightmap=dict(box=BIG_BOX, dims=(64, 64), ids=WITH_FLOOR, features=("height", "rgb"), source=True),
                                 point_cloud=dict(points=4096, ids=WITH_FLOOR, colors=True, crop=CROP_BOX, terminal=True)),
    # the voxel grid at small dims and the object boxes with the nearest depth
    "voxel-boxes": dict(voxel_grid=dict(box=BIG_BOX, dims=(16, 16, 8), ids=WITH_FLOOR, features=("occupancy", "rgb"), source=True),
                        object_boxes=dict(depth=True)),
}


@pytest.mark.parametrize("unit", list(DEPTH_CONSUMERS))
def test_depth_consumers_past_2_31_elements(hip_lib, unit):
    """n = 8 256 at 512 x 512 with both planes: the element index of the depth words crosses 2^31 at env 8 192 (their byte offset 2^32 at env 4 096 and 2^33 at env 8 192); every
    consumer applies the same `env * pixels` offset to the depth, the segmentation (2^31 B at env 8 192) and the colours.  The 2^32-element tier is not built (module docstring)"""
    crossings = [(k, "bytes", 1 << 32) for k in ("depth_front", "depth_top")] + [(k, "elements", 1 << 31) for k in ("depth_front", "depth_top")]
    if unit == "normals":
        crossings += [(k, "bytes", b) for k in ("normals_front", "normals_top") for b in (1 << 32, 1 << 33)]   # (a word of four int8 a pixel: 2^31 words are 2^33 B)
    seen = _far_end(8256, dict(image_size=BIG, image_planes=BOTH, **DEPTH_CONSUMERS[unit]), crossings)
    assert seen["probes"] == [0, 4095, 4096, 8191, 8192, 8255]
    assert seen["guarded"] == {"normals": ["normals_front", "normals_top"], "voxel-boxes": ["voxel_grid", "object_boxes"]}.get(unit, ["point_cloud", "heightmap"])
    assert ("point_cloud_terminal" in seen["terminal_calls"]) == ("cloud" in unit)


def test_float32_stack_and_history_past_4_gib(hip_lib):
    """The float32 stack of 3 frames of front + top with the depth channel, terminal stacks kept, at 64 x 64: (K, C, H, W) = (3, 8, 64, 64) is 384 KiB an env and the history
    256 KiB.  n = 16 448 takes the stack past 2^31 B (env 5 461 straddles) and 2^32 B (env 10 922 straddles) and the history past 2^31 B (env 8 192 starts) and 2^32 B
    (env 16 384 starts).  K + 1 steps: the history shifts, and two steps end episodes (a save, a refill with reset_fill = "repeat", obs_stack_terminal)"""
    spec = dict(frames=3, cameras=("front", "top"), dtype="float32", reset_fill="repeat", planes=("depth",), terminal=True)
    seen = _far_end(16448, dict(image_size=(64, 64), image_planes=("depth",), obs_stack=spec),
                    [(k, "bytes", b) for k in ("obs_stack", "obs_stack_history") for b in (1 << 31, 1 << 32)], steps=4)
    assert seen["probes"] == [0, 5460, 5461, 8191, 8192, 10921, 10922, 16383, 16384, 16447] and seen["resets"] == 2
    assert seen["guarded"] == ["obs_stack", "obs_stack_history"] and "obs_stack_terminal" in seen["terminal_calls"]


def test_uint8_stack_past_4_gib(hip_lib):
    """The uint8 stack of 2 frames of front + top at 128 x 128: (2, 6, 128, 128) is 192 KiB an env; n = 21 888 takes it past 2^31 B (env 10 922 straddles) and 2^32 B
    (env 21 845 straddles); its history, one slot, past 2^31 B (env 21 845 straddles).  K + 1 steps"""
    spec = dict(frames=2, cameras=("front", "top"), dtype="uint8", reset_fill="repeat", terminal=True)
    seen = _far_end(21888, dict(image_size=(128, 128), obs_stack=spec),
                    [("obs_stack", "bytes", 1 << 31), ("obs_stack", "bytes", 1 << 32), ("obs_stack_history", "bytes", 1 << 31)], steps=3)
    assert seen["probes"] == [0, 10921, 10922, 21844, 21845, 21887] and seen["guarded"] == ["obs_stack", "obs_stack_history"]


def test_point_cloud_past_4_gib(hip_lib):
    """8 192 points of x y z r g b of all three cameras, ids with the floor, at 16 x 32: 196 608 B an env; n = 21 888 takes the points past 2^31 B (env 10 922 straddles) and
    2^32 B (env 21 845 straddles).  The 32 768-B-an-env source (0.7 GB) crosses nothing here and is compared all the same; point_cloud_terminal"""
    seen = _far_end(21888, dict(image_size=(16, 32), image_planes=BOTH, wrist_camera=True, point_cloud=dict(points=8192, ids=WITH_FLOOR, colors=True, terminal=True)),
                    [("point_cloud", "bytes", 1 << 31), ("point_cloud", "bytes", 1 << 32)])
    assert seen["probes"] == [0, 10921, 10922, 21844, 21845, 21887] and "point_cloud" in seen["guarded"] and "point_cloud_source" in seen["arrays"]
    assert "point_cloud_terminal" in seen["terminal_calls"]


def test_voxel_grid_past_4_gib(hip_lib):
    """The float32 grid of occupancy + r g b at (32, 32, 32) of all three cameras, ids with the floor, with its source, at 16 x 32: 512 KiB an env; n = 8 256 takes it past
    2^31 B (env 4 096 starts) and 2^32 B (env 8 192 starts).  The source (128 KiB an env) crosses nothing here and is compared all the same"""
    grid = dict(box=BIG_BOX, dims=(32, 32, 32), ids=WITH_FLOOR, features=("occupancy", "rgb"), dtype="float32", source=True)
    seen = _far_end(8256, dict(image_size=(16, 32), image_planes=BOTH, wrist_camera=True, voxel_grid=grid), [("voxel_grid", "bytes", 1 << 31), ("voxel_grid", "bytes", 1 << 32)])
    assert seen["probes"] == [0, 4095, 4096, 8191, 8192, 8255] and "voxel_grid" in seen["guarded"] and "voxel_grid_source" in seen["arrays"]


def test_heightmap_past_4_gib(hip_lib):
    """The largest map lcr_heightmap_check accepts, 128 x 128 = 16 384 cells, with r g b and its source, of all three cameras, ids with the floor, at 16 x 32: 256 KiB an
    env; n = 16 448 takes it past 2^31 B (env 8 192 starts) and 2^32 B (env 16 384 starts); the source (64 KiB an env, 1 GB) crosses nothing"""
    hm = dict(box=BIG_BOX, dims=(128, 128), ids=WITH_FLOOR, features=("height", "rgb"), source=True)
    seen = _far_end(16448, dict(image_size=(16, 32), image_planes=BOTH, wrist_camera=True, heightmap=hm), [("heightmap", "bytes", 1 << 31), ("heightmap", "bytes", 1 << 32)])
    assert seen["probes"] == [0, 8191, 8192, 16383, 16384, 16447] and "heightmap" in seen["guarded"] and "heightmap_source" in seen["arrays"]
