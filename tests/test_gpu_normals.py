"""The surface normals on the GPU (VecSim(..., surface_normals=True | dict(cameras=, frame=)); lcr_enable_normals): the library's device planes against the numpy model of
tests/normals_ref.py, which is fed the library's own depth and segmentation planes, `normals_boxes` and `normals_pose` read back.

What is exact: every byte of every plane.  The rule is pinned to the bit (include/lcr.h: "Surface normals"), so each plane is compared exactly, after enabling and after
every step of seeded random actions, and the guard regions around every plane are read back at the end of each rollout.

Each rollout ASSERTS the regime it is there for, so a case that never reaches it fails:
  stack   n = 70 (a ragged second wave of envs), 36 x 52 (W no multiple of 16), front + top + wrist, world frame, 55 steps: every env auto-resets; ids 9 and 10 are both
          seen; at least three different face codes are seen on a cube over the rollout; the wrist plane is seen both with and without a cube.
  push    n = 5 at 16 x 20 and at 20 x 16 (a frame smaller than a workgroup), camera frame, 6 steps: pixels with the marker bit carry the normal of the surface under
          the marker.
  reach   n = 3 at the default 240 x 320, 1 step; n = 64 at 84 x 84, 3 steps.
  look    reach, n = 5 at 32 x 32 with two look variants that turn the cameras, camera frame: the two variants give different bytes for the same floor.

What is geometry: `normals_boxes` (float32 forward kinematics) against oracle.render_oracle.scene (fp64) within 1e-6, and the face against the entry face of the oracle's
slab test at box pixels where the library's id equals tests/planes_ref.py's and the margin (the largest e minus the second largest) is at least 4 x 1e-4 x depth: 1e-4 is
the planes test's own relative depth tolerance, the factor 4 covers depth error along an oblique ray.  At most 5 % of the box pixels may be left out.  Checked first on the
CPU (the model on the fp32 twin's planes of the 8 seed-17 states, both cameras): stack 64 x 64 leaves out 124 of 7 578 box pixels (1.6 %), push 84 x 84 146 of 12 107
(1.2 %), no face differs among the rest.
On an MI355X the rollouts gave (every byte equal to the model's in all of them): stack 3 920 env-checks, all 70 envs auto-reset, ids 0 .. 10 seen, all six face codes on
a cube, the wrist plane with a cube in 688 env-checks and without in 3 232; push 16 x 20 371 and 20 x 16 379 pixels under the marker (one of them on a box), two
different floor words (two cameras, camera frame); default 84 522 box pixels; many 444 947.  Geometry: the boxes within 1.6e-7 of the oracle's, the same 124 of 7 578 and
146 of 12 107 box pixels below the margin as on the CPU, no face differs among the rest.
"""
import functools

import numpy as np
import pytest

from tests import normals_ref

pytestmark = pytest.mark.gpu

ALL = ("front", "top", "wrist")
# name, task, n, size (H, W), cameras, frame, steps
ROLLOUTS = [
    ("stack", "stack", 70, (36, 52), ALL, "world", 55),
    ("push", "push", 5, (16, 20), ("front", "top"), "camera", 6),
    ("push", "push", 5, (20, 16), ("front", "top"), "camera", 6),
    ("default", "reach", 3, None, ("front", "top"), "world", 1),
    ("many", "reach", 64, (84, 84), ("front", "top"), "world", 3),
]
ROLLOUT_IDS = [f"{r[0]}-{r[1]}-n{r[2]}-" + ("default" if r[3] is None else f"{r[3][0]}x{r[3][1]}") for r in ROLLOUTS]
ATTRS = ("normals_front", "normals_top", "normals_wrist", "normals_spec", "normals_boxes", "normals_pose")


def _kw(size, wrist, **more):
    kw = dict(observation_mode="both", image_planes=("depth", "segmentation"), wrist_camera=True if wrist else None, **more)
    if size is not None:
        kw["image_size"] = size
    return kw


def _check(sim, when):
    """the invariant: every plane is the header's function of the env's current planes, boxes and pose, exactly -> {camera: (plane, seg, table index)}"""
    sp = sim.normals_spec
    boxes, poses = sim.normals_boxes.numpy(), sim.normals_pose.numpy()
    assert boxes.shape == (9, 15, sim.n) and poses.shape == (len(sp["cameras"]), 13, sim.n) and np.isfinite(boxes).all() and np.isfinite(poses).all()
    out = {}
    for slot, cam in enumerate(sp["cameras"]):
        depth, seg = getattr(sim, "depth_" + cam).numpy(), getattr(sim, "seg_" + cam).numpy()
        want, index, _ = normals_ref.planes(depth, seg, boxes, poses[slot], sp["frame"], detail=True)
        got = getattr(sim, "normals_" + cam).numpy()
        assert got.shape == want.shape == seg.shape + (4,) and got.dtype == np.int8
        bad = np.argwhere((got != want).any(axis=-1))
        assert bad.size == 0, (when, cam, len(bad), bad[:6].tolist(), [(got[tuple(b)].tolist(), want[tuple(b)].tolist(), int(seg[tuple(b)])) for b in bad[:6]])
        out[cam] = (got, seg, index)
    return out


def _check_guards(sim, when):
    from gym_lowcostrobot_amd import _capi
    from tests.test_gpu_wrist import _guards

    for cam in sim.normals_spec["cameras"]:
        for side, g in zip(("before", "behind"), _guards(sim, getattr(sim, "normals_" + cam))):
            assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (when, cam, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())


@functools.lru_cache(maxsize=None)
def _rollout(case):
    """runs one rollout, checking the invariant after enabling and after every step -> the regime counters"""
    from gym_lowcostrobot_amd import VecSim

    name, task, n, size, cams, frame, steps = case
    sim = VecSim(task, n, base_seed=17, surface_normals=dict(cameras=cams, frame=frame), **_kw(size, "wrist" in cams))
    assert sim.normals_spec == {"cameras": cams, "frame": frame}
    act = sim.alloc_actions()
    was_reset = np.zeros(n, bool)
    st = {"checks": 0, "box_pixels": 0, "ids": set(), "cube_faces": set(), "wrist_with_cube": 0, "wrist_without_cube": 0, "marked": 0, "marked_on_box": 0, "floor_words": set()}
    for t in range(-1, steps):
        if t >= 0:
            sim.fill_random_actions(act, 23, t); sim.step_device(act.ptr)
            was_reset |= sim.outputs()["did_reset"].astype(bool)
        planes = _check(sim, f"step {t}")
        st["checks"] += n
        for cam, (got, seg, index) in planes.items():
            ids = seg & 0x7F
            st["ids"] |= set(np.unique(ids).tolist())
            st["box_pixels"] += int((ids >= 2).sum())
            cube = (ids == 9) | (ids == 10)
            st["cube_faces"] |= set(np.unique(got[..., 3][cube]).tolist())
            assert (got[ids == 0] == 0).all() and (got[..., 3][ids == 1] == 5).all() and ((got[..., 3][ids >= 2] >= 1) & (got[..., 3][ids >= 2] <= 6)).all()
            st["floor_words"] |= set(np.unique(got.view(np.uint32)[..., 0][ids == 1]).tolist())   # (the four bytes of a pixel as one little-endian word)
            if frame == "world":
                assert (got[ids == 1] == (0, 0, 127, 5)).all()
            if cam == "wrist":
                with_cube = cube.reshape(n, -1).any(axis=1)
                st["wrist_with_cube"] += int(with_cube.sum()); st["wrist_without_cube"] += int((~with_cube).sum())
            marked = (seg & 0x80) != 0
            if marked.any():   # the marker bit is ignored: the word is that of the same plane with the bit cleared
                depth = getattr(sim, "depth_" + cam).numpy()
                slot = cams.index(cam)
                plain = normals_ref.planes(depth, ids.astype(np.uint8), sim.normals_boxes.numpy(), sim.normals_pose.numpy()[slot], frame)
                np.testing.assert_array_equal(got[marked], plain[marked])
                st["marked"] += int(marked.sum()); st["marked_on_box"] += int((marked & (ids >= 2)).sum())
    _check_guards(sim, "after the rollout")
    obs = sim.observations()
    for cam in cams:
        np.testing.assert_array_equal(obs["normals_" + cam], getattr(sim, "normals_" + cam).numpy())
    st["all_reset"] = bool(was_reset.all()); st["resets"] = int(was_reset.sum())
    sim.free(act); sim.close()
    print(f"normals rollout {ROLLOUT_IDS[ROLLOUTS.index(case)]}: " + str({k: (sorted(v) if isinstance(v, set) else v) for k, v in st.items()}))
    return st


@pytest.mark.parametrize("case", ROLLOUTS, ids=ROLLOUT_IDS)
def test_every_plane_equals_the_model_after_every_step(hip_lib, case):
    st = _rollout(case)
    name = case[0]
    assert st["checks"] == case[2] * (case[6] + 1) and st["box_pixels"] > 0
    if name == "stack":
        assert st["all_reset"], st                                         # every env auto-resets within the rollout
        assert {9, 10} <= st["ids"], st                                    # both cubes are seen
        assert len(st["cube_faces"]) >= 3, st                              # a tumbling cube shows different faces
        assert st["wrist_with_cube"] > 0 and st["wrist_without_cube"] > 0, st
        assert st["marked"] == 0                                           # StackTwoCubes has no marker
    if name == "push":
        assert st["marked"] > 0, st                                        # the marker bit is exercised and ignored
    if case[5] == "world":
        assert st["floor_words"] == {0x057F0000}                           # (0, 0, 127, 5), low byte first


def test_two_look_variants_turn_the_cameras_and_the_floor_follows(hip_lib):
    """camera frame with per-env cameras: an env's planes are in the axes of ITS variant's cameras, so the same floor has different bytes in the two variants"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 5, (32, 32)
    # (turned about HORIZONTAL axes: a turn about the world's z leaves the z component of every camera axis, which is all the floor's normal sees, where it was)
    variants = [{}, {"cam_dpos": [[0.03, 0.0, 0.02], [0.0, 0.04, 0.05]], "cam_drot": [[0.2, 0.0, 0.0], [0.0, 0.25, 0.0]], "fovy_deg": [50.0, 40.0]}]
    sim = VecSim("reach", n, base_seed=5, look_variants=variants, surface_normals=dict(frame="camera"), **_kw(size, False))
    variant = (np.arange(n) % 2).astype(np.int32)
    sim.set_look(variant=variant, rgb=np.random.default_rng(1).uniform(0, 1, (9, n)).astype(np.float32))
    act = sim.alloc_actions()
    for t in range(-1, 2):
        if t >= 0:
            sim.fill_random_actions(act, 3, t); sim.step_device(act.ptr)
        planes = _check(sim, f"step {t}")
        pose = sim.normals_pose.numpy()
        assert all((pose[:, :, e] == pose[:, :, e % 2]).all() for e in range(n)) and (pose[:, 3:12, 0] != pose[:, 3:12, 1]).any()
        for cam, (got, seg, _) in planes.items():
            words = []
            for e in range(n):
                floor = got[e][(seg[e] & 0x7F) == 1]
                assert len(floor) > 0 and (floor == floor[0]).all() and floor[0, 3] == 5
                words.append(tuple(floor[0].tolist()))
            assert words[0] == words[2] == words[4] and words[1] == words[3] and words[0] != words[1], (cam, words)
    _check_guards(sim, "after the steps")
    sim.free(act); sim.close()


@pytest.mark.parametrize("task,size", [("stack", (64, 64)), ("push", (84, 84))], ids=["stack-64x64", "push-84x84"])
def test_boxes_and_faces_against_the_oracle(hip_lib, task, size):
    """geometry: the boxes the kernel used are the oracle's within 1e-6, and the face is the oracle's entry face wherever the ids agree and the margin is at least
    4 x 1e-4 x depth; at most 5 % of the box pixels are left out"""
    from gym_lowcostrobot_amd import VecSim
    from tests import planes_ref
    from tests.test_image_planes_abi import _states
    from tests.test_normals_abi import CAMS, entry_face, oracle_boxes, oracle_pose

    H, W = size
    n = 8
    qpos, target = _states(task, n)
    sim = VecSim(task, n, base_seed=3, surface_normals=True, **_kw(size, False))
    sim.set_state(qpos=qpos, target=target)
    sim.reset(mask=np.zeros(n, np.uint8))            # no env reset, but re-renders the frames from the new state
    planes = _check(sim, "the seed-17 states")
    boxes = sim.normals_boxes.numpy()
    n_box = n_out = n_bad = 0
    worst = 0.0
    for e in range(n):
        ref = oracle_boxes(task, qpos[:, e], target[:, e])
        worst = max(worst, float(np.abs(boxes[:, :, e].astype(np.float64) - ref).max()))
        for cam, name in zip(("front", "top"), CAMS):
            got, seg, _ = planes[cam]
            depth = getattr(sim, "depth_" + cam).numpy()
            _, seg_ref = planes_ref.planes(task, qpos[:, e], target[:, e], name, W, H)
            pose = oracle_pose(task, name, H)
            np.testing.assert_allclose(sim.normals_pose.numpy()[("front", "top").index(cam), :, e], pose, rtol=0, atol=1e-6)
            _, _, margin = normals_ref.planes(depth[e][None], seg[e][None], boxes[:, :, e][:, :, None], sim.normals_pose.numpy()[("front", "top").index(cam), :, e][:, None], "world", detail=True)
            want = entry_face(seg[e], ref, pose, H, W)
            box = (want > 0) & (seg[e] & 0x7F == seg_ref & 0x7F)
            clear = margin[0] >= np.float32(4 * 1e-4) * depth[e]
            n_box += int(box.sum()); n_out += int((box & ~clear).sum())
            n_bad += int((box & clear & (got[e][..., 3] != want)).sum())
    print(f"[normals vs oracle] {task} {H}x{W}: boxes within {worst:.2e} of the oracle's; {n_box} box pixels with the oracle's id, {n_out} ({n_out / max(n_box, 1):.4f}) below the "
          f"margin, {n_bad} faces differ among the rest")
    sim.close()
    assert worst <= 1e-6
    assert n_box > 0 and n_bad == 0
    assert n_out <= 0.05 * n_box


def test_off_means_off(hip_lib):
    """a handle without surface_normals has none of the attributes, and its colour frames, planes and object boxes are byte-equal to those of a handle with them after the
    same seeded steps"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 6, (36, 52)
    kw = _kw(size, True, base_seed=11, object_boxes=dict(depth=True))
    off, on = VecSim("push", n, **kw), VecSim("push", n, surface_normals=dict(frame="camera"), **kw)
    for a in ATTRS:
        assert not hasattr(off, a), a
        assert hasattr(on, a), a
    assert not any(k.startswith("normals") for k in off.observations())
    acts = [a.alloc_actions() for a in (off, on)]
    for t in range(4):
        for s_, act in zip((off, on), acts):
            s_.fill_random_actions(act, 9, t); s_.step_device(act.ptr)
        for key in ("image_front", "image_top", "image_wrist", "depth_front", "depth_top", "depth_wrist", "seg_front", "seg_top", "seg_wrist", "object_boxes"):
            a, b = getattr(off, key).numpy(), getattr(on, key).numpy()
            assert a.tobytes() == b.tobytes(), (t, key)
        _check(on, f"step {t}")
    _check_guards(on, "after the steps")
    for s_, act in zip((off, on), acts):
        s_.free(act); s_.close()


def test_two_shards_equal_one_handle(hip_lib):
    """ShardedVecSim, two shards of 64, against one handle of 128 with the same seeds"""
    from gym_lowcostrobot_amd import VecSim
    from gym_lowcostrobot_amd.sharding import ShardedVecSim

    size = (36, 52)
    kw = _kw(size, False, base_seed=4, surface_normals=True)
    one = VecSim("stack", 128, **kw)
    two = ShardedVecSim("stack", 128, [0, 0], **kw)
    assert all(s_.normals_front.shape == (64, 36, 52, 4) and s_.normals_spec == one.normals_spec for s_ in two.shards)
    act = one.alloc_actions()
    for t in range(-1, 3):
        if t >= 0:
            one.fill_random_actions(act, 7, t); one.step_device(act.ptr)
            two.fill_random_actions(7, t); two.step_device()
        for cam in ("front", "top"):
            whole = getattr(one, "normals_" + cam).numpy()
            parts = np.concatenate([getattr(s_, "normals_" + cam).numpy() for s_ in two.shards])
            np.testing.assert_array_equal(whole, parts)
        np.testing.assert_array_equal(one.normals_boxes.numpy(), np.concatenate([s_.normals_boxes.numpy() for s_ in two.shards], axis=2))
    for s_ in two.shards:
        _check(s_, "a shard")
        _check_guards(s_, "a shard")
    one.free(act); one.close(); two.close()
