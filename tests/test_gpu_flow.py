"""The motion vectors on the GPU (VecSim(..., motion_vectors=True | dict(cameras=)); lcr_enable_motion_vectors): the library's device planes against the numpy model of
tests/flow_ref.py, which is fed the library's own depth and segmentation planes, `flow_valid`, `flow_boxes` and `flow_pose` read back.

What is exact: every byte of every plane and `flow_valid`.  The rule is pinned to the bit (include/lcr.h: "Motion vectors"), so each plane is compared as uint16 words,
after enabling and after every step of seeded random actions, and the guard regions around every plane are read back at the end of each rollout.  After every restart
(enabling, reset, set_look, set_state) the planes are zero, valid is 0 and "before" is bit-equal to "now".

Each rollout ASSERTS the regime it is there for, so a case that never reaches it fails:
  stack   n = 70 (a ragged second wave of envs), 36 x 52 (W no multiple of 16), front + top + wrist, 55 steps: every env auto-resets, in that step its planes are zero and
          valid is 0, in the next step it is valid again; nonzero words are seen on every arm id 3 .. 8; on the fixed cameras every floor and base pixel (ids 1, 2) of a
          valid env is the +0.0 pair; the wrist floor is nonzero while the arm moves; the box of the link the wrist camera is mounted on stays below 1e-2 px in the wrist
          plane (it is rigid with the camera: an answer known without the model).
  push    n = 5 at 16 x 20 and at 20 x 16 (a frame smaller than a workgroup), 6 steps.
  reach   n = 3 at the default 240 x 320, 1 step; n = 64 at 84 x 84, 3 steps.
  look    reach, n = 5 at 32 x 32, two look variants that turn the cameras, a sampler and episodes of 3 steps: a reset that changes an env's variant gives valid 0, and
          every valid env measures with its own variant's camera, now and before.
  falling cube  push, n = 5: set_state puts the cube in the air in view of the front camera; planes zero and valid 0; then two zero-action steps: fy > 0 on the cube's
          pixels of the front plane, larger in the second step.

On an MI355X the rollouts gave (every word equal to the model's in all of them): stack 3 920 env-checks, all 70 envs auto-reset and 72 env-steps valid again right behind
a reset, 5 865 650 pixels ran the chain, nonzero words on ids 1 .. 10, 2 424 143 nonzero wrist-floor pixels, 960 622 pixels of the link the wrist camera rides on with at
most 9.3e-5 px, 13 223 145 floor and base pixels of valid envs on the fixed cameras all the +0.0 pair, the largest finite flow 63 712 px (a wrist pixel whose point passed
close by the previous camera); push 16 x 20 1 345 and 20 x 16 2 002 chain pixels, nonzero ids 3 .. 9, at most 6.1 and 7.8 px; default 28 006 chain pixels, at most
36.1 px; many 222 489, at most 30.4 px.
"""
import functools

import numpy as np
import pytest

from tests import flow_ref

pytestmark = pytest.mark.gpu

ALL = ("front", "top", "wrist")
# name, task, n, size (H, W), cameras, steps
ROLLOUTS = [
    ("stack", "stack", 70, (36, 52), ALL, 55),
    ("push", "push", 5, (16, 20), ("front", "top"), 6),
    ("push", "push", 5, (20, 16), ("front", "top"), 6),
    ("default", "reach", 3, None, ("front", "top"), 1),
    ("many", "reach", 64, (84, 84), ("front", "top"), 3),
]
ROLLOUT_IDS = [f"{r[0]}-{r[1]}-n{r[2]}-" + ("default" if r[3] is None else f"{r[3][0]}x{r[3][1]}") for r in ROLLOUTS]
ATTRS = ("flow_front", "flow_top", "flow_wrist", "flow_valid", "flow_boxes", "flow_pose", "flow_spec")
LOOK_VARIANTS = [{}, {"cam_dpos": [[0.03, 0.0, 0.02], [0.0, 0.04, 0.05]], "cam_drot": [[0.2, 0.0, 0.0], [0.0, 0.25, 0.0]], "fovy_deg": [50.0, 40.0]}]


def _kw(size, wrist, **more):
    kw = dict(observation_mode="both", image_planes=("depth", "segmentation"), wrist_camera=True if wrist else None, **more)
    if size is not None:
        kw["image_size"] = size
    return kw


def _words(a):
    """a float16 plane as its uint16 words"""
    return np.ascontiguousarray(a).view(np.uint16)


def _check(sim, when, restarted=False):
    """the invariant: every plane is the header's function of the env's current planes, the history and valid, to the word -> {camera: (plane, seg, chain mask)}, valid"""
    cams = sim.flow_spec["cameras"]
    boxes, poses, valid = sim.flow_boxes.numpy(), sim.flow_pose.numpy(), sim.flow_valid.numpy()
    assert boxes.shape == (2, 9, 15, sim.n) and poses.shape == (2, len(cams), 13, sim.n) and np.isfinite(boxes).all() and np.isfinite(poses).all()
    assert valid.shape == (sim.n,) and valid.dtype == np.uint8 and (valid <= 1).all()
    if restarted:
        assert not valid.any(), when
        assert boxes[0].tobytes() == boxes[1].tobytes() and poses[0].tobytes() == poses[1].tobytes(), when
    out = {}
    for slot, cam in enumerate(cams):
        depth, seg = getattr(sim, "depth_" + cam).numpy(), getattr(sim, "seg_" + cam).numpy()
        want, ran = flow_ref.planes(depth, seg, boxes, poses[:, slot], valid, detail=True)
        got = getattr(sim, "flow_" + cam).numpy()
        assert got.shape == want.shape == seg.shape + (2,) and got.dtype == np.float16
        bad = np.argwhere((_words(got) != _words(want)).any(axis=-1))
        assert bad.size == 0, (when, cam, len(bad), bad[:6].tolist(), [(got[tuple(b)].tolist(), want[tuple(b)].tolist(), int(seg[tuple(b)])) for b in bad[:6]])
        if restarted:
            assert not _words(got).any(), (when, cam)
        out[cam] = (got, seg, ran)
    return out, valid.astype(bool)


def _check_guards(sim, when):
    from gym_lowcostrobot_amd import _capi
    from tests.test_gpu_wrist import _guards

    for cam in sim.flow_spec["cameras"]:
        for side, g in zip(("before", "behind"), _guards(sim, getattr(sim, "flow_" + cam))):
            assert g.size >= _capi.WRIST_GUARD and (g == _capi.WRIST_GUARD_BYTE).all(), (when, cam, side, np.nonzero(g != _capi.WRIST_GUARD_BYTE)[0][:8].tolist())


@functools.lru_cache(maxsize=None)
def _rollout(case):
    """runs one rollout, checking the invariant after enabling and after every step -> the regime counters"""
    from gym_lowcostrobot_amd import VecSim

    name, task, n, size, cams, steps = case
    sim = VecSim(task, n, base_seed=17, motion_vectors=dict(cameras=cams), **_kw(size, "wrist" in cams))
    assert sim.flow_spec == {"cameras": cams}
    mount = None if "wrist" not in cams else int(sim.wrist_camera["link"])   # link_i is box i, surface id i + 2
    act = sim.alloc_actions()
    was_reset = np.zeros(n, bool)
    last_reset = np.zeros(n, bool)
    st = {"checks": 0, "chain_pixels": 0, "nonzero_ids": set(), "valid_after_reset": 0, "wrist_floor_nonzero": 0, "mount_pixels": 0, "mount_worst": 0.0, "static_pixels": 0,
          "worst_flow": 0.0}
    for t in range(-1, steps):
        if t >= 0:
            sim.fill_random_actions(act, 23, t); sim.step_device(act.ptr)
        planes, valid = _check(sim, f"step {t}", restarted=t < 0)
        st["checks"] += n
        if t >= 0:
            did = sim.outputs()["did_reset"].astype(bool)
            np.testing.assert_array_equal(valid, ~did)                    # an env the step auto-reset is not valid in that step ...
            st["valid_after_reset"] += int((last_reset & valid).sum())    # ... and valid again in the next
            was_reset |= did; last_reset = did
        for cam, (got, seg, ran) in planes.items():
            ids = seg & 0x7F
            zero = ~_words(got).any(axis=-1)
            assert zero[~valid].all() and zero[(ids == 0) | (ids > 10)].all()
            st["chain_pixels"] += int(ran.sum())
            st["nonzero_ids"] |= set(np.unique(ids[~zero]).tolist())
            finite = np.abs(got[np.isfinite(got)].astype(np.float32))
            st["worst_flow"] = max(st["worst_flow"], float(finite.max()) if finite.size else 0.0)
            if cam != "wrist":   # a fixed camera: the floor and the base never move, and carry the +0.0 pair exactly
                still = valid[:, None, None] & (ids <= 2)
                assert zero[still].all() and not ran[still].any(), (t, cam)
                st["static_pixels"] += int(still.sum())
            elif t >= 0:
                floor = valid[:, None, None] & (ids == 1)
                st["wrist_floor_nonzero"] += int((floor & ~zero).sum())
                if mount:   # the link the camera rides on: rigid with the camera, so its flow is rounding alone
                    m = valid[:, None, None] & (ids == mount + 2)
                    st["mount_pixels"] += int(m.sum())
                    if m.any():
                        st["mount_worst"] = max(st["mount_worst"], float(np.abs(got[m].astype(np.float32)).max()))
    _check_guards(sim, "after the rollout")
    obs = sim.observations()
    for cam in cams:
        assert obs["flow_" + cam].tobytes() == getattr(sim, "flow_" + cam).numpy().tobytes()
    st["all_reset"] = bool(was_reset.all()); st["resets"] = int(was_reset.sum())
    sim.free(act); sim.close()
    print(f"flow rollout {ROLLOUT_IDS[ROLLOUTS.index(case)]}: " + str({k: (sorted(v) if isinstance(v, set) else v) for k, v in st.items()}))
    return st


@pytest.mark.parametrize("case", ROLLOUTS, ids=ROLLOUT_IDS)
def test_every_plane_equals_the_model_after_every_step(hip_lib, case):
    st = _rollout(case)
    name = case[0]
    assert st["checks"] == case[2] * (case[5] + 1) and st["chain_pixels"] > 0 and st["static_pixels"] > 0
    assert st["nonzero_ids"] - {0}, st                                      # something moved and was measured
    if name == "stack":
        assert st["all_reset"], st                                         # every env auto-resets within the rollout
        assert st["valid_after_reset"] > 0, st                             # and is valid again in the step behind its reset
        assert {3, 4, 5, 6, 7, 8} <= st["nonzero_ids"], st                 # the links move
        assert st["wrist_floor_nonzero"] > 0, st                           # the floor moves under the wrist camera
        assert st["mount_pixels"] > 0 and st["mount_worst"] < 1e-2, st     # the link the camera rides on does not move in its plane


def test_a_falling_cube_moves_down_the_front_plane(hip_lib):
    """set_state puts the cube in the air in view of the front camera and restarts the flow; two zero-action steps later the cube's pixels carry fy > 0, larger in the
    second step (it accelerates), and every word equals the model's"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 5, (36, 52)
    sim = VecSim("push", n, base_seed=2, motion_vectors=dict(cameras=("front", "top")), **_kw(size, False))
    act = sim.alloc_actions()
    sim.fill_random_actions(act, 5, 0); sim.step_device(act.ptr)
    _, valid = _check(sim, "a first step")
    assert valid.any()
    state = sim.get_state()
    qpos, qvel = np.array(state["qpos"], np.float64), np.zeros_like(np.array(state["qvel"], np.float64))
    # 0.35 m down the front camera's axis, between the camera and the arm: the CPU ray caster shows 16 to 20 cube pixels there at this size for every arm pose tried,
    # the arm's zero pose among them, and down to 6 cm lower
    qpos[6], qpos[7], qpos[8] = 0.0305, 0.1708, 0.1076 + 0.003 * np.arange(n)
    qpos[9:13] = np.array([1.0, 0.0, 0.0, 0.0])[:, None]
    sim.set_state(qpos=qpos, qvel=qvel)
    _check(sim, "after set_state", restarted=True)
    fy = []
    for t in range(2):
        sim.step(np.zeros((n, sim.action_dim), np.float32))
        planes, valid = _check(sim, f"falling step {t}")
        assert valid.all()
        got, seg, ran = planes["front"]
        cube = (seg & 0x7F) == 9
        assert cube.reshape(n, -1).any(axis=1).all() and ran[cube].all()     # every env shows its cube, and its pixels run the chain
        assert (got[cube][:, 1] > 0).all(), got[cube][:, 1].min()
        fy.append(np.array([got[e][cube[e]][:, 1].astype(np.float32).mean() for e in range(n)]))
    print(f"falling cube: mean fy per env, step 0 {fy[0].round(4).tolist()}, step 1 {fy[1].round(4).tolist()}")
    assert (fy[1] > fy[0]).all(), fy
    _check_guards(sim, "after the fall")
    sim.free(act); sim.close()


def test_a_reset_that_changes_the_camera_is_not_valid_and_valid_steps_use_the_variants_camera(hip_lib):
    from gym_lowcostrobot_amd import VecSim

    n, size = 5, (32, 32)
    sim = VecSim("reach", n, base_seed=5, max_episode_steps=3, look_variants=LOOK_VARIANTS, look_sampler={"seed": 9}, motion_vectors=True, **_kw(size, False))
    act = sim.alloc_actions()
    seen = {}          # variant -> its two camera poses as bytes
    changed = valid_steps = 0
    variant = sim.look()["variant"].copy()
    _check(sim, "enabled", restarted=True)
    pose = sim.flow_pose.numpy()
    for e in range(n):
        assert seen.setdefault(int(variant[e]), pose[0, :, :, e].tobytes()) == pose[0, :, :, e].tobytes()
    for t in range(14):
        sim.fill_random_actions(act, 3, t); sim.step_device(act.ptr)
        planes, valid = _check(sim, f"step {t}")
        now = sim.look()["variant"]
        did = sim.outputs()["did_reset"].astype(bool)
        np.testing.assert_array_equal(valid, ~did)
        assert did[now != variant].all()                                   # only a reset changes the variant
        changed += int((now != variant).sum())
        pose = sim.flow_pose.numpy()
        for e in range(n):
            assert seen.setdefault(int(now[e]), pose[0, :, :, e].tobytes()) == pose[0, :, :, e].tobytes()   # "now" is the env's variant's camera
            if valid[e]:
                assert pose[1, :, :, e].tobytes() == pose[0, :, :, e].tobytes()   # and so is "before": the fixed cameras of a valid env are static
                valid_steps += 1
            elif now[e] != variant[e]:
                assert pose[1, :, :, e].tobytes() == seen[int(variant[e])]       # before the reset it was the other variant's
                for cam, (got, _, _) in planes.items():
                    assert not _words(got[e]).any()
        variant = now.copy()
    print(f"flow look: {changed} resets changed the variant, {valid_steps} valid env-steps, variants seen {sorted(seen)}")
    assert changed > 0 and valid_steps > 0 and len(seen) == 2 and seen[0] != seen[1]
    _check_guards(sim, "after the steps")
    sim.free(act); sim.close()


def test_every_other_entry_point_restarts(hip_lib):
    """reset(), a masked reset, the no-op reset, set_look and set_state each zero every plane and give valid 0 with "before" a copy of "now"; the step behind each is valid"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 6, (20, 28)
    sim = VecSim("push", n, base_seed=8, look_variants=LOOK_VARIANTS, motion_vectors=True, **_kw(size, True))
    assert sim.flow_spec == {"cameras": ALL}
    act = sim.alloc_actions()
    t = 0

    def step():
        nonlocal t
        sim.fill_random_actions(act, 31, t); sim.step_device(act.ptr); t += 1
        planes, valid = _check(sim, f"step {t}")
        np.testing.assert_array_equal(valid, ~sim.outputs()["did_reset"].astype(bool))   # measured, but for an env this very step auto-reset
        assert valid.any() and any(_words(got).any() for got, _, _ in planes.values())   # and something moved
    _check(sim, "enabled", restarted=True)
    step()
    restarts = {
        "reset": lambda: sim.reset(),
        "masked reset": lambda: sim.reset(mask=(np.arange(n) % 2).astype(np.uint8)),
        "no-op reset": lambda: sim.reset(mask=np.zeros(n, np.uint8)),
        "set_look": lambda: sim.set_look(variant=(np.arange(n) % 2).astype(np.int32)),
        "set_state": lambda: sim.set_state(qpos=np.array(sim.get_state()["qpos"], np.float64)),
    }
    for name, call in restarts.items():
        call()
        _check(sim, f"after {name}", restarted=True)
        step(); step()
    _check_guards(sim, "after the restarts")
    sim.free(act); sim.close()


def test_off_means_off(hip_lib):
    """a handle without motion_vectors has none of the attributes, and its colour frames, planes and normals are byte-equal to those of a handle with them after the same
    seeded steps"""
    from gym_lowcostrobot_amd import VecSim

    n, size = 6, (36, 52)
    kw = _kw(size, True, base_seed=11, surface_normals=True)
    off, on = VecSim("push", n, **kw), VecSim("push", n, motion_vectors=True, **kw)
    for a in ATTRS:
        assert not hasattr(off, a), a
        assert hasattr(on, a), a
    assert not any(k.startswith("flow") for k in off.observations())
    assert {"flow_front", "flow_top", "flow_wrist"} <= set(on.observations())
    acts = [a.alloc_actions() for a in (off, on)]
    for t in range(4):
        for s_, act in zip((off, on), acts):
            s_.fill_random_actions(act, 9, t); s_.step_device(act.ptr)
        for key in ("image_front", "image_top", "image_wrist", "depth_front", "depth_top", "depth_wrist", "seg_front", "seg_top", "seg_wrist",
                    "normals_front", "normals_top", "normals_wrist"):
            a, b = getattr(off, key).numpy(), getattr(on, key).numpy()
            assert a.tobytes() == b.tobytes(), (t, key)
        _check(on, f"step {t}")
    _check_guards(on, "after the steps")
    for s_, act in zip((off, on), acts):
        s_.free(act); s_.close()


def test_the_same_spec_again_is_a_no_op_and_another_is_refused(hip_lib):
    import ctypes

    from gym_lowcostrobot_amd import VecSim, _capi

    sim = VecSim("reach", 4, motion_vectors=dict(cameras=("front",)), **_kw((16, 16), False))
    ptr = sim.flow_front.ptr
    same, other = _capi.MotionSpec.from_any(dict(cameras=("front",))), _capi.MotionSpec.from_any(dict(cameras=("front", "top")))
    assert sim.L.lcr_enable_motion_vectors(sim.handle, ctypes.byref(same)) == 0
    view = _capi.LcrMotionView()
    assert sim.L.lcr_get_motion_vectors(sim.handle, ctypes.byref(view)) == 0 and view.flow_front == ptr and not view.flow_top and view.slots == 1
    assert sim.L.lcr_enable_motion_vectors(sim.handle, ctypes.byref(other)) == _capi.LCR_ERR_INVALID
    msg = sim.L.lcr_last_error()
    assert b"cameras 1" in msg and b"cameras 3" in msg, msg
    wrist = _capi.MotionSpec.from_any(dict(cameras=("wrist",)))
    assert sim.L.lcr_enable_motion_vectors(sim.handle, ctypes.byref(wrist)) == _capi.LCR_ERR_INVALID and b"wrist" in sim.L.lcr_last_error()
    sim.close()
    plain = VecSim("reach", 4, observation_mode="both", image_size=(16, 16), image_planes=("depth",))
    assert plain.L.lcr_enable_motion_vectors(plain.handle, ctypes.byref(same)) == _capi.LCR_ERR_INVALID and b"the segmentation plane is missing" in plain.L.lcr_last_error()
    plain.close()
