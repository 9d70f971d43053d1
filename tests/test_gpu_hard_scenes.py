"""The frame kernels' culling at the constructed states of tests/hard_scenes.py: cubes cut by the frame borders, outside the frame, on tile seams, of a few pixels and of less
than one, centimetres in front of a camera (the full-frame record of build_prim), around and behind it, hidden behind one another and behind the base, in and under the floor; the
marker over, behind and in front of everything; the arm at its joint limits, along the image axes and end-on; the wrist camera's own hard poses.  tests/test_hard_scenes.py
shows on the CPU that every scene reaches its regime.

One sim per (task, build) holds the whole catalogue of the task as its envs (70 stack, 77 pick_place, 76 push, not padded: the several-envs-per-workgroup mappings
end on a ragged workgroup in stack and pick_place), driven as the other image tests are: set_state, then reset(mask = zeros).  Builds: colours at the default 240 x 320 (the
fixed-size kernel), at 36 x 52 and at 256 x 512 (32 tile columns: a full-frame primitive sets tb = 31); both planes at 240 x 320 and 36 x 52; the look with both planes at
120 x 160 (look_ref.GPU_VARIANTS: they move the cameras by centimetres, so the scenes are no longer where their claims say, (c) is not asked there, and no primitive
is within 0.02 m of a moved camera: the look build's full-frame record is NOT reached by this test); the wrist camera with both planes at
84 x 84.  The frames of a (task, build) are drawn once and the cases of the 240 x 320 builds, one per scene family, share them: the fp64 models cost 0.07 s a frame there.

Per env and camera:
  (a) batched against the one-ray-per-pixel path of the same library (render, render_planes; the wrist's singles): pixels beyond +-2 levels <= _raycast_pixels(H, W), pixels
      failing planes_ref.agree(..., 1e-5) <= _raycast_pixels(H, W) -- and every such pixel has more than one segmentation byte in the 3 x 3 neighbourhood of the per-pixel
      segmentation (the whole byte, marker bit included: the marker's outline is a box edge like any other): the two paths share box_hit and the background kernels, so they can differ only where a box meets the floor, the sky or another box.  A culled tile shows
      as differences inside a face, however few.
  (b) batched against the fp64 model (render_oracle / planes_ref, look_ref, wrist_ref): <= _oracle_pixels(H, W) pixels beyond +-2 levels, <= _ref_pixels(H, W) pixels failing
      planes_ref.agree(..., 1e-4), at every build but 256 x 512.  Where the per-pixel path itself -- not the code under test -- exceeds that against the fp64 model, the scene's
      bound is that count plus one pixel (_PARENT_PATH_SCENES, the precedent of tests/test_gpu_image_size._PARENT_PATH_PIXELS).
  (c) the scene's claims on the GPU's own segmentation planes, or, in a colour-only build, the claims about the cubes' pixels on its colour frames.

Measured on an MI355X, worst count per frame over all scenes, the same in all three tasks -- what differs from the models is background, not a constructed primitive:
  build             (a) colour / planes   allowed      (b) colour / planes   allowed      per-pixel path vs fp64 model
  colours 240x320        0 / -             15.4             2 / -              76.8             2
  colours 36x52          0 / -              2.3             0 / -              11.5             0
  colours 256x512        0 / -             26.2             (not compared)
  planes 240x320         0 / 0             15.4             2 / 0              76.8             2 / 0
  planes 36x52           0 / 0              2.3             0 / 0              11.5             0 / 0
  look 120x160           7 / 0              7.7             5 / 0              38.4             6 / 0
  wrist 84x84            0 / 0              5.4             1 / 0              26.9             1 / 0
No scene needs a bound of its own: _PARENT_PATH_SCENES is empty.  The seven pixels of the look build are those tests/test_gpu_look.py reports for its random states; here
they pass the neighbourhood rule, so they lie where two segmentation ids meet (the horizon of the rolled camera_front or a silhouette), not inside a surface.
pytest --durations of the 55 cases (107 s together): the slowest is 4.4 s (stack-colours-240x320-border: it draws the sim, 154 frames twice, and compares 40 of them with
the fp64 model); the border and arm cases of the 240 x 320 builds take 3.7 - 4.0 s, the look cases 3.5 - 3.8 s, every other case less than 3.5 s.
"""
import functools

import numpy as np
import pytest

from tests import hard_scenes as hs
from tests import look_ref, planes_ref, wrist_ref
from tests.test_gpu_image_planes import _ref_pixels
from tests.test_gpu_image_size import _oracle_pixels, _raycast_pixels
from tests.test_look_abi import gpu_test_colours

pytestmark = pytest.mark.gpu

BOTH = ("depth", "segmentation")
FAMILIES = ("border", "seam", "near", "occl", "marker", "arm", "wrist")
# build -> (H, W), VecSim keywords, compared with the fp64 model
BUILDS = {
    "colours-240x320": ((240, 320), {}, True),
    "colours-36x52": ((36, 52), {"image_size": (36, 52)}, True),
    "colours-256x512": ((256, 512), {"image_size": (256, 512)}, False),
    "planes-240x320": ((240, 320), {"image_size": (240, 320), "image_planes": BOTH}, True),
    "planes-36x52": ((36, 52), {"image_size": (36, 52), "image_planes": BOTH}, True),
    "look-120x160": ((120, 160), {"image_size": (120, 160), "image_planes": BOTH, "look_variants": look_ref.GPU_VARIANTS}, True),
    "wrist-84x84": ((84, 84), {"image_size": (84, 84), "wrist_camera": True, "image_planes": BOTH}, True),
}
CASES = [(t, b, f) for b, (size, _, _) in BUILDS.items() for t in hs.TASKS for f in (FAMILIES if size[0] * size[1] >= 240 * 320 and BUILDS[b][2] else ("all",))
         if not (f == "marker" and t == "stack")]

# (build, task, scene, camera, "colour" | "planes") -> pixels by which the per-pixel path of the parent commit differs from the fp64 model, where that exceeds the allowance; the
# bound of that frame is the count plus one pixel
_PARENT_PATH_SCENES = {}


@functools.lru_cache(maxsize=2)
def _drawn(task, build):
    """the frames of one sim that holds the catalogue: batched and per-pixel, read back; the sim is closed again"""
    from gym_lowcostrobot_amd import VecSim

    (H, W), kw, _ = BUILDS[build]
    cat = hs.catalogue(task, H, W)
    n = len(cat)
    sim = VecSim(task, n, observation_mode="both", auto_reset=False, **kw)      # (depth_far = 10, the default)
    assert sim.image_size == (H, W) and sim.n == n
    qpos = np.stack([s[1] for s in cat], 1)
    target = np.stack([s[2] for s in cat], 1).astype(np.float32)
    sim.set_state(qpos=qpos, target=target)
    look = None
    if "look_variants" in kw:
        look = ((np.arange(n) % 4).astype(np.int32), gpu_test_colours(n))
        sim.set_look(variant=look[0], rgb=look[1])      # redraws the frames from the new state
    else:
        sim.reset(mask=np.zeros(n, np.uint8))            # no env reset, but re-renders frames and planes from the new state
    obs = sim.observations()
    cams = [(hs.FRONT, "front"), (hs.TOP, "top")] + ([(hs.WRIST, "wrist")] if "wrist_camera" in kw else [])
    out = {"cat": cat, "cams": cams, "look": look, "size": (H, W), "planes": "image_planes" in kw}
    for cam, c in cams:
        out[cam] = {"rgb": obs[f"image_{c}"].copy(), "px_rgb": np.stack([sim.render(e, cam, W, H) for e in range(n)])}
        px = [sim.render_planes(e, cam, W, H) for e in range(n)]
        out[cam]["px_depth"], out[cam]["px_seg"] = np.stack([p[0] for p in px]), np.stack([p[1] for p in px])
        if out["planes"]:
            out[cam]["depth"], out[cam]["seg"] = obs[f"depth_{c}"].copy(), obs[f"segmentation_{c}"].copy()
    sim.close()
    return out


def _several_ids_nearby(seg):
    """pixels whose 3 x 3 neighbourhood holds more than one segmentation byte -- id or marker bit: the translucent marker is a box, and the two paths may fall on different
    sides of its outline as of any other"""
    p = np.pad(seg, 1, mode="edge")
    H, W = seg.shape
    nb = np.stack([p[i:i + H, j:j + W] for i in range(3) for j in range(3)])
    return nb.min(0) != nb.max(0)


def _model(task, build, cam, q, t, H, W, look, e):
    """(colour frame, depth, segmentation) of the fp64 model of this build's camera"""
    if cam == hs.WRIST:
        return wrist_ref.render(task, q, t, None, W, H), wrist_ref.planes(task, q, t, None, W, H, depth_far=10.0)
    if look is not None:
        v, rgb = look_ref.GPU_VARIANTS[look[0][e]], look[1][:, e]
        return look_ref.render(task, q, t, cam, W, H, v=v, rgb=rgb), look_ref.planes(task, q, t, cam, W, H, v=v, depth_far=10.0)
    from oracle import render_oracle
    return render_oracle.render(task, q, t, cam, W, H), planes_ref.planes(task, q, t, cam, W, H, depth_far=10.0)


@pytest.mark.parametrize("task,build,family", CASES, ids=[f"{t}-{b}-{f}" for t, b, f in CASES])
def test_hard_scenes(hip_lib, task, build, family):
    (H, W), kw, with_model = BUILDS[build]
    D = _drawn(task, build)
    cat, look, has_planes = D["cat"], D["look"], D["planes"]
    fails, worst = [], {"a colour": 0, "a planes": 0, "b colour": 0, "b planes": 0, "path colour": 0, "path planes": 0}
    for e, sc in enumerate(cat):
        name, q, t, claims = sc
        if family != "all" and not name.startswith(family):
            continue
        for cam, _c in D["cams"]:
            F = D[cam]
            # (a) against the per-pixel path of the same library
            several = _several_ids_nearby(F["px_seg"][e])
            diff = np.abs(F["rgb"][e].astype(int) - F["px_rgb"][e].astype(int)).max(-1) > 2
            checks = [("a colour", diff)]
            if has_planes:
                checks.append(("a planes", ~planes_ref.agree(F["depth"][e], F["seg"][e], F["px_depth"][e], F["px_seg"][e], 1e-5)))
            for what, bad in checks:
                cnt = int(bad.sum())
                worst[what] = max(worst[what], cnt)
                if cnt > _raycast_pixels(H, W):
                    fails.append((name, cam, what, cnt, np.argwhere(bad)[:5].tolist()))
                inside = bad & ~several
                if inside.any():
                    fails.append((name, cam, what + ": differences away from every silhouette", int(inside.sum()), np.argwhere(inside)[:5].tolist()))
            # (b) against the fp64 model
            if with_model:
                ref, (dref, sref) = _model(task, build, cam, q, t, H, W, look, e)
                mdiff = lambda a: np.abs(a.astype(int) - ref.astype(int)).max(-1) > 2   # noqa: E731
                res = [("colour", mdiff(F["rgb"][e]), mdiff(F["px_rgb"][e]), _oracle_pixels(H, W))]
                if has_planes:
                    res.append(("planes", ~planes_ref.agree(F["depth"][e], F["seg"][e], dref, sref, 1e-4), ~planes_ref.agree(F["px_depth"][e], F["px_seg"][e], dref, sref, 1e-4),
                                _ref_pixels(H, W)))
                for what, bad, path_bad, allowed in res:
                    cnt, path = int(bad.sum()), int(path_bad.sum())
                    worst["b " + what] = max(worst["b " + what], cnt); worst["path " + what] = max(worst["path " + what], path)
                    if path > allowed:
                        print(f"[hard scenes] per-pixel path vs fp64 model beyond the allowance: {(build, task, name, cam, what)}: {path} (allowed {allowed:.1f}; batched {cnt})")
                    allowed = max(allowed, _PARENT_PATH_SCENES.get((build, task, name, cam, what), 0))
                    if cnt > allowed:
                        fails.append((name, cam, "b " + what, cnt, allowed, np.argwhere(bad)[:5].tolist()))
        # (c) the scene's claims on the GPU's own planes / frames
        if look is None:
            if has_planes:
                broken = hs.check_claims(task, sc, lambda cam: D[cam]["seg"][e] if cam in D else None, H, W, geometric=False)
            else:
                broken = hs.check_claims(task, hs.colour_claims(sc), lambda cam: hs.seg_from_rgb(D[cam]["rgb"][e]) if cam in D else None, H, W, geometric=False)
            fails += [("claim",) + b for b in broken]
    print(f"[hard scenes] {task} {build} {family}: worst per frame -- (a) batched vs per-pixel path {worst['a colour']} colour / {worst['a planes']} plane pixels (allowed "
          f"{_raycast_pixels(H, W):.1f}); (b) batched vs fp64 model {worst['b colour']} / {worst['b planes']} (allowed {_oracle_pixels(H, W):.1f}), per-pixel path vs fp64 model "
          f"{worst['path colour']} / {worst['path planes']}")
    assert not fails, fails
