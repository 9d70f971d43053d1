"""The catalogue of tests/hard_scenes.py reaches its regimes: every claim of every scene holds in the fp64 models -- tests/planes_ref.planes and tests/wrist_ref.planes at
240 x 320 and 36 x 52, and, for the claims a colour frame can decide (the cubes' pixel counts and places), oracle.render_oracle.render and tests/wrist_ref.render at 36 x 52.  A
scene that misses its regime fails here, on the CPU, before tests/test_gpu_hard_scenes.py draws it.  No GPU.
"""
import numpy as np
import pytest

from oracle import render_oracle
from tests import hard_scenes as hs
from tests import planes_ref, wrist_ref

SIZES = [(240, 320), (36, 52)]


def test_the_catalogue_has_every_family_and_float32_states():
    for task in hs.TASKS:
        cat = hs.catalogue(task)
        names = [s[0] for s in cat]
        families = {n.split("_")[0] for n in names}
        assert families == {"border", "seam", "near", "occl", "arm", "wrist"} | ({"marker"} if task != "stack" else set()), (task, families)
        for fam, least in (("border", 20), ("seam", 4), ("near", 10), ("occl", 7), ("arm", 20), ("wrist", 5)):
            assert sum(n.startswith(fam) for n in names) >= least, (task, fam)
        for name, q, t, claims in cat:
            assert q.shape == (20 if task == "stack" else 13,) and t.shape == (3,) and claims, name
            np.testing.assert_array_equal(q, q.astype(np.float32).astype(np.float64), err_msg=name)
            np.testing.assert_array_equal(t, t.astype(np.float32).astype(np.float64), err_msg=name)
            for c in range(2 if task == "stack" else 1):
                assert abs(np.linalg.norm(q[9 + 7 * c:13 + 7 * c]) - 1.0) < 1e-6, name
        # the same names at every frame size, so that one docstring can speak of a scene
        assert names == [s[0] for s in hs.catalogue(task, 36, 52)] == [s[0] for s in hs.catalogue(task, 256, 512)]
    # joint 6 ends at [-2.45, 0.032]
    q = {s[0]: s[1] for s in hs.catalogue("push")}
    assert q["arm_joint6_lo"][5] == np.float32(-2.45) and q["arm_joint6_hi"][5] == np.float32(0.032) and q["arm_joint1_hi"][0] == np.float32(3.14)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", hs.TASKS)
def test_every_claim_holds_in_the_fp64_models(task, size):
    H, W = size
    bad = []
    for sc in hs.catalogue(task, H, W):
        name, q, t, claims = sc
        cache = {}

        def planes_of(cam):
            if cam not in cache:
                cache[cam] = wrist_ref.planes(task, q, t, None, W, H)[1] if cam == hs.WRIST else planes_ref.planes(task, q, t, cam, W, H)[1]
            return cache[cam]

        bad += hs.check_claims(task, sc, planes_of, H, W)
        if size == (36, 52):   # the claims a colour-only build is checked with, on the models' colour frames
            cc = hs.colour_claims(sc)

            def colours_of(cam):
                rgb = wrist_ref.render(task, q, t, None, W, H) if cam == hs.WRIST else render_oracle.render(task, q, t, cam, W, H)
                return hs.seg_from_rgb(rgb)

            bad += [("colours",) + b for b in hs.check_claims(task, cc, colours_of, H, W, geometric=False)]
    assert not bad, bad


def test_the_near_plane_cases_the_models_define():
    """axis-aligned cubes on the axis of camera_top at 36 x 52: centre depths 0.036 and 0.03 fill all 1 872 pixels, 0.05 fills 1 368, 0.01 (the camera inside the cube) and
    -0.05 (behind it) give none"""
    C = hs.camera_of("stack", hs.TOP)
    for depth, want in ((0.036, 1872), (0.03, 1872), (0.05, 1368), (0.01, 0), (-0.05, 0)):
        q, t = hs._state("stack", cube=hs.unproject(C, 0.5, 0.5, depth, 52 / 36), cube_R=hs._axes(C))
        seg = planes_ref.planes("stack", q, t, hs.TOP, 52, 36)[1]
        assert int(((seg & 0x7F) == hs.ID_CUBE).sum()) == want, (depth, want)
        rgb = render_oracle.render("stack", q, t, hs.TOP, 52, 36)
        assert int((hs.seg_from_rgb(rgb) == hs.ID_CUBE).sum()) == want, (depth, want)


@pytest.mark.parametrize("size", [(240, 320), (256, 512), (120, 160), (84, 84), (36, 52)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_end_on_states_reach_the_fallback_at_every_build_size(size):
    """build_prim's `len` (hard_scenes.kernel_axis_len: the distance of the means of the projected corners of the two end faces, not of the projected face centres) of the
    four end-on states is below 1e-4 pixels -- a tenth of the kernel's 1e-3 -- in fp64 and in float32 at every frame size of tests/test_gpu_hard_scenes.py; the home pose,
    for contrast, has tens of pixels"""
    H, W = size
    cat = {s[0]: s for s in hs.catalogue("push", H, W)}
    for (box, cam), _q in hs.END_ON.items():
        name, q, t, claims = cat[f"arm_end_on_link{box}_{cam.split('_')[1]}"]
        assert ("axis_px", cam, box, 1e-4) in claims
        for dtype in (np.float64, np.float32):
            assert hs.kernel_axis_len("push", cam, q, t, box, H, dtype) < 1e-4, (name, dtype)
        home = cat["arm_joint6_hi"]
        assert hs.kernel_axis_len("push", cam, home[1], home[2], box, H) > 0.02 * H, (name, "home")
