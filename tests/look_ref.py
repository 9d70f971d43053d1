"""Reference of the frames and planes drawn with a look (a plain helper of tests/test_look_abi.py and tests/test_gpu_look.py): numpy, fp64, one ray per pixel, no tiles, no
culling, no cached background -- written from the definitions of include/lcr.h (lcr_look_variant, the sampler), not from the kernels.

A look = a variant (everything the background depends on: the two observation cameras moved and turned, their field of view, floor, sky, light, the arm's colours) + nine
per-env colour channels (cube, second cube, target marker).  The scene comes from the committed oracle (oracle.render_oracle.scene / camera) with the cameras moved and the
colours replaced; `render` follows oracle.render_oracle.render operation by operation, so that the default variant with the task's colours gives its very bytes.
  camera   position = scene position + cam_dpos; the axes X, Y, Z are rotated by |cam_drot| rad about cam_drot / |cam_drot| (Rodrigues; a zero vector leaves them);
           s = 2 tan(fovy / 2) / H
  colours  floor cells odd / even, sky = sky_rgb + a * sky_slope with a = clip(2 * normalised d.z, 0, 1), Lambert term ambient + diffuse * cos for floor, arm, cubes, marker
`dtype` = np.float32 runs the same ray arithmetic in fp32 on the fp64 scene (the "twin": it models neither fp32 forward kinematics nor a hardware reciprocal).
`planes` gives the depth / segmentation planes through the moved cameras (tests/planes_ref.py's definitions; colours and light do not show in them).
"""
import numpy as np

from oracle import render_oracle
from tests import planes_ref

CAM_INDEX = {"camera_front": 0, "camera_top": 1}
TASK_RGB = (0.5, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 1.0)   # cube, second cube, target marker (the geom rgba of the scene files)


def default_variant():
    """the values of lcr_look_variant_default, as Python doubles (what oracle.render_oracle.render draws with)"""
    return {"cam_dpos": np.zeros((2, 3)), "cam_drot": np.zeros((2, 3)), "fovy_deg": np.array([45.0, 45.0]),
            "floor_rgb": np.array([[0.2, 0.3, 0.4], [0.1, 0.2, 0.3]]), "sky_rgb": np.array([0.15, 0.25, 0.35]), "sky_slope": np.array([0.15, 0.25, 0.35]),
            "ambient": 0.3, "diffuse": 0.6, "arm_rgb": np.array([0.8, 0.8, 0.8]), "finger_rgb": np.array([0.75, 0.75, 0.75])}


def variant(**fields):
    """the default variant with some fields replaced; every number rounded to float32 as the library receives it"""
    v = default_variant()
    for k, val in fields.items():
        assert k in v, k
        v[k] = np.broadcast_to(np.asarray(val, float), np.shape(v[k])).copy() if np.ndim(v[k]) else float(val)
    return {k: (np.asarray(a, np.float32).astype(np.float64) if np.ndim(a) else float(np.float32(a))) for k, a in v.items()}


# The variants of the GPU tests: every field is used, offsets of both signs, a rotation about each world axis, fovy below and above 45.
GPU_VARIANTS = [
    variant(cam_dpos=[[0.02, 0.03, -0.03], [0.0, 0.05, 0.05]], cam_drot=[[0.07, 0.0, 0.02], [0.03, -0.02, 0.0]], fovy_deg=[45.0, 42.0]),   # (the scene's colours and light)
    variant(cam_dpos=[[0.05, -0.08, 0.04], [-0.06, 0.03, -0.1]], cam_drot=[[0.1, 0.0, 0.0], [0.0, 0.0, 0.3]], fovy_deg=[38.0, 55.0],
            floor_rgb=[[0.45, 0.35, 0.2], [0.3, 0.2, 0.1]], sky_rgb=[0.3, 0.2, 0.25], sky_slope=[0.4, 0.1, 0.3], ambient=0.45, diffuse=0.5,
            arm_rgb=[0.6, 0.7, 0.5], finger_rgb=[0.3, 0.3, 0.35]),
    variant(cam_dpos=[[-0.1, 0.06, -0.05], [0.08, -0.07, 0.1]], cam_drot=[[0.0, -0.12, 0.0], [-0.08, 0.0, 0.0]], fovy_deg=[60.0, 40.0],
            floor_rgb=[[0.1, 0.4, 0.3], [0.5, 0.5, 0.45]], sky_rgb=[0.05, 0.1, 0.3], sky_slope=[0.5, 0.45, 0.2], ambient=0.2, diffuse=0.9,
            arm_rgb=[0.9, 0.85, 0.3], finger_rgb=[0.2, 0.6, 0.8]),
    variant(cam_dpos=[[0.0, 0.1, 0.15], [0.12, 0.0, -0.2]], cam_drot=[[0.0, 0.0, 0.15], [0.0, 0.1, 0.0]], fovy_deg=[50.0, 30.0],
            floor_rgb=[[0.6, 0.6, 0.6], [0.25, 0.25, 0.3]], sky_rgb=[0.4, 0.4, 0.45], sky_slope=[0.2, 0.2, 0.2], ambient=0.35, diffuse=0.75,
            arm_rgb=[0.35, 0.35, 0.4], finger_rgb=[0.9, 0.5, 0.1]),
]


def camera(task, cam, v):
    """(position, X, Y, Z, fovy in degrees) of observation camera `cam` of variant `v`"""
    c = CAM_INDEX[cam]
    pos, X, Y, Z = render_oracle.camera(task, cam)
    pos = pos + np.asarray(v["cam_dpos"][c], float)
    r = np.asarray(v["cam_drot"][c], float)
    th = np.linalg.norm(r)
    if th > 0.0:
        k = r / th
        X, Y, Z = (a * np.cos(th) + np.cross(k, a) * np.sin(th) + k * (k @ a) * (1.0 - np.cos(th)) for a in (X, Y, Z))
    return pos, X, Y, Z, float(v["fovy_deg"][c])


def boxes_of(task, qpos, target, v, rgb):
    """the boxes of oracle.render_oracle.scene in the colours of the look: (centre, R, half, colour, alpha) -- seven arm boxes, the cube(s), the marker"""
    boxes = render_oracle.scene(task, qpos, target)[1]
    rgb = np.asarray(rgb, float)
    cols = [np.asarray(v["finger_rgb"] if i >= 5 else v["arm_rgb"], float) for i in range(7)] + [rgb[0:3]]
    if task == "stack":
        cols.append(rgb[3:6])
    if task in ("push", "pick_place"):
        cols.append(rgb[6:9])
    assert len(cols) == len(boxes)
    return [(bc, R, bh, col, alpha) for (bc, R, bh, _c, alpha), col in zip(boxes, cols)]


def render(task, qpos, target=None, cam="camera_front", W=320, H=240, v=None, rgb=TASK_RGB, dtype=np.float64):
    """(H, W, 3) uint8: oracle.render_oracle.render with the cameras, colours and light of the look"""
    v = default_variant() if v is None else v
    dt = np.dtype(dtype).type
    pos, X, Y, Z, fovy = camera(task, cam, v)
    pos, X, Y, Z = (np.asarray(a, dtype) for a in (pos, X, Y, Z))
    boxes = boxes_of(task, qpos, target, v, rgb)
    amb, dif = dt(v["ambient"]), dt(v["diffuse"])
    s = dt(2.0 * np.tan(np.radians(fovy) / 2) / H)
    vv, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx = (u + 0.5 - 0.5 * W).astype(dtype) * s
    sy = -(vv + 0.5 - 0.5 * H).astype(dtype) * s
    rd = sx[..., None] * X + sy[..., None] * Y - Z
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    assert rd.dtype == np.dtype(dtype)
    ro = pos
    tbest = np.full((H, W), 1e30, dtype)
    col = np.zeros((H, W, 3), dtype)
    nbest = np.zeros((H, W, 3), dtype); nbest[..., 2] = 1.0
    sky = np.zeros((H, W), bool)
    down = rd[..., 2] < dt(-1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = np.where(down, -ro[2] / rd[..., 2], dt(1e30))
    fx = np.where(down, ro[0] + np.where(down, tf, dt(0.0)) * rd[..., 0], dt(0.0))
    fy = np.where(down, ro[1] + np.where(down, tf, dt(0.0)) * rd[..., 1], dt(0.0))
    cell = ((np.floor(fx * dt(10)).astype(np.int64) + np.floor(fy * dt(10)).astype(np.int64)) & 1).astype(bool)
    col[down & cell] = np.asarray(v["floor_rgb"][0], dtype); col[down & ~cell] = np.asarray(v["floor_rgb"][1], dtype)
    tbest[down] = tf[down]
    a = np.clip(rd[..., 2] * dt(2), 0, 1)
    sk, sl = np.asarray(v["sky_rgb"], dtype), np.asarray(v["sky_slope"], dtype)
    skycol = np.stack([sk[0] + a * sl[0], sk[1] + a * sl[1], sk[2] + a * sl[2]], -1)
    col[~down] = skycol[~down]; sky[~down] = True
    talpha = np.zeros((H, W), dtype); tcol = np.zeros((H, W, 3), dtype)
    for (bc, R, bh, bcol, alpha) in boxes:
        R = np.asarray(R, dtype); bh = np.asarray(bh, dtype); bcol = np.asarray(bcol, dtype)
        ol = R.T @ (ro - np.asarray(bc, dtype))
        dl = rd @ R
        dls = np.where(np.abs(dl) > dt(1e-9), dl, dt(1e-9))
        t1 = (-bh - ol) / dls; t2 = (bh - ol) / dls
        tn = np.minimum(t1, t2); tx = np.maximum(t1, t2)
        tmin = tn.max(-1); tmax = tx.min(-1)
        hit = (tmin <= tmax) & (tmin > 0) & (tmin < tbest)
        ax = np.where(tmin == tn[..., 0], 0, np.where(tmin == tn[..., 1], 1, 2))
        sign = -np.sign(np.take_along_axis(dl, ax[..., None], -1)[..., 0]); sign[sign == 0] = 1.0
        n = R.T[ax] * sign[..., None]
        if alpha < 1.0:
            lam = amb + dif * np.maximum(0, -np.einsum("hwk,hwk->hw", n, rd))
            tcol = np.where(hit[..., None], lam[..., None] * bcol, tcol); talpha = np.where(hit, dt(alpha), talpha)
        else:
            tbest = np.where(hit, tmin, tbest); sky &= ~hit
            nbest[hit] = n[hit]; col[hit] = bcol
            talpha = np.where(hit, dt(0.0), talpha)
    lam = np.where(sky, dt(1.0), np.minimum(amb + dif * np.maximum(0, -np.einsum("hwk,hwk->hw", nbest, rd)), dt(1.0)))
    out = lam[..., None] * col
    out = np.where((talpha > 0)[..., None], talpha[..., None] * tcol + (1 - talpha[..., None]) * out, out)
    assert out.dtype == np.dtype(dtype)
    return np.clip(np.rint(out * dt(255.0)), 0, 255).astype(np.uint8)


def planes(task, qpos, target=None, cam="camera_front", W=320, H=240, v=None, depth_far=10.0, dtype=np.float64):
    """(depth (H, W) float32, seg (H, W) uint8) through the camera of variant `v`: the definitions of tests/planes_ref.py"""
    v = default_variant() if v is None else v
    dt = np.dtype(dtype).type
    pos, X, Y, Z, fovy = camera(task, cam, v)
    pos, X, Y, Z = (np.asarray(a, dtype) for a in (pos, X, Y, Z))
    boxes = render_oracle.scene(task, qpos, target)[1]
    s = dt(2.0 * np.tan(np.radians(fovy) / 2) / H)
    vv, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx = ((u + 0.5 - 0.5 * W).astype(dtype) * s)[..., None]
    sy = (-(vv + 0.5 - 0.5 * H).astype(dtype) * s)[..., None]
    d = sx * X + sy * Y - Z
    down = d[..., 2] / np.sqrt((d * d).sum(-1)) < dt(-1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(down, -pos[2] / np.where(down, d[..., 2], dt(-1.0)), dt(np.inf)).astype(dtype)
    seg = np.where(down, planes_ref.ID_FLOOR, planes_ref.ID_SKY).astype(np.uint8)
    marker = np.zeros((H, W), bool)
    for k, (bc, R, bh, _col, alpha) in enumerate(boxes):
        R = np.asarray(R, dtype); bh = np.asarray(bh, dtype)
        ol = R.T @ (pos - np.asarray(bc, dtype))
        dl = d @ R
        dls = np.where(np.abs(dl) > dt(1e-9), dl, dt(1e-9))
        t1 = (-bh - ol) / dls; t2 = (bh - ol) / dls
        tmin = np.minimum(t1, t2).max(-1); tmax = np.maximum(t1, t2).min(-1)
        hit = (tmin <= tmax) & (tmin > 0) & (tmin < t)
        if alpha < 1.0:
            marker = hit
        else:
            t = np.where(hit, tmin, t); seg = np.where(hit, np.uint8(k + planes_ref.ID_ARM0), seg)
    depth = np.minimum(t, dt(depth_far)).astype(np.float32)
    return depth, (seg | np.where(marker, planes_ref.MARKER_BIT, 0).astype(np.uint8)).astype(np.uint8)


# ---- the sampler (include/lcr.h): Philox-4x32-10 keyed by the seed, counter (global env id low, high, episode, block) ----
def _philox(seed, gid, episode, blk):
    M0, M1, mask = 0xD2511F53, 0xCD9E8D57, 0xFFFFFFFF
    c = [gid & mask, (gid >> 32) & mask, episode & mask, blk]
    k0, k1 = seed & mask, (seed >> 32) & mask
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & mask, (p0 >> 32) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & mask, (k1 + 0xBB67AE85) & mask
    return c


def sample(seed, gid, episode, K, lo, hi):
    """(variant, rgb[9] float32) of global env `gid` in its episode `episode`; lo, hi: the nine channel bounds (cube, second cube, marker)"""
    w = [x for b in range(3) for x in _philox(int(seed), int(gid), int(episode), b)]
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    rng = hi - lo
    u = np.array([(w[1 + j] >> 8) for j in range(9)], np.float32) * np.float32(1.0 / 16777216.0)
    val = np.minimum((u.astype(np.float64) * rng.astype(np.float64) + lo.astype(np.float64)).astype(np.float32), hi)   # (fma: one rounding)
    return (w[0] * K) >> 32, val
