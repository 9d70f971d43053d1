"""Reference of the wrist camera's frames and planes (a plain helper of tests/test_wrist_abi.py and tests/test_gpu_wrist.py): numpy, fp64, one ray per pixel, no tiles, no
culling -- written from the definitions of include/lcr.h (lcr_wrist_camera), not from the kernels.

  mount    link 0 = world frame, 1 .. 6 = body frame of link_1 .. link_6; pos and MuJoCo xyaxes in that frame; fovy in degrees.  The numbers are float32, as the library
           receives them.
  axes     fp64: X normalised, Y minus its projection on X, normalised (oracle.render_oracle.camera's Gram-Schmidt), Z = X x Y; then rounded to float32.
  pose     ro = p_link + R_link pos, axes = R_link axes, with the link frames of the committed oracle (oracle.orc.link_frames); link 0: the numbers themselves.
  rays     s = 2 tan(fovy / 2) / H in fp64, rounded to float32; d = sx X_w + sy Y_w - Z_w.
  floor    seen only where the normalised d.z < -1e-6 AND ro.z > 0; otherwise the ray takes the sky formula a = clip(2 d.z, 0, 1) (segmentation 0, depth depth_far) and
           the floor limits no box.
  scene, shading, marker, depth and segmentation: those of the other cameras -- `render` follows tests/look_ref.render (and so oracle.render_oracle.render) operation by
           operation, `planes` tests/look_ref.planes.  With a look: the variant's floor, sky, light and arm colours and the env's colours; its camera offsets do not apply.
`dtype` = np.float32 runs the same ray arithmetic in fp32 on the fp64 scene and camera pose (the "twin": it models neither fp32 forward kinematics nor a hardware reciprocal).
`exact=True` keeps the finished axes and `s` in fp64: the mount of a scene camera then gives the very numbers oracle.render_oracle.render draws with.
"""
import numpy as np

from oracle import orc, render_oracle
from tests import look_ref, planes_ref

TASK_RGB = look_ref.TASK_RGB


def default_mount():
    """the values of lcr_wrist_camera_default"""
    return mount(5, (0.03, 0.0033, 0.045), (0, 1, 0, -0.4226, 0, 0.9063), 60.0)


def mount(link, pos, xyaxes, fovy_deg):
    """a mount with every number rounded to float32, as the library receives it"""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)   # noqa: E731
    return {"link": int(link), "pos": f(pos), "xyaxes": f(xyaxes), "fovy_deg": float(np.float32(fovy_deg))}


# the second mount of the GPU tests: on link_4, looking along its +x with a roll, fovy 90
OTHER_MOUNT = mount(4, (0.02, -0.01, 0.03), (0.1, 1.0, 0.2, -0.3, 0.1, 0.9), 90.0)


def scene_camera_mount(task, cam):
    """a world-frame mount with the pose of a scene camera, in fp64 as oracle.render_oracle.camera reads it (fovy 45: MuJoCo's default)"""
    rec = [c for c in render_oracle._G["scenes"][render_oracle.SCENE_OF_TASK[task]]["cameras"] if c["name"] == cam][0]
    xy = rec["xyaxes"] if "xyaxes" in rec else [1, 0, 0, 0, 1, 0]
    return {"link": 0, "pos": np.array(rec["pos"], float), "xyaxes": np.array(xy, float), "fovy_deg": 45.0}


def axes(m, exact=False):
    """X, Y, Z of the mount in its link's frame"""
    X, Y = np.array(m["xyaxes"][:3], float), np.array(m["xyaxes"][3:], float)
    X /= np.linalg.norm(X); Y -= (Y @ X) * X; Y /= np.linalg.norm(Y)
    Z = np.cross(X, Y)
    if exact:
        return X, Y, Z
    return tuple(a.astype(np.float32).astype(np.float64) for a in (X, Y, Z))


def camera(m, qpos, exact=False):
    """(position, X, Y, Z) of the camera in the world for arm pose qpos[:6]"""
    X, Y, Z = axes(m, exact)
    pos = np.asarray(m["pos"], float)
    if m["link"] == 0:
        return pos, X, Y, Z
    R, p = orc.link_frames(np.asarray(qpos, float)[:6])
    R, p = R[m["link"] - 1], p[m["link"] - 1]
    return p + R @ pos, R @ X, R @ Y, R @ Z


def _scale(m, H, exact):
    s = 2.0 * np.tan(np.radians(m["fovy_deg"]) / 2) / H
    return s if exact else float(np.float32(s))


def render(task, qpos, target=None, m=None, W=320, H=240, v=None, rgb=TASK_RGB, dtype=np.float64, exact=False):
    """(H, W, 3) uint8: tests/look_ref.render through the mounted camera, with the floor rule of a camera that may sit below the floor"""
    m = default_mount() if m is None else m
    v = look_ref.default_variant() if v is None else v
    dt = np.dtype(dtype).type
    pos, X, Y, Z = (np.asarray(a, dtype) for a in camera(m, qpos, exact))
    boxes = look_ref.boxes_of(task, qpos, target, v, rgb)
    amb, dif = dt(v["ambient"]), dt(v["diffuse"])
    s = dt(_scale(m, H, exact))
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
    down = (rd[..., 2] < dt(-1e-6)) & bool(ro[2] > 0)          # the floor rule
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


def planes(task, qpos, target=None, m=None, W=320, H=240, depth_far=10.0, dtype=np.float64, exact=False):
    """(depth (H, W) float32, seg (H, W) uint8) through the mounted camera: the definitions of tests/planes_ref.py with the floor rule"""
    m = default_mount() if m is None else m
    dt = np.dtype(dtype).type
    pos, X, Y, Z = (np.asarray(a, dtype) for a in camera(m, qpos, exact))
    boxes = render_oracle.scene(task, qpos, target)[1]
    s = dt(_scale(m, H, exact))
    vv, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx = ((u + 0.5 - 0.5 * W).astype(dtype) * s)[..., None]
    sy = (-(vv + 0.5 - 0.5 * H).astype(dtype) * s)[..., None]
    d = sx * X + sy * Y - Z
    down = (d[..., 2] / np.sqrt((d * d).sum(-1)) < dt(-1e-6)) & bool(pos[2] > 0)
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
