"""Reference of the depth and segmentation planes of the image observations (a plain helper of tests/test_image_planes_abi.py and
tests/test_gpu_image_planes.py): numpy, one ray per pixel, no tiles, no culling, no cached background -- written from the definitions of include/lcr.h, not from
the kernels.

Ray of pixel (row, px) of a camera with axes X, Y, Z at `ro`:  d = sx X + sy Y - Z  (un-normalised; sx, sy as the colour path has them).  d . (-Z) = 1, so the ray
parameter t is the distance along the optical axis in metres: the z-depth a depth camera reports.
  depth  float32  min(t of the nearest opaque surface, depth_far); floor t = -ro.z / d.z where the NORMALISED d.z < -1e-6 (the horizon rule of the colours), sky depth_far
  seg    uint8    low 7 bits: 0 sky, 1 floor, 2 .. 8 the seven arm boxes, 9 cube (Stack: the red one), 10 second cube; bit 7: the translucent target marker
                  (Push / PickPlace) covers the pixel in front of that surface.  The marker never writes depth and never is the id.
Cameras and boxes come from the committed oracle (oracle.render_oracle.camera / scene): the first seven boxes are the arm in id order, then the cube(s), then the marker
(alpha 0.3).  `dtype` = np.float32 runs the same ray arithmetic in fp32 on the fp64 scene (the "twin": it does not model fp32 forward kinematics or a hardware reciprocal).
"""
import numpy as np

from oracle import render_oracle

MARKER_BIT = 0x80
ID_SKY, ID_FLOOR, ID_ARM0, ID_CUBE, ID_CUBE2 = 0, 1, 2, 9, 10


def planes(task, qpos, target=None, cam="camera_front", W=320, H=240, depth_far=10.0, dtype=np.float64):
    """-> (depth (H, W) float32, seg (H, W) uint8) of one env"""
    dt = np.dtype(dtype).type
    pos, X, Y, Z = (np.asarray(a, dtype) for a in render_oracle.camera(task, cam))
    boxes = render_oracle.scene(task, qpos, target)[1]
    s = dt(2.0 * np.tan(np.radians(45.0) / 2) / H)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx = ((u + 0.5 - 0.5 * W).astype(dtype) * s)[..., None]
    sy = (-(v + 0.5 - 0.5 * H).astype(dtype) * s)[..., None]
    d = sx * X + sy * Y - Z
    assert d.dtype == np.dtype(dtype)
    down = d[..., 2] / np.sqrt((d * d).sum(-1)) < dt(-1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(down, -pos[2] / np.where(down, d[..., 2], dt(-1.0)), dt(np.inf)).astype(dtype)
    seg = np.where(down, ID_FLOOR, ID_SKY).astype(np.uint8)
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
            assert k == len(boxes) - 1, "the marker is the last box: every opaque surface has been seen"
            marker = hit
        else:
            assert k + ID_ARM0 <= ID_CUBE2
            t = np.where(hit, tmin, t); seg = np.where(hit, np.uint8(k + ID_ARM0), seg)
    depth = np.minimum(t, dt(depth_far)).astype(np.float32)
    return depth, (seg | np.where(marker, MARKER_BIT, 0).astype(np.uint8)).astype(np.uint8)


def id_class(seg):
    """visibility class of a segmentation byte: 0 floor / sky, 1 arm, 2 red cube, 3 blue cube"""
    i = seg & 0x7F
    return np.where(i < ID_ARM0, 0, np.where(i < ID_CUBE, 1, np.where(i == ID_CUBE, 2, 3))).astype(np.uint8)


def rgb_class(rgb):
    """the same class read off a colour frame of oracle.render_oracle.render: r = g = b is the (grey) arm, g = b = 0 < r the red cube, r = g = 0 < b the blue one,
    anything else floor or sky (meaningful where the translucent marker does not blend in)"""
    r, g, b = (rgb[..., i].astype(int) for i in range(3))
    return np.where((r == g) & (g == b), 1, np.where((g == 0) & (b == 0) & (r > 0), 2, np.where((r == 0) & (g == 0) & (b > 0), 3, 0))).astype(np.uint8)


def agree(depth, seg, depth_ref, seg_ref, rel):
    """per-pixel agreement: the segmentation byte is equal and |z - z_ref| <= rel z_ref"""
    return (seg == seg_ref) & (np.abs(depth.astype(np.float64) - depth_ref.astype(np.float64)) <= rel * depth_ref.astype(np.float64))
