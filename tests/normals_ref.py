"""The numpy model of the surface normals (include/lcr.h: "Surface normals", lcr_enable_normals), written from the header text, not from the kernel.  It is fed the
library's own depth and segmentation planes, the boxes it reports (`normals_boxes`: centre, X, Y, Z, half-extents of the nine opaque boxes as the kernel used them) and the
camera pose it reports (`normals_pose`: ro, X, Y, Z, s), so it needs no float32 forward kinematics of its own, and returns the (H, W, 4) int8 plane, exactly.

Every fused step of the rule goes through the exact fused multiply-add of tests/cloud_crop_ref.py (fp64 product and sum, rounded once; the rare elements near a rounding
midpoint recomputed in rational arithmetic); every other step is one numpy float32 operation, which rounds once, as the header asks.  rint is to nearest even, as rintf is.
tests/test_normals_abi.py holds the model to the slab test of the CPU ray caster; tests/test_gpu_normals.py holds the library's device buffers to planes()."""
import numpy as np

from tests.cloud_crop_ref import fmaf

F32 = np.float32
N_BOXES, BOX_FLOATS = 9, 15
FLOOR_CODE = 5


def dot(a, b):
    """lcr_arm.h's dot on (..., 3) float32 arrays: fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z))"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    m = a[..., 2] * b[..., 2]                      # one rounded float32 multiply
    assert m.dtype == F32
    return fmaf(a[..., 0], b[..., 0], fmaf(a[..., 1], b[..., 1], m))


def quantise(c):
    """clamp((int)rintf(127.0f * component), -127, 127) -> int8"""
    m = F32(127.0) * np.asarray(c, F32)
    assert m.dtype == F32
    return np.clip(np.rint(m), -127, 127).astype(np.int8)


def points(t, pose, rows, cols, H, W):
    """the pinned point of pixels (rows, cols) at depths t through the cameras pose (13, M): ro, X, Y, Z, s per pixel -> (M, 3) float32"""
    pose = np.asarray(pose, F32)
    hx = cols.astype(F32) + F32(0.5) - F32(0.5) * F32(W)      # exact half-integers
    hy = rows.astype(F32) + F32(0.5) - F32(0.5) * F32(H)
    sx = hx * pose[12]                                         # one rounded float32 multiply
    sy = -(hy * pose[12])
    assert sx.dtype == F32 and sy.dtype == F32
    p = np.empty((len(t), 3), F32)
    for k in range(3):
        dk = fmaf(sx, pose[3 + k], fmaf(sy, pose[6 + k], -pose[9 + k]))
        p[:, k] = fmaf(np.asarray(t, F32), dk, pose[k])
    return p


def face(p, box):
    """the face of points p (M, 3) on their boxes box (15, M): c, X, Y, Z, h -> (axis (M,), side (M,), margin (M,) float32: the largest e minus the second largest)"""
    box = np.asarray(box, F32)
    u = p - box[0:3].T                                         # one float32 subtraction per axis
    assert u.dtype == F32
    l = np.stack([dot(u, box[3 + 3 * k: 6 + 3 * k].T) for k in range(3)], axis=1)
    e = np.abs(l) - box[12:15].T                               # one float32 subtraction
    assert e.dtype == F32
    axis = np.where((e[:, 0] >= e[:, 1]) & (e[:, 0] >= e[:, 2]), 0, np.where(e[:, 1] >= e[:, 2], 1, 2))
    side = (np.take_along_axis(l, axis[:, None], 1)[:, 0] < F32(0.0)).astype(np.int64)
    es = np.sort(e, axis=1)
    return axis, side, es[:, 2] - es[:, 1]


def table(boxes, pose, frame):
    """the at most 55 quantised vectors of every env: boxes (9, 15, N), pose (13, N) -> (N, 56, 4) int8: word 0 the sky, word 1 the floor, word 2 + 6 b + 2 axis + side the
    face of box b"""
    boxes, pose = np.asarray(boxes, F32), np.asarray(pose, F32)
    N = boxes.shape[2]
    n = np.zeros((N, 56, 3), F32)
    w = np.zeros((N, 56), np.int8)
    n[:, 1] = (0.0, 0.0, 1.0); w[:, 1] = FLOOR_CODE
    for b in range(N_BOXES):
        for ax in range(3):
            A = boxes[b, 3 + 3 * ax: 6 + 3 * ax].T            # (N, 3)
            for side in range(2):
                j = 2 + 6 * b + 2 * ax + side
                n[:, j] = -A if side else A
                w[:, j] = 1 + 2 * ax + side
    if frame == "camera":
        n = np.stack([dot(n, pose[3 + 3 * k: 6 + 3 * k].T[:, None, :]) for k in range(3)], axis=-1)
    else:
        assert frame == "world", frame
    out = np.concatenate([quantise(n), w[..., None]], axis=-1)
    out[:, 0] = 0
    return out


def planes(depth, seg, boxes, pose, frame="world", detail=False):
    """depth (N, H, W) float32, seg (N, H, W) uint8, boxes (9, 15, N), pose (13, N) of ONE camera slot -> (N, H, W, 4) int8; with `detail` also the table index (N, H, W)
    and the margin (N, H, W) float32 (inf where the pixel shows no box)"""
    depth, seg = np.asarray(depth, F32), np.asarray(seg, np.uint8)
    boxes, pose = np.asarray(boxes, F32), np.asarray(pose, F32)
    N, H, W = seg.shape
    assert depth.shape == seg.shape and boxes.shape == (N_BOXES, BOX_FLOATS, N) and pose.shape == (13, N)
    ids = (seg & 0x7F).astype(np.int64)                        # the marker bit is ignored
    index = np.where(ids == 1, 1, 0)                           # sky, ids above 10: word 0
    margin = np.full((N, H, W), np.inf, F32)
    env, rows, cols = np.nonzero((ids >= 2) & (ids <= 10))
    if len(env):
        b = ids[env, rows, cols] - 2
        p = points(depth[env, rows, cols], pose[:, env], rows, cols, H, W)
        axis, side, m = face(p, boxes[b, :, env].T)
        index[env, rows, cols] = 2 + 6 * b + 2 * axis + side
        margin[env, rows, cols] = m
    out = table(boxes, pose, frame)[np.arange(N)[:, None, None], index]
    return (out, index, margin) if detail else out


def plane(depth, seg, boxes, pose, frame="world"):
    """one env: depth (H, W), seg (H, W), boxes (9, 15), pose (13,) -> (H, W, 4) int8"""
    return planes(np.asarray(depth)[None], np.asarray(seg)[None], np.asarray(boxes, F32)[:, :, None], np.asarray(pose, F32)[:, None], frame)[0]
