"""numpy model of the point cloud (include/lcr.h: lcr_enable_point_cloud), written from the header text.  It is fed the library's own planes, frames and reported camera
poses, per camera slot (the selected cameras in the order front, top, wrist), and returns what the header defines: count and source exactly (integer decisions on the
segmentation bytes), the points in fp64 from the float32 inputs (the r g b channels are float32 values, exact in fp64)."""
import numpy as np

CAMERAS = ("front", "top", "wrist")   # slot order
DEFAULT_IDS = 0x7FC                   # arm (2 .. 8), cube (9), second cube (10)
IDS = {"floor": 1 << 1, "arm": 0x7F << 2, "cube": 1 << 9, "cube2": 1 << 10}
INV255 = np.float32(1 / 255)          # the stack's float32 rule


def ids_mask(ids):
    """a tuple of names / surface ids -> the mask; None or () -> the default"""
    m = 0
    for i in ids or ():
        m |= IDS[i] if isinstance(i, str) else 1 << int(i)
    return m or DEFAULT_IDS


def select(M, P):
    """the candidate of every output point: ((2 j + 1) M) // (2 P) in exact integers; M = 0: -1"""
    if M == 0:
        return np.full(P, -1, np.int64)
    return np.array([((2 * j + 1) * int(M)) // (2 * int(P)) for j in range(P)], np.int64)


def candidates(seg, ids):
    """seg: list per slot of (N, H, W) uint8 -> (N, slots H W) bool, candidates in the header's numbering (camera slot, then row-major pixel)"""
    flat = np.concatenate([np.asarray(s, np.uint8).reshape(s.shape[0], -1) for s in seg], axis=1)
    idn = (flat & 0x7F).astype(np.int64)                      # the marker bit 7 is ignored
    return ((np.int64(ids) >> np.minimum(idn, 63)) & 1).astype(bool)


def rays(source, poses, H, W):
    """per chosen candidate (source (N, P) int, -1: none): slot, pixel, sx, sy in fp64 from the float32 ray scale of the reported poses (slots, 13, N)"""
    src = np.maximum(np.asarray(source, np.int64), 0)
    slot, pix = src // (H * W), src % (H * W)
    row, px = pix // W, pix % W
    env = np.arange(src.shape[0])[:, None]
    s = np.asarray(poses, np.float32).astype(np.float64)[slot, 12, env]
    sx = (px + 0.5 - 0.5 * W) * s
    sy = -(row + 0.5 - 0.5 * H) * s
    return slot, pix, sx, sy


def cloud(depth, seg, rgb, poses, spec):
    """depth / seg / rgb: lists per slot of (N, H, W) float32 / (N, H, W) uint8 / (N, H, W, 3) uint8 (rgb may be None without colours); poses (slots, 13, N) float32: ro, X,
    Y, Z, s; spec: dict with points, ids (a mask, 0 = default), colors.  -> points (N, P, C) float64, count (N,) int64, source (N, P) int64"""
    P, ids, colors = int(spec["points"]), int(spec.get("ids", 0)) or DEFAULT_IDS, bool(spec.get("colors", False))
    N, H, W = seg[0].shape
    cand = candidates(seg, ids)
    count = cand.sum(axis=1).astype(np.int64)
    source = np.full((N, P), -1, np.int64)
    for e in range(N):
        if count[e]:
            source[e] = np.flatnonzero(cand[e])[select(count[e], P)]
    slot, pix, sx, sy = rays(source, poses, H, W)
    env = np.arange(N)[:, None]
    pose = np.asarray(poses, np.float32).astype(np.float64)
    t = np.stack([np.asarray(d, np.float32).reshape(N, -1) for d in depth]).astype(np.float64)[slot, env, pix]
    C = 6 if colors else 3
    pts = np.zeros((N, P, C), np.float64)
    for k in range(3):
        ro, X, Y, Z = pose[slot, k, env], pose[slot, 3 + k, env], pose[slot, 6 + k, env], pose[slot, 9 + k, env]
        pts[:, :, k] = ro + t * (sx * X + sy * Y - Z)
    if colors:
        c = np.stack([np.asarray(f, np.uint8).reshape(N, -1, 3) for f in rgb])[slot, env, pix]
        pts[:, :, 3:] = c.astype(np.float32) * INV255
    pts[count == 0] = 0.0
    return pts, count, source


def xyz_bound(depth, poses, source, H, W):
    """(N, P) per-component bound on |float32 point - fp64 point|: 8 2^-23 (|ro|_inf + t (|sx| + |sy| + 1)), see tests/test_gpu_cloud.py"""
    N = source.shape[0]
    slot, pix, sx, sy = rays(source, poses, H, W)
    env = np.arange(N)[:, None]
    pose = np.asarray(poses, np.float32).astype(np.float64)
    t = np.stack([np.asarray(d, np.float32).reshape(N, -1) for d in depth]).astype(np.float64)[slot, env, pix]
    ro = np.abs(pose[:, 0:3]).max(axis=1)[slot, env]
    return 8.0 * 2.0 ** -23 * (ro + t * (np.abs(sx) + np.abs(sy) + 1.0))
