"""The numpy model of the point cloud's farthest-point sampling (include/lcr.h: "The point cloud by farthest-point sampling"), written from the header text: the pool, the
greedy order and the distance pinned to the bit.  tests/test_cloud_fps_abi.py holds it to a brute-force greedy in exact rational arithmetic; tests/test_gpu_cloud_fps.py holds
the library's device buffers to it.

The distance.  dx, dy, dz are float32 subtractions and dx * dx a float32 multiply: numpy float32 arithmetic rounds each once.  A fused step fmaf(a, a, c) is the exact
a a + c rounded ONCE to float32.  The product of two float32 numbers is exact in fp64 (48 bits); the fp64 sum with c rounds once to 53 bits, and rounding that to float32
rounds a second time -- which differs from the single rounding only if the fp64 sum lies on a float32 rounding midpoint although the exact sum does not, or the other way
round.  Both can happen only if the fp64 sum is within one fp64 ulp of a midpoint: those elements (and every result in the float32 denormal range, where the midpoints lie
elsewhere) are recomputed with fractions.Fraction."""
from fractions import Fraction

import numpy as np

from tests import cloud_ref

F32, F64 = np.float32, np.float64
FALLBACKS = [0]   # how many elements the model has recomputed exactly (the tests read it to see that a constructed case takes that path)


def pool_sources(cand_row, Q):
    """cand_row: (slots H W,) bool, the candidates of one env in the header's numbering -> (Q,) int64 source of every pool entry, -1 without candidates"""
    idx = np.flatnonzero(cand_row)
    if idx.size == 0:
        return np.full(Q, -1, np.int64)
    return idx[cloud_ref.select(idx.size, Q)]


def points_at(depth, rgb, poses, source, H, W, colors):
    """the header's point formula in fp64 at given sources (N, P) (-1: zeros), as tests/cloud_ref.py's cloud() forms it at its own -> (N, P, C) float64"""
    N = source.shape[0]
    slot, pix, sx, sy = cloud_ref.rays(source, poses, H, W)
    env = np.arange(N)[:, None]
    pose = np.asarray(poses, F32).astype(F64)
    t = np.stack([np.asarray(d, F32).reshape(N, -1) for d in depth]).astype(F64)[slot, env, pix]
    pts = np.zeros(source.shape + (6 if colors else 3,), F64)
    for k in range(3):
        ro, X, Y, Z = pose[slot, k, env], pose[slot, 3 + k, env], pose[slot, 6 + k, env], pose[slot, 9 + k, env]
        pts[:, :, k] = ro + t * (sx * X + sy * Y - Z)
    if colors:
        c = np.stack([np.asarray(f, np.uint8).reshape(N, -1, 3) for f in rgb])[slot, env, pix]
        pts[:, :, 3:] = c.astype(F32) * cloud_ref.INV255
    pts[np.asarray(source) < 0] = 0.0
    return pts


def round_f32(x):
    """a Fraction -> the nearest float32, ties to even (exact: no intermediate rounding decides)"""
    if x == 0:
        return F32(0.0)
    r = F32(float(x))   # (near enough: the answer is r or a neighbour)
    best = None
    for c in (np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - x)
        even = (int(np.asarray(c, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, c, even)
    return F32(best[1])


def _fused(sq, a, c):
    """the fused step from the exact fp64 square sq of the float32 array a, and the float32 array c >= 0"""
    s = sq + c.astype(F64)                                     # one fp64 rounding
    r = s.astype(F32)
    low = s.view(np.uint64) & np.uint64(0x1FFFFFFF)           # the 29 bits of the fp64 significand below the float32 one; a midpoint is 0x10000000
    near = ((low - np.uint64(0x0FFFFFFF)) & np.uint64(0x1FFFFFFF)) <= np.uint64(2)   # low in {0x0fffffff, 0x10000000, 0x10000001}: within an fp64 ulp of a midpoint
    near |= (s != 0) & (s < F64(2.0 ** -126))                  # float32 denormals
    if near.any():
        af, cf, rf = np.broadcast_to(a, r.shape).reshape(-1), np.broadcast_to(c, r.shape).reshape(-1), r.reshape(-1).copy()
        for i in np.flatnonzero(near.reshape(-1)):
            rf[i] = round_f32(Fraction(float(af[i])) * Fraction(float(af[i])) + Fraction(float(cf[i])))
            FALLBACKS[0] += 1
        r = rf.reshape(r.shape)
    return r


def fused(a, c):
    """fmaf(a, a, c) for float32 arrays a, c >= 0: the exact a a + c, rounded once to float32"""
    a, c = np.asarray(a, F32), np.asarray(c, F32)
    a64 = a.astype(F64)
    return _fused(a64 * a64, a, c)   # (the product of two float32 numbers is exact in fp64)


def dist(p, q):
    """the header's distance between float32 points p (..., 3) and q (..., 3), bit for bit: one subtraction per axis, one rounded multiply, two fused steps"""
    d = np.asarray(p, F32) - np.asarray(q, F32)
    assert d.dtype == F32
    d64 = d.astype(F64)
    sq = d64 * d64                    # exact
    m = sq[..., 0].astype(F32)        # the float32 product dx * dx: the exact product rounded once
    return _fused(sq[..., 2], d[..., 2], _fused(sq[..., 1], d[..., 1], m))


def fps_order(points_f32, P):
    """points_f32: (..., Q, 3) float32 pool points -> (..., P) int64: the pool entries in greedy order.  mind starts at + inf; the entry with the largest mind goes out, ties
    to the lowest index (np.argmax returns the first); its mind becomes - 1; every other entry with mind >= 0 takes min(mind, dist)"""
    pts = np.asarray(points_f32)
    assert pts.dtype == F32 and pts.shape[-1] == 3
    lead, Q = pts.shape[:-2], pts.shape[-2]
    assert 0 < P <= Q
    pts = pts.reshape((-1, Q, 3))
    B = pts.shape[0]
    rows = np.arange(B)
    mind = np.full((B, Q), np.inf, F32)
    order = np.empty((B, P), np.int64)
    for k in range(P):
        i = np.argmax(mind, axis=1)
        order[:, k] = i
        d = dist(pts, pts[rows, i][:, None, :])
        mind = np.where(mind >= 0, np.minimum(mind, d), mind)
        mind[rows, i] = -1.0
    return order.reshape(lead + (P,))
