"""The numpy model of the point cloud inside a crop box (include/lcr.h: "The point cloud inside a crop box"), written from the header text: the point pinned to the bit, the
inside test, and the candidates that follow from both.  Selection, pool and greedy order are then those of tests/cloud_ref.py and tests/cloud_fps_ref.py, as they are.
tests/test_cloud_crop_abi.py holds the model to an evaluation in exact rational arithmetic; tests/test_gpu_cloud_crop.py holds the library's device buffers to it.

The fused multiply-add.  fmaf(a, b, c) is the exact a b + c rounded ONCE to float32.  The method is cloud_fps_ref._fused with two factors and either sign of c: the product
of two float32 numbers is exact in fp64 (48 bits); the fp64 sum with c rounds once to 53 bits, and rounding that to float32 rounds a second time -- which differs from the
single rounding only if the fp64 sum lies within one fp64 ulp of a float32 rounding midpoint.  Those elements, and every result in the float32 denormal range (where the
midpoints lie elsewhere), are recomputed with fractions.Fraction.  With c of the other sign the sum may cancel; a cancelled fp64 sum still carries 53 bits of the exact one,
so the same test covers it -- and it is then often EXACT and a true tie: a floor point is t d_z + ro_z with t = - ro_z / d_z rounded, and what is left of the 48-bit
product has some 25 bits.  An fp64 sum that is exact (the error term of Knuth's two-sum is zero) has been rounded once when it is rounded to float32, tie or not, so
those elements are not recomputed: without this a rollout spends its time in Fraction on ties the conversion already rounds to even."""
from fractions import Fraction

import numpy as np

from tests import cloud_ref
from tests.cloud_fps_ref import round_f32

F32, F64 = np.float32, np.float64
FALLBACKS = [0]   # how many elements fmaf has recomputed exactly (the tests read it to see that a constructed case takes that path)


def fmaf(a, b, c):
    """fmaf(a, b, c) for float32 arrays (broadcast against each other): the exact a b + c, rounded once to float32"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    shape = a.shape
    a, b, c = np.atleast_1d(a), np.atleast_1d(b), np.atleast_1d(c)   # (numpy scalars would warn about the wrap-around in the midpoint test below)
    p, c64 = a.astype(F64) * b.astype(F64), c.astype(F64)      # an exact product
    s = p + c64                                                # one fp64 rounding
    with np.errstate(invalid="ignore"):
        v = s - p
        inexact = ((p - (s - v)) + (c64 - v)) != 0             # two-sum: the error of that rounding, itself exact
    r = s.astype(F32)
    low = s.view(np.uint64) & np.uint64(0x1FFFFFFF)            # the 29 bits of the fp64 significand below the float32 one; a midpoint is 0x10000000
    near = ((low - np.uint64(0x0FFFFFFF)) & np.uint64(0x1FFFFFFF)) <= np.uint64(2)   # low in {0x0fffffff, 0x10000000, 0x10000001}: within an fp64 ulp of a midpoint
    near &= inexact                                            # (an exact sum is rounded once by the conversion above)
    near |= (s != 0) & (np.abs(s) < F64(2.0 ** -126))          # float32 denormals
    near &= np.isfinite(s)
    if near.any():
        af, bf, cf, rf = a.reshape(-1), b.reshape(-1), c.reshape(-1), r.reshape(-1).copy()
        for i in np.flatnonzero(near.reshape(-1)):
            rf[i] = round_f32(Fraction(float(af[i])) * Fraction(float(bf[i])) + Fraction(float(cf[i])))
            FALLBACKS[0] += 1
        r = rf.reshape(r.shape)
    return r.reshape(shape)


def points_f32(depth, poses, H, W):
    """the pinned point of EVERY pixel.  depth: list per slot of (N, H, W) float32; poses (slots, 13, N) float32: ro, X, Y, Z, s -> (N, slots H W, 3) float32"""
    poses = np.asarray(poses, F32)
    N = depth[0].shape[0]
    hx = (np.arange(W, dtype=F32) + F32(0.5) - F32(0.5) * F32(W))[None, None, :]   # exact half-integers
    hy = (np.arange(H, dtype=F32) + F32(0.5) - F32(0.5) * F32(H))[None, :, None]
    out = []
    for sl, d in enumerate(depth):
        t = np.asarray(d, F32).reshape(N, H, W)
        pose = poses[sl][:, :, None, None]                    # (13, N, 1, 1)
        sx = hx * pose[12]                                     # one rounded float32 multiply (numpy float32 arithmetic rounds once)
        sy = -(hy * pose[12])
        assert sx.dtype == F32 and sy.dtype == F32
        p = np.empty((N, H, W, 3), F32)
        for k in range(3):
            dk = fmaf(sx, pose[3 + k], fmaf(sy, pose[6 + k], -pose[9 + k]))
            p[..., k] = fmaf(t, dk, pose[k])
        out.append(p.reshape(N, H * W, 3))
    return np.concatenate(out, axis=1)


def inside(p, lo, hi):
    """lo_k <= p_k && p_k <= hi_k for all three k, as float32 comparisons -> bool (...,)"""
    p, lo, hi = np.asarray(p), np.asarray(lo, F32), np.asarray(hi, F32)
    assert p.dtype == F32
    with np.errstate(invalid="ignore"):
        return ((lo <= p) & (p <= hi)).all(axis=-1)


def candidates(seg, ids, depth, poses, box, points=None):
    """candidates by id (cloud_ref.candidates) whose pinned point lies inside box = (lo, hi) -> (N, slots H W) bool; `points`: points_f32 if the caller has it"""
    N, H, W = seg[0].shape
    p = points_f32(depth, poses, H, W) if points is None else points
    return cloud_ref.candidates(seg, ids) & inside(p, box[0], box[1])


def cloud(depth, seg, rgb, poses, spec, box):
    """the strided cloud inside the box, as cloud_ref.cloud returns it but with the pinned float32 points: points (N, P, C) float32, count (N,), source (N, P)"""
    P, ids, colors = int(spec["points"]), int(spec.get("ids", 0)) or cloud_ref.DEFAULT_IDS, bool(spec.get("colors", False))
    N, H, W = seg[0].shape
    p = points_f32(depth, poses, H, W)
    cand = candidates(seg, ids, depth, poses, box, p)
    count = cand.sum(axis=1).astype(np.int64)
    source = np.full((N, P), -1, np.int64)
    pts = np.zeros((N, P, 6 if colors else 3), F32)
    flat_rgb = np.concatenate([np.asarray(f, np.uint8).reshape(N, -1, 3) for f in rgb], axis=1) if colors else None
    for e in range(N):
        if count[e]:
            source[e] = np.flatnonzero(cand[e])[cloud_ref.select(count[e], P)]
            pts[e, :, :3] = p[e, source[e]]
            if colors:
                pts[e, :, 3:] = flat_rgb[e, source[e]].astype(F32) * cloud_ref.INV255
    return pts, count, source, cand, p
