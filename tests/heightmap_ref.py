"""The numpy model of the heightmap (include/lcr.h: "The heightmap", lcr_enable_heightmap), written from the header text.  It is fed the library's own planes, frames,
reported camera poses and reported inv_cell, per camera slot (the selected cameras in the order front, top, wrist), and returns what the header defines, exactly: the map's
float32 bits, source, count and filled.

A candidate is one by the id rule of the point cloud; its point is the pinned chain of the voxel grid's section, evaluated with an exact fused multiply-add -- both through
tests/voxel_ref.py, which the grid's tests hold --; its cell along x and y is two float32 operations per axis, u = p - lo and v = u * inv_cell, which numpy's float32
arithmetic rounds once each; its height word is the bits of the float32 u_z = p_z - lo_z with the sign bit cleared; its key is a uint64, and a cell's value the maximum
key.  tests/test_heightmap_abi.py holds cell_of and height_of to an evaluation in exact rational arithmetic; tests/test_gpu_heightmap.py holds the library's device buffers to
heightmap()."""
import numpy as np

from tests.voxel_ref import cloud_crop_ref, cloud_ref   # the point chain and the id rule the grid's model uses

F32 = np.float32
ALL = np.uint64(0xFFFFFFFF)


def cell_of(p, lo, inv_cell, dims):
    """p (..., 3) float32 points; lo (3,) float32, inv_cell (2,) float32; dims (Hx, Hy) -> (inside along x and y (...,) bool, index (..., 2) int64: ix, iy, meaningful
    where inside)"""
    p, lo, inv = np.asarray(p), np.asarray(lo, F32), np.asarray(inv_cell, F32)
    assert p.dtype == F32 and inv.shape == (2,)
    u = p[..., :2] - lo[:2]                      # one float32 subtraction
    v = u * inv                                  # one rounded float32 multiply
    assert u.dtype == F32 and v.dtype == F32
    D = np.asarray(dims, np.int64)
    with np.errstate(invalid="ignore"):
        inside = ((u >= F32(0.0)) & (v < D.astype(F32))).all(axis=-1)   # - 0.0 >= 0.0: inside, in cell 0
        idx = np.where(inside[..., None], v, F32(0.0)).astype(np.int64)  # (int)v truncates; v >= 0 here
    return inside, idx


def height_of(p, lo_z, hi_z):
    """p (..., 3) float32 points -> (inside along z (...,) bool: u_z >= 0 and p_z <= hi_z, both faces included; hb (...,) uint32: the bits of u_z, sign bit cleared)"""
    p = np.asarray(p)
    assert p.dtype == F32
    pz = np.ascontiguousarray(p[..., 2])
    u = pz - F32(lo_z)                           # one float32 subtraction
    assert u.dtype == F32
    with np.errstate(invalid="ignore"):
        inside = (u >= F32(0.0)) & (pz <= F32(hi_z))
    return inside, u.view(np.uint32) & np.uint32(0x7FFFFFFF)


def keys(inside, hb):
    """the 64-bit key of every pixel of an env, 0 where it is no inside candidate.  inside (N, G) bool, hb (N, G) uint32 -> (N, G) uint64"""
    g = np.arange(inside.shape[1], dtype=np.uint64)
    k = (hb.astype(np.uint64) << np.uint64(32)) | (ALL - g)
    return np.where(inside, k, np.uint64(0))


def cells(key, lin, M):
    """per env: the maximum key among the candidates of every cell, 0 where none.  key (N, G) uint64, lin (N, G) -> (N, M) uint64"""
    N = key.shape[0]
    out = np.zeros((N, M), np.uint64)
    for e in range(N):
        g = np.flatnonzero(key[e])
        np.maximum.at(out[e], lin[e, g], key[e, g])
    return out


def heightmap(depth, seg, rgb, poses, spec, inv_cell, points=None):
    """depth / seg / rgb: lists per slot of (N, H, W) float32 / (N, H, W) uint8 / (N, H, W, 3) uint8 (rgb may be None without colours); poses (slots, 13, N) float32: ro, X, Y,
    Z, s; spec: dict with lo, hi, dims (Hx, Hy), ids (a mask, 0 = default), rgb (bool); inv_cell: the two float32 values the library reports.
    -> dict(heightmap (N, C, Hy, Hx) float32, source (N, Hy, Hx) int32, count (N,), filled (N,), key (N, Hy Hx) uint64, inside (N, slots H W) bool, by_id (N, slots H W) bool,
            lin (N, slots H W), hb (N, slots H W) uint32, points (N, slots H W, 3) float32)"""
    Hx, Hy = (int(d) for d in spec["dims"])
    M = Hx * Hy
    ids, colours = int(spec.get("ids", 0)) or cloud_ref.DEFAULT_IDS, bool(spec.get("rgb", False))
    N, H, W = seg[0].shape
    p = cloud_crop_ref.points_f32(depth, poses, H, W) if points is None else points
    by_id = cloud_ref.candidates(seg, ids)
    in_xy, idx = cell_of(p, spec["lo"], inv_cell, (Hx, Hy))
    in_z, hb = height_of(p, spec["lo"][2], spec["hi"][2])
    inside = by_id & in_xy & in_z
    lin = idx[..., 1] * Hx + idx[..., 0]
    key = cells(keys(inside, hb), lin, M)
    filled = key != 0
    src = np.where(filled, (ALL - (key & ALL)).astype(np.int64), -1)
    C = 4 if colours else 1
    out = np.zeros((N, C, M), F32)
    out[:, 0] = (key >> np.uint64(32)).astype(np.uint32).view(F32)      # + 0.0 where empty
    if colours:
        flat = np.concatenate([np.asarray(f, np.uint8).reshape(N, -1, 3) for f in rgb], axis=1)
        env = np.arange(N)[:, None]
        byte = np.where(filled[..., None], flat[env, np.maximum(src, 0)], 0).transpose(0, 2, 1)
        out[:, 1:] = byte.astype(F32) * cloud_ref.INV255                # the stack's element rule
    return {"heightmap": out.reshape(N, C, Hy, Hx), "source": src.reshape(N, Hy, Hx).astype(np.int32), "count": inside.sum(axis=1).astype(np.int64),
            "filled": filled.sum(axis=1).astype(np.int64), "key": key, "inside": inside, "by_id": by_id, "lin": lin, "hb": hb, "points": p}

