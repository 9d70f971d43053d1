"""The numpy model of the voxel grid (include/lcr.h: "The voxel grid", lcr_enable_voxel_grid), written from the header text.  It is fed the library's own planes, frames,
reported camera poses and reported inv_cell, per camera slot (the selected cameras in the order front, top, wrist), and returns what the header defines, exactly: the grid's
bytes (or float32 bits), source, count and occupied.

A candidate is one by the id rule of the point cloud (cloud_ref.candidates); its point is the pinned chain of the crop section, evaluated with an exact fused multiply-add
(cloud_crop_ref.points_f32); its voxel is two float32 operations per axis, u = p - lo and v = u * inv_cell, which numpy's float32 arithmetic rounds once each, as the
header asks.  tests/test_voxel_abi.py holds voxel_of to an evaluation in exact rational arithmetic; tests/test_gpu_voxel.py holds the library's device buffers to grid()."""
import numpy as np

from tests import cloud_crop_ref, cloud_ref

F32 = np.float32


def voxel_of(p, lo, inv_cell, dims):
    """p (..., 3) float32 points; lo (3,), inv_cell (3,) float32; dims (Dx, Dy, Dz) -> (inside (...,) bool, index (..., 3) int64: ix, iy, iz, meaningful where inside)"""
    p, lo, inv = np.asarray(p), np.asarray(lo, F32), np.asarray(inv_cell, F32)
    assert p.dtype == F32
    u = p - lo                                   # one float32 subtraction
    v = u * inv                                  # one rounded float32 multiply
    assert u.dtype == F32 and v.dtype == F32
    D = np.asarray(dims, np.int64)
    with np.errstate(invalid="ignore"):
        inside = ((u >= F32(0.0)) & (v < D.astype(F32))).all(axis=-1)   # - 0.0 >= 0.0: inside, in cell 0
        idx = np.where(inside[..., None], v, F32(0.0)).astype(np.int64)  # (int)v truncates; v >= 0 here
    return inside, idx


def linear(idx, dims):
    """(..., 3) ix, iy, iz -> the voxel's place in [Dz][Dy][Dx]"""
    Dx, Dy, _ = dims
    return (idx[..., 2] * Dy + idx[..., 1]) * Dx + idx[..., 0]


def sources(inside, lin, V):
    """per env: the smallest global pixel index among the candidates of every voxel, - 1 where none.  inside (N, G) bool, lin (N, G) -> (N, V) int64"""
    N = inside.shape[0]
    src = np.full((N, V), -1, np.int64)
    for e in range(N):
        g = np.flatnonzero(inside[e])
        src[e, lin[e, g][::-1]] = g[::-1]        # (written from the largest g down: the smallest stays)
    return src


def grid(depth, seg, rgb, poses, spec, inv_cell, points=None):
    """depth / seg / rgb: lists per slot of (N, H, W) float32 / (N, H, W) uint8 / (N, H, W, 3) uint8 (rgb may be None without colours); poses (slots, 13, N) float32: ro, X, Y,
    Z, s; spec: dict with lo, dims, ids (a mask, 0 = default), rgb (bool), dtype ("uint8" | "float32"); inv_cell: the three float32 values the library reports.
    -> dict(voxels (N, C, Dz, Dy, Dx), source (N, Dz, Dy, Dx) int32, count (N,), occupied (N,), inside (N, slots H W) bool, by_id (N, slots H W) bool, lin (N, slots H W),
            points (N, slots H W, 3) float32)"""
    dims = tuple(int(d) for d in spec["dims"])
    Dx, Dy, Dz = dims
    V = Dx * Dy * Dz
    ids, colours = int(spec.get("ids", 0)) or cloud_ref.DEFAULT_IDS, bool(spec.get("rgb", False))
    N, H, W = seg[0].shape
    p = cloud_crop_ref.points_f32(depth, poses, H, W) if points is None else points
    by_id = cloud_ref.candidates(seg, ids)
    ins, idx = voxel_of(p, spec["lo"], inv_cell, dims)
    inside = by_id & ins
    lin = linear(idx, dims)
    src = sources(inside, lin, V)
    occ = src >= 0
    C = 4 if colours else 1
    vox = np.zeros((N, C, V), np.uint8)
    vox[:, 0] = np.where(occ, 255, 0)
    if colours:
        flat = np.concatenate([np.asarray(f, np.uint8).reshape(N, -1, 3) for f in rgb], axis=1)
        env = np.arange(N)[:, None]
        vox[:, 1:] = np.where(occ[..., None], flat[env, np.maximum(src, 0)], 0).transpose(0, 2, 1)
    if spec.get("dtype", "uint8") == "float32":
        vox = vox.astype(F32) * cloud_ref.INV255          # the stack's element rule
    return {"voxels": vox.reshape(N, C, Dz, Dy, Dx), "source": src.reshape(N, Dz, Dy, Dx).astype(np.int32), "count": inside.sum(axis=1).astype(np.int64),
            "occupied": occ.sum(axis=1).astype(np.int64), "inside": inside, "by_id": by_id, "lin": lin, "points": p}
