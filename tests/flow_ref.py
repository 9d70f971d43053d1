"""The numpy model of the motion vectors (include/lcr.h: "Motion vectors", lcr_enable_motion_vectors), written from the header text, not from the kernel.  It is fed the
library's own depth and segmentation planes, `flow_valid`, and the history the library reports -- `flow_boxes` (2, 9, 15, N) and `flow_pose` (2, slots, 13, N), [0] now and
[1] before, exactly what the kernel used -- so it needs no float32 forward kinematics of its own, and returns the (N, H, W, 2) float16 plane, exactly.

Every fused step of the rule goes through the exact fused multiply-add of tests/cloud_crop_ref.py; the pinned point and lcr_arm.h's dot are those of tests/normals_ref.py;
every other step is one numpy float32 operation, which rounds once, as the header asks: numpy's float32 division is correctly rounded, and astype(float16) rounds once, to
nearest even.  tests/test_flow_abi.py holds the model to fp64 rigid motion; tests/test_gpu_flow.py holds the library's device buffers to planes()."""
import numpy as np

from tests.cloud_crop_ref import fmaf
from tests.normals_ref import dot, points

F32 = np.float32
N_BOXES, BOX_FLOATS = 9, 15


def static(boxes, pose):
    """bit-equality of the uint32 words now and before: boxes (2, 9, 15, N), pose (2, 13, N) -> (box static (9, N) bool: its 12 words c, A0, A1, A2; camera static (N,) bool:
    the slot's 13 words)"""
    bw = np.ascontiguousarray(boxes, F32).view(np.uint32)
    pw = np.ascontiguousarray(pose, F32).view(np.uint32)
    return (bw[0, :, :12] == bw[1, :, :12]).all(axis=1), (pw[0] == pw[1]).all(axis=0)


def chain(t, rows, cols, H, W, pose_now, pose_before, box_now=None, box_before=None, detail=False):
    """the header's chain for M pixels: depths t (M,), poses (13, M), boxes (15, M) or None for the floor (q = p) -> (M, 2) float32 (fx, fy), zeros where the point lies behind
    the previous camera; with `detail` also p and q (M, 3)"""
    pose_before = np.asarray(pose_before, F32)
    p = points(t, pose_now, rows, cols, H, W)
    if box_now is None:
        q = p
    else:
        box_now, box_before = np.asarray(box_now, F32), np.asarray(box_before, F32)
        u = p - box_now[0:3].T                                     # one float32 subtraction per axis
        assert u.dtype == F32
        l = [dot(u, box_now[3 + 3 * k: 6 + 3 * k].T) for k in range(3)]
        q = np.empty_like(p)
        for ax in range(3):
            q[:, ax] = fmaf(l[0], box_before[3 + ax], fmaf(l[1], box_before[6 + ax], fmaf(l[2], box_before[9 + ax], box_before[ax])))
    w = q - pose_before[0:3].T
    assert w.dtype == F32
    a, b, d = (dot(w, pose_before[3 + 3 * k: 6 + 3 * k].T) for k in range(3))
    den = (-d) * pose_before[12]
    assert den.dtype == F32
    ok = den > F32(0.0)
    safe = np.where(ok, den, F32(1.0))
    gx, gy = a / safe, b / safe                                    # ONE correctly rounded float32 division each
    hx = cols.astype(F32) + F32(0.5) - F32(0.5) * F32(W)           # exact
    hy = rows.astype(F32) + F32(0.5) - F32(0.5) * F32(H)
    f = np.stack([hx - gx, hy + gy], axis=1)
    assert f.dtype == F32
    f[~ok] = 0.0
    return (f, p, q) if detail else f


def planes(depth, seg, boxes, pose, valid, detail=False):
    """depth (N, H, W) float32, seg (N, H, W) uint8, boxes (2, 9, 15, N), pose (2, 13, N) of ONE camera slot, valid (N,) -> (N, H, W, 2) float16; with `detail` also the
    mask (N, H, W) of the pixels that ran the chain"""
    depth, seg = np.asarray(depth, F32), np.asarray(seg, np.uint8)
    boxes, pose = np.asarray(boxes, F32), np.asarray(pose, F32)
    N, H, W = seg.shape
    assert depth.shape == seg.shape and boxes.shape == (2, N_BOXES, BOX_FLOATS, N) and pose.shape == (2, 13, N) and np.shape(valid) == (N,)
    box_static, cam_static = static(boxes, pose)
    ids = (seg & 0x7F).astype(np.int64)                            # the marker bit is ignored
    on = np.asarray(valid).astype(bool)[:, None, None]
    b = np.clip(ids - 2, 0, N_BOXES - 1)
    env_of = np.arange(N)[:, None, None]
    moving = ~(box_static[b, env_of] & cam_static[env_of])
    floor = on & (ids == 1) & ~cam_static[:, None, None]
    box = on & (ids >= 2) & (ids <= 10) & moving
    out = np.zeros((N, H, W, 2), F32)                              # sky, ids above 10, static surfaces, envs that are not valid: (+0.0, +0.0)
    env, rows, cols = np.nonzero(floor)
    if len(env):
        out[env, rows, cols] = chain(depth[env, rows, cols], rows, cols, H, W, pose[0][:, env], pose[1][:, env])
    env, rows, cols = np.nonzero(box)
    if len(env):
        k = b[env, rows, cols]
        out[env, rows, cols] = chain(depth[env, rows, cols], rows, cols, H, W, pose[0][:, env], pose[1][:, env], boxes[0][k, :, env].T, boxes[1][k, :, env].T)
    with np.errstate(over="ignore"):
        half = out.astype(np.float16)                              # to nearest even; an overflow gives an infinity
    return (half, floor | box) if detail else half


def plane(depth, seg, boxes, pose, valid=1):
    """one env: depth (H, W), seg (H, W), boxes (2, 9, 15), pose (2, 13) -> (H, W, 2) float16"""
    return planes(np.asarray(depth)[None], np.asarray(seg)[None], np.asarray(boxes, F32)[..., None], np.asarray(pose, F32)[..., None], np.array([valid]))[0]
