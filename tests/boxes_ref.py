"""A numpy model of the object boxes (include/lcr.h: "Object boxes"): the record of every env, camera slot and object from segmentation (and depth) planes, by the header's
words -- a boolean match plane per object, then minima, maxima, counts and sums over it.  No chunks, no segments, no atomics: nothing of how the kernel gets there."""
import numpy as np

MARKER = 0x80000000
FIELDS = ("x0", "y0", "x1", "y1", "count", "sum_x", "sum_y", "nearest")
NAMES = {"floor": 1 << 1, "arm": 0x7F << 2, "cube": 1 << 9, "cube2": 1 << 10, "marker": MARKER, "base_link": 1 << 2, **{f"link_{i}": 1 << (2 + i) for i in range(1, 7)}}


def mask_of(obj):
    """a name, a surface id 1 .. 10 or a tuple of those -> the 32-bit mask"""
    if isinstance(obj, str):
        return NAMES[obj]
    if isinstance(obj, (tuple, list)):
        m = 0
        for o in obj:
            m |= mask_of(o)
        return m
    assert 1 <= int(obj) <= 10, obj
    return 1 << int(obj)


def matches(seg, mask):
    """the header's match rule per byte: ((m >> (b & 0x7f)) & 1) != 0, or (m & MARKER) && (b & 0x80); an id of 31 or more selects no bit -> bool, the shape of seg"""
    seg = np.asarray(seg, np.uint8)
    ident = (seg & 0x7F).astype(np.int64)
    by_id = ((np.int64(mask & 0x7FFFFFFF) >> np.minimum(ident, 62)) & 1).astype(bool) & (ident < 31)
    if mask & MARKER:
        by_id = by_id | ((seg & 0x80) != 0)
    return by_id


def record(seg, mask, depth=None):
    """one [H][W] plane and one object -> the eight int64 values of the record (`nearest` the uint32 word as a non-negative int; the caller views it as int32)"""
    m = matches(seg, mask)
    if not m.any():
        return np.zeros(8, np.int64)
    r, c = np.nonzero(m)
    near = 0
    if depth is not None:
        near = int(np.ascontiguousarray(depth, np.float32).view(np.uint32)[m].min())
    return np.array([c.min(), r.min(), c.max() + 1, r.max() + 1, len(c), c.sum(), r.sum(), near], np.int64)


def boxes(segs, masks, depths=None):
    """segs: a list over the camera slots of [N][H][W] uint8; depths: None or the list of [N][H][W] float32; masks: the objects -> [N][S][O][8] int32 (`nearest` as the
    int32 with the word's bits)"""
    N, H, W = segs[0].shape
    out = np.zeros((N, len(segs), len(masks), 8), np.int64)
    rows, cols = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    for s, seg in enumerate(segs):
        words = None if depths is None else np.ascontiguousarray(depths[s], np.float32).view(np.uint32).astype(np.int64)
        for o, mask in enumerate(masks):   # (record() for all envs at once; tests/test_object_boxes_abi.py holds the two together)
            m = matches(seg, mask)
            in_col, in_row = m.sum(axis=1, dtype=np.int64), m.sum(axis=2, dtype=np.int64)   # [N][W], [N][H]
            rec = out[:, s, o]
            rec[:, 0] = (in_col > 0).argmax(axis=1)
            rec[:, 1] = (in_row > 0).argmax(axis=1)
            rec[:, 2] = W - (in_col[:, ::-1] > 0).argmax(axis=1)
            rec[:, 3] = H - (in_row[:, ::-1] > 0).argmax(axis=1)
            rec[:, 4] = in_col.sum(axis=1)
            rec[:, 5] = (in_col * cols).sum(axis=1)
            rec[:, 6] = (in_row * rows).sum(axis=1)
            if words is not None:
                rec[:, 7] = np.where(m, words, 0xFFFFFFFF).min(axis=(1, 2))
            rec[rec[:, 4] == 0] = 0
    assert (out[..., :7] >= 0).all() and (out[..., :7] < 2 ** 31).all()
    return out.astype(np.uint32).view(np.int32)
