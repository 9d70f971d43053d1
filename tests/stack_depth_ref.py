"""numpy model of the observation stack with the depth channel (include/lcr.h: "The depth channel of the observation stack", lcr_enable_obs_stack_planes), written from the
header text.  Two parts:

  the element rule   depth_elements(d, dtype, depth_far): the element of float32 depth d -- fminf(d * inv_far, 1) in float32, that rounded to float16, or
                     min((int)fmaf(d, s255, 0.5), 255) -- with the two float32 constants the header fixes (constants(depth_far)).
  the slots          StackDepthRef: the colour model of tests/stack_ref.py (imported, unchanged) beside a stack of the RAW float32 depths that moves with it: push, refill
                     (repeat / zero), newest-slot rewrite.  A zero refill holds d = 0, whose element is zero bits in all three types, so the raw stack can be converted at
                     the end: expected(dtype, fill) interleaves per camera r, g, b, d -> (N, K, 4 ncam, H, W).

Everything is exact: the tests compare byte for byte.  The uint8 rule forms d * s255 + 0.5 in float64 and rounds it ONCE to float32 (the product of two float32 values is
exact in float64; the sum with 0.5 is then rounded twice, to float64 and to float32): tests/test_stack_depth_abi.py shows with exact rational arithmetic that this equals the
fused operation on the inputs it lists."""
import numpy as np

from tests import stack_ref
from tests.stack_ref import DTYPES, FILLS   # noqa: F401  (re-exported: the depth stack has the colour stack's types and refill rules)


def constants(depth_far):
    """(inv_far, s255): the float32 constants fixed when the stack is enabled, from depth_far as the library holds it (a float32)"""
    far = float(np.float32(depth_far))
    return np.float32(1.0 / far), np.float32(255.0 / far)


def depth_elements(d, dtype, depth_far):
    """the element of depth d (float32, metres, in [0, depth_far])"""
    d = np.asarray(d, np.float32)
    inv_far, s255 = constants(depth_far)
    if np.dtype(dtype) == np.uint8:
        t = (d.astype(np.float64) * np.float64(s255) + 0.5).astype(np.float32)   # fmaf(d, s255, 0.5f)
        return np.minimum(t.astype(np.int32), 255).astype(np.uint8)             # truncation toward zero (t >= 0.5), then the clamp
    m = d * inv_far                                                              # ONE rounded float32 multiply
    assert m.dtype == np.float32
    m = np.minimum(m, np.float32(1.0))
    return m if np.dtype(dtype) == np.float32 else m.astype(np.float16)          # (float16: round to nearest even)


def interleave(colours, depths):
    """colours (..., 3 ncam, H, W) and depths (..., ncam, H, W) of one element type -> (..., 4 ncam, H, W): every camera as r, g, b, d"""
    ncam = depths.shape[-3]
    assert colours.shape[-3] == 3 * ncam and colours.dtype == depths.dtype
    out = np.empty(colours.shape[:-3] + (4 * ncam,) + colours.shape[-2:], colours.dtype)
    for c in range(ncam):
        out[..., 4 * c:4 * c + 3, :, :] = colours[..., 3 * c:3 * c + 3, :, :]
        out[..., 4 * c + 3, :, :] = depths[..., c, :, :]
    return out


def rgbd_elements(frames, depths, dtype, depth_far):
    """the selected cameras' frames (n, H, W, 3) uint8 and depth planes (n, H, W) float32, in channel order -> their elements (n, 4 ncam, H, W)"""
    return interleave(stack_ref.convert(stack_ref.channels_first(frames), dtype), depth_elements(np.stack(depths, axis=1), dtype, depth_far))


class StackDepthRef:
    def __init__(self, frames, depths, K, depth_far):
        """enabling: every env is refilled from its current frames and depth planes"""
        self.K, self.depth_far = int(K), depth_far
        self.rgb = stack_ref.StackRef(frames, K)
        d = self._planes(depths)
        self.d32 = {fill: np.zeros((d.shape[0], self.K) + d.shape[1:], np.float32) for fill in FILLS}
        self._apply(d, np.ones(d.shape[0], bool), "newest")

    @staticmethod
    def _planes(depths):
        return np.stack([np.asarray(d, np.float32) for d in depths], axis=1)   # (N, ncam, H, W)

    def _apply(self, d, refill, other):
        """the slot semantics of the colour stack (stack_ref.StackRef._apply), on the raw depths"""
        refill = np.asarray(refill).astype(bool)
        for fill, s in self.d32.items():
            if other == "push" and self.K > 1:
                s[~refill, :-1] = s[~refill, 1:]
            s[refill, :-1] = d[refill, None] if fill == "repeat" else 0
            s[:, -1] = d

    def step(self, frames, depths, did_reset):
        self.rgb.step(frames, did_reset)
        self._apply(self._planes(depths), did_reset, "push")

    def reset(self, frames, depths, mask=None):
        self.rgb.reset(frames, mask)
        d = self._planes(depths)
        self._apply(d, np.ones(d.shape[0], bool) if mask is None else mask, "newest")

    def set_look(self, frames, depths):
        self.rgb.set_look(frames)
        d = self._planes(depths)
        self._apply(d, np.zeros(d.shape[0], bool), "newest")

    def expected(self, dtype="uint8", fill="repeat"):
        return interleave(self.rgb.expected(dtype, fill), depth_elements(self.d32[fill], dtype, self.depth_far))
