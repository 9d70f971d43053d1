"""numpy model of the observation stack (include/lcr.h: lcr_enable_obs_stack).  It is fed the library's own uint8 frames after each call plus the flag bytes of that call
(did_reset of a step, the mask of a reset) and holds the expected stack [N][K][C][H][W] for both refill rules; `expected(dtype, fill)` gives it in any of the three element
types.  Everything is exact: the tests compare byte for byte."""
import numpy as np

CAMERAS = ("front", "top", "wrist")   # channel order
FILLS = ("repeat", "zero")
DTYPES = ("uint8", "float16", "float32")
INV255 = np.float32(1 / 255)          # 0x3b808081: the fp32 constant the float elements are multiplied by


def convert(x, dtype):
    """the element of source byte x: uint8 the byte; float32 ONE fp32 multiply by the fp32 constant 1 / 255 (not a division); float16 that value rounded to nearest even"""
    x = np.asarray(x, np.uint8)
    if np.dtype(dtype) == np.uint8:
        return x.copy()
    f = x.astype(np.float32) * INV255
    assert f.dtype == np.float32
    return f if np.dtype(dtype) == np.float32 else f.astype(np.float16)


def channels_first(frames):
    """frames: the selected cameras' (N, H, W, 3) uint8 arrays in the order front, top, wrist -> (N, 3 len(frames), H, W), each camera as r, g, b"""
    return np.concatenate([np.ascontiguousarray(np.moveaxis(np.asarray(f, np.uint8), -1, 1)) for f in frames], axis=1)


class StackRef:
    def __init__(self, frames, K):
        """enabling: every env is refilled from its current frames"""
        x = channels_first(frames)
        self.K = int(K)
        self.u8 = {fill: np.zeros((x.shape[0], self.K) + x.shape[1:], np.uint8) for fill in FILLS}
        self._apply(x, np.ones(x.shape[0], bool), "newest")

    def _apply(self, x, refill, other):
        """envs with refill set are refilled from x; the others are pushed (other == "push") or have their newest slot rewritten ("newest")"""
        refill = np.asarray(refill).astype(bool)
        for fill, s in self.u8.items():
            if other == "push" and self.K > 1:
                s[~refill, :-1] = s[~refill, 1:]
            s[refill, :-1] = x[refill, None] if fill == "repeat" else 0
            s[:, -1] = x

    def step(self, frames, did_reset):
        self._apply(channels_first(frames), did_reset, "push")

    def reset(self, frames, mask=None):
        """lcr_reset: masked envs (None: all) are refilled, the others keep their older slots; an all-zero mask is the redraw after set_state"""
        x = channels_first(frames)
        self._apply(x, np.ones(x.shape[0], bool) if mask is None else mask, "newest")

    def set_look(self, frames):
        x = channels_first(frames)
        self._apply(x, np.zeros(x.shape[0], bool), "newest")

    def expected(self, dtype="uint8", fill="repeat"):
        return convert(self.u8[fill], dtype)
