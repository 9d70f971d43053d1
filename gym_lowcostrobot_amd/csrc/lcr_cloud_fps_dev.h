// lcr_cloud_fps_dev.h -- the device code the farthest-point kernels share (lcr_cloud_fps.hip: the pool of the point cloud; lcr_cloud_crop.hip: the pool of the cloud inside
// a crop box): the keys, the wave reductions and the distance the header pins to the bit.  The greedy loop itself is a statement list (lcr_cloud_fps_loop.inc.h), for the
// reason lcr_cloud_dev.h gives.
#ifndef LCR_CLOUD_FPS_DEV_H
#define LCR_CLOUD_FPS_DEV_H
#include <hip/hip_runtime.h>

#include "lcr_cloud.h"

namespace {

constexpr int KEY_INF = 0x7f800000;   // the key of mind = + inf
constexpr int KEY_CHOSEN = -1;        // the key of an entry that has gone out, and of one beyond the pool

// v of the lane the DPP control CTRL names; `idle` in a lane the control gives no source
template <int CTRL>
__device__ __forceinline__ int dpp_lane(int idle, int v) { return __builtin_amdgcn_update_dpp(idle, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ unsigned dpp_lane(unsigned idle, unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp((int)idle, (int)v, CTRL, 0xf, 0xf, false); }

// max / min of v over the 64 lanes of the wave, the same in every lane (a scalar).  Four steps inside the rows of 16 (lane ^ 1, lane ^ 2, mirror of the half row, mirror
// of the row: every lane then holds its row's result), then row_bcast15 (lane 15 of every row to the next row) and row_bcast31 (lane 31 to rows 2 and 3): lane 63 holds the
// wave's.  A lane without a source takes the operation's identity (which lets the compiler fold the move into the max / min).  Integer max and min are exact, associative
// and idempotent: no order of the steps can change the result.
#define LCR_WAVE_REDUCE(name, T, op, idle)                             \
    __device__ __forceinline__ T name(T v) {                           \
        v = op(v, dpp_lane<0xb1>(idle, v));  /* quad_perm [1,0,3,2] */ \
        v = op(v, dpp_lane<0x4e>(idle, v));  /* quad_perm [2,3,0,1] */ \
        v = op(v, dpp_lane<0x141>(idle, v)); /* row_half_mirror */     \
        v = op(v, dpp_lane<0x140>(idle, v)); /* row_mirror */          \
        v = op(v, dpp_lane<0x142>(idle, v)); /* row_bcast15 */         \
        v = op(v, dpp_lane<0x143>(idle, v)); /* row_bcast31 */         \
        return (T)__builtin_amdgcn_readlane((int)v, 63);               \
    }
LCR_WAVE_REDUCE(wave_max, int, max, (int)0x80000000)
LCR_WAVE_REDUCE(wave_min, unsigned, min, 0xffffffffu)
#undef LCR_WAVE_REDUCE

// The header's distance as the bits of a float32: dx, dy, dz one subtraction each, one rounded multiply, two fused steps.  The empty asm statements hide each rounded
// result from the optimiser: under -ffast-math it may otherwise re-associate the differences or contract the product into what follows.
// It is never NaN: the points are finite (a depth is at most depth_far, the cameras are finite), so are their differences and squares (|p| of the order of 10 m), and a sum
// of non-negative finite terms far below the float32 range is a finite non-negative number -- whose bits, as an integer, order as the floats do.
__device__ __forceinline__ int fps_dist(float ax, float ay, float az, float bx, float by, float bz) {
    float dx = ax - bx, dy = ay - by, dz = az - bz;
    asm("" : "+v"(dx));
    asm("" : "+v"(dy));
    asm("" : "+v"(dz));
    float m = dx * dx;
    asm("" : "+v"(m));
    return __float_as_int(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, m)));
}

}  // namespace

#endif
