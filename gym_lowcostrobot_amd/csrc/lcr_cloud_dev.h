// lcr_cloud_dev.h -- the device code the kernels of the depth-plane observations share: the point cloud (lcr_cloud.hip, lcr_cloud_fps.hip, lcr_cloud_crop.hip), the voxel
// grid (lcr_voxel.hip), the heightmap (lcr_heightmap.hip), the surface normals (lcr_normals.hip) and the motion vectors (lcr_flow.hip).
// The small functions are here, each ONCE: the candidate test, the camera in LDS, the pinned point of a pixel (pinned_point), lcr_arm.h's dot with every step pinned (pinned_dot), the cell of a point along an axis (cell_axis),
// the float32 colour element and the wave sum.  The long blocks -- pass 1 and the prefix (lcr_cloud_pass1.inc.h), the way from a candidate number to its point
// (lcr_cloud_point.inc.h) and the cameras of an env (lcr_obs_cameras.inc.h) -- are statement lists that a kernel includes INSIDE its body: as text, not as functions,
// because the strided kernels then compile to the instructions they had before the farthest-point kernels existed (inlined functions went through the optimiser in another
// order and came out scheduled differently).  Folding the copies the units once held onto this file and the camera list left every unit's device assembly unchanged
// (profiles/obs_fold.txt).  The cloud's mapping is described at the top of lcr_cloud.hip.
#ifndef LCR_CLOUD_DEV_H
#define LCR_CLOUD_DEV_H
#include <hip/hip_runtime.h>

#include "lcr_cloud.h"
#include "lcr_wrist_pose.h"

using namespace lcrdev;

namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));   // 16 B: one group of segmentation bytes

constexpr int MAX_SEG = 3 * 512 * 512 / 16 / LCR_CLOUD_SEG;   // 768 segments at most

// 1 where byte b (a segmentation byte: id in the low 7 bits, bit 7 the marker) names a candidate surface.  Bits 0 and 11 .. 31 of ids are clear (the launcher refuses
// others): ids above 31 fall on bit 31, and a zero byte -- the sky, and the filler of a group beyond the env's last -- is never a candidate
__device__ __forceinline__ unsigned is_candidate(unsigned b, unsigned ids) { return (ids >> min(b & 0x7fu, 31u)) & 1u; }
__device__ __forceinline__ unsigned count_word(unsigned w, unsigned ids) {
    return is_candidate(w, ids) + is_candidate(w >> 8, ids) + is_candidate(w >> 16, ids) + is_candidate(w >> 24, ids);
}
// sum of the four bytes of w (each <= 16)
__device__ __forceinline__ unsigned byte_sum(unsigned w) { return (w * 0x01010101u) >> 24; }

__device__ __forceinline__ unsigned wave_scan_inclusive(unsigned v, unsigned lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(v, d, 64);
        if (lane >= (unsigned)d) v += o;
    }
    return v;
}

__device__ __forceinline__ void store_cam(float *sh, const LcrCam &C) {
    sh[0] = C.px; sh[1] = C.py; sh[2] = C.pz;
    sh[3] = C.xx; sh[4] = C.xy; sh[5] = C.xz; sh[6] = C.yx; sh[7] = C.yy; sh[8] = C.yz; sh[9] = C.zx; sh[10] = C.zy; sh[11] = C.zz;
    sh[12] = C.s;
}

// The header's point of pixel (row, px) at depth t through the camera `cam` (ro, X, Y, Z, s as store_cam lays them out), to the bit: hx and hy are exact half-integers
// (hW = W / 2, hH = H / 2), sx and sy one rounded multiply each, d = fmaf(sx, X, fmaf(sy, Y, - Z)) and p = fmaf(t, d, ro) per axis.  The empty asm statements hide each
// rounded result from the optimiser: under -ffast-math it may otherwise re-associate or contract across them.
__device__ __forceinline__ void pinned_point(unsigned px, unsigned row, float hW, float hH, float t, const float (&cam)[13], float (&p)[3]) {
    const float hx = (float)px + 0.5f - hW;
    const float hy = (float)row + 0.5f - hH;
    float sx = hx * cam[12];
    asm("" : "+v"(sx));
    float sy = -(hy * cam[12]);
    asm("" : "+v"(sy));
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float i = __builtin_fmaf(sy, cam[6 + k], -cam[9 + k]);
        asm("" : "+v"(i));
        float d = __builtin_fmaf(sx, cam[3 + k], i);
        asm("" : "+v"(d));
        float q = __builtin_fmaf(t, d, cam[k]);
        asm("" : "+v"(q));
        p[k] = q;
    }
}

// lcr_arm.h's dot, fmaf(a.x, b.x, fmaf(a.y, b.y, a.z b.z)), with every rounded step opaque
__device__ __forceinline__ float pinned_dot(float ax, float ay, float az, float bx, float by, float bz) {
    float m = az * bz;
    asm("" : "+v"(m));
    float i = __builtin_fmaf(ay, by, m);
    asm("" : "+v"(i));
    float d = __builtin_fmaf(ax, bx, i);
    asm("" : "+v"(d));
    return d;
}

// The header's cell of a point along one axis of a grid or a map: u = p - lo, one float32 subtraction; v = u inv, one rounded float32 multiply; inside iff u >= 0 && v < D;
// the index is (int)v.  Both operations are opaque to the optimiser
__device__ __forceinline__ bool cell_axis(float p, float lo, float inv, float D, unsigned &i) {
    float u = p - lo;
    asm("" : "+v"(u));
    float v = u * inv;
    asm("" : "+v"(v));
    i = (unsigned)(int)v;
    return u >= 0.0f && v < D;
}

// the stack's float32 element: one correctly rounded multiply by the float32 constant 1 / 255
__device__ __forceinline__ float elem(unsigned x) { return (float)x * (1.0f / 255.0f); }

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace

#endif
