// lcr_cloud_dev.h -- the device code the point-cloud kernels share (lcr_cloud.hip: the strided cloud; lcr_cloud_fps.hip: farthest-point sampling from a strided pool).
// The small functions are here.  The two long blocks -- the cameras, pass 1 and the prefix (lcr_cloud_pass1.inc.h), and the way from a candidate number to its point
// (lcr_cloud_point.inc.h) -- are statement lists that a kernel includes INSIDE its body: as text, not as functions, because the strided kernels then compile to the
// instructions they had before the farthest-point kernels existed (inlined functions went through the optimiser in another order and came out scheduled differently).
// The mapping is described at the top of lcr_cloud.hip.
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

}  // namespace

#endif
