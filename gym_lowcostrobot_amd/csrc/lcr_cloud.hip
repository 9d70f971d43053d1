// lcr_cloud.hip -- the point cloud (lcr_enable_point_cloud, include/lcr.h): one kernel that turns the selected cameras' segmentation, depth and colour planes into
// P world-frame points per env, behind the frame kernels on their stream.
//
// The mapping: a workgroup of four waves is ONE env; any n works, no workgroup spans envs.
//   pass 1  reads the segmentation planes only, 16 B per lane: thread t of round r takes the 16-pixel GROUP g = 256 r + t of the env's slots x H W / 16 groups (camera slot
//           major, so groups -- and the candidates inside them -- are in the order the header numbers candidates in).  It counts the group's candidates by byte compares
//           against the id mask and keeps the count (0 .. 16) as one byte in LDS.  Four rounds are in flight at a time: their loads are issued before any is counted, and
//           nothing in the loop crosses lanes.  64 consecutive groups are one SEGMENT; a thread per segment then adds its 64 count bytes up (16 dwords), and wave 0 turns the
//           <= 768 totals into an exclusive prefix (a run per lane, one wave scan); its end is M.
//   pass 2  one thread per output point j: candidate c = ((2 j + 1) M) / (2 P) in 64 bits; a binary search in the segment prefix, a walk over the segment's 64 count bytes
//           (a dword -- four groups -- at a time), a reload of that group's 16 id bytes to pick its r-th candidate; one depth float and, with colours, three bytes; the
//           point and its source index go out.
// Meanwhile the first thread of wave 3 has written the cameras' poses: front / top from the arguments or the env's look variant, the wrist camera from the link chain of
// the pose snapshot with the device code of the wrist kernel (lcr_wrist_pose.h).
// LDS: slots H W / 16 count bytes (49 152 B for three 512 x 512 cameras) + 3 088 B of prefix + 192 B of cameras.  HBM: one byte per pixel and slot, O(P) beside it.
#include <hip/hip_runtime.h>

#include "../../include/lcr.h"
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

template <bool COLORS>
__global__ __launch_bounds__(LCR_CLOUD_THREADS) void lcr_point_cloud_kernel(const LcrCloud A) {
    __shared__ __attribute__((aligned(16))) unsigned segpre[MAX_SEG + 4];   // exclusive prefix of the segment totals; [nseg] = M
    __shared__ __attribute__((aligned(16))) float cams[3][16];              // ro, X, Y, Z, s of every slot
    extern __shared__ __attribute__((aligned(16))) unsigned char cnt[];     // [nseg][64] candidates of every group

    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned env = blockIdx.x;
    if (env >= (unsigned)A.n) return;   // (uniform; the grid is exact)
    const unsigned pixels = (unsigned)A.W * (unsigned)A.H;
    const unsigned gpc = pixels >> 4;                                  // groups per camera
    const unsigned G = gpc * (unsigned)A.slots;                        // groups of the env
    const unsigned nseg = (G + LCR_CLOUD_SEG - 1) / LCR_CLOUD_SEG;
    const unsigned rounds = (G + LCR_CLOUD_THREADS - 1) / LCR_CLOUD_THREADS;
    const size_t env_px = (size_t)env * pixels;

    // ---- the cameras (one thread; the others are on their way through pass 1) ----
    if (tid == LCR_CLOUD_THREADS - 64) {
        for (int sl = 0; sl < A.slots; sl++) {
            LcrCam C;
            if (A.cam[sl] == LCR_CLOUD_CAM_WRIST) {
                float q[6];
                for (int j = 0; j < 6; j++) q[j] = A.qpos[(size_t)j * A.n + env];
                ArmFrames F;
                arm_frames(q, F);
                wrist_camera(F, A.mount, C);
            } else if (A.var) {
                C = A.var[A.variant[env]].cam[A.cam[sl]];
            } else {
                C = A.cam[sl] == LCR_CLOUD_CAM_FRONT ? A.front : A.top;
            }
            store_cam(cams[sl], C);
            float *po = A.pose + (size_t)sl * 13 * A.n + env;
            for (int k = 0; k < 13; k++) po[(size_t)k * A.n] = cams[sl][k];
        }
    }

    // ---- pass 1: candidates per group, UNROLL rounds in flight; then the totals per segment ----
    constexpr int UNROLL = 4;
    const unsigned ngrp = nseg * LCR_CLOUD_SEG;   // the count bytes in LDS: the env's groups and the filler of the last segment (which counts 0: the walk of pass 2 never enters it)
    for (unsigned r0 = 0; r0 < rounds; r0 += UNROLL) {
        v4u w[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const unsigned g = (r0 + u) * LCR_CLOUD_THREADS + tid;
            w[u] = v4u{0u, 0u, 0u, 0u};
            if (g < G) {
                const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
                const unsigned char *plane = sl == 0 ? A.seg[0] : sl == 1 ? A.seg[1] : A.seg[2];
                w[u] = *(const v4u *)(plane + env_px + (size_t)gi * 16);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const unsigned g = (r0 + u) * LCR_CLOUD_THREADS + tid;
            if (g < ngrp) cnt[g] = (unsigned char)(count_word(w[u].x, A.ids) + count_word(w[u].y, A.ids) + count_word(w[u].z, A.ids) + count_word(w[u].w, A.ids));
        }
    }
    __syncthreads();
    for (unsigned s = tid; s < nseg; s += LCR_CLOUD_THREADS) {
        const v4u *c4 = (const v4u *)(cnt + s * LCR_CLOUD_SEG);
        unsigned tot = 0;
#pragma unroll
        for (int k = 0; k < LCR_CLOUD_SEG / 16; k++) { const v4u c = c4[k]; tot += byte_sum(c.x) + byte_sum(c.y) + byte_sum(c.z) + byte_sum(c.w); }
        segpre[s] = tot;
    }
    __syncthreads();

    // ---- the prefix over the segment totals: lane l of wave 0 takes the run [l per, (l + 1) per) ----
    if (wave == 0) {
        const unsigned per = (nseg + 63) / 64;   // <= 12
        const unsigned a = lane * per, b = min(a + per, nseg);
        unsigned sum = 0;
        for (unsigned i = a; i < b; i++) sum += segpre[i];
        const unsigned incl = wave_scan_inclusive(sum, lane);
        unsigned run = incl - sum;
        for (unsigned i = a; i < b; i++) { const unsigned t = segpre[i]; segpre[i] = run; run += t; }
        if (lane == 63) segpre[nseg] = incl;     // M
    }
    __syncthreads();
    const unsigned M = segpre[nseg];
    if (tid == 0) A.count[env] = (int)M;

    // ---- pass 2: one thread per point ----
    const unsigned P = (unsigned)A.points;
    constexpr int C = COLORS ? 6 : 3;
    float *const out = A.out + (size_t)env * P * C;
    int *const src = A.source + (size_t)env * P;
    const unsigned *cntw = (const unsigned *)cnt;
    for (unsigned j = tid; j < P; j += LCR_CLOUD_THREADS) {
        float *o = out + (size_t)j * C;
        if (M == 0) {
#pragma unroll
            for (int k = 0; k < C; k++) o[k] = 0.f;
            src[j] = -1;
            continue;
        }
        const unsigned cand = (unsigned)(((unsigned long long)(2u * j + 1u) * (unsigned long long)M) / (unsigned long long)(2u * P));   // < M
        // the segment: the last s with segpre[s] <= cand (segpre[nseg] = M > cand)
        unsigned lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const unsigned mid = (lo + hi) >> 1;
            if (segpre[mid] <= cand) lo = mid; else hi = mid;
        }
        unsigned rem = cand - segpre[lo];   // < the segment's total
        // the group inside the segment: four count bytes at a time, then the bytes of that dword
        unsigned wi = lo * (LCR_CLOUD_SEG / 4), word = cntw[wi], ws = byte_sum(word);
        for (int k = 1; k < LCR_CLOUD_SEG / 4 && rem >= ws; k++) { rem -= ws; word = cntw[++wi]; ws = byte_sum(word); }
        unsigned g = wi * 4;
        for (int k = 0; k < 3 && rem >= (word & 0xffu); k++) { rem -= word & 0xffu; word >>= 8; g++; }
        g = min(g, G - 1u);   // (cand < M puts the group among the env's own; the clamp keeps every address below inside the planes whatever the counts hold)
        // its rem-th candidate
        const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
        const unsigned char *plane = sl == 0 ? A.seg[0] : sl == 1 ? A.seg[1] : A.seg[2];
        const v4u w = *(const v4u *)(plane + env_px + (size_t)gi * 16);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
        unsigned b = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned hit = is_candidate(ww[k >> 2] >> (8 * (k & 3)), A.ids);
            if (hit && rem == 0) b = k;
            rem -= hit;   // (wraps below zero once the candidate is found: never 0 again within 16 steps)
        }
        const unsigned pix = gi * 16 + b;
        const unsigned row = pix / (unsigned)A.W, px = pix - row * (unsigned)A.W;
        src[j] = (int)(sl * pixels + pix);
        const float *cam = cams[sl];
        const float *dplane = sl == 0 ? A.depth[0] : sl == 1 ? A.depth[1] : A.depth[2];
        const float t = dplane[env_px + pix];
        // the ray of the planes: d = sx X + sy Y - Z, sx and sy as the frame kernels form them (exact half-integers times s: one rounding each)
        const float sx = ((float)px + 0.5f - 0.5f * (float)A.W) * cam[12];
        const float sy = -((float)row + 0.5f - 0.5f * (float)A.H) * cam[12];
        const float dx = fmaf(sx, cam[3], fmaf(sy, cam[6], -cam[9]));
        const float dy = fmaf(sx, cam[4], fmaf(sy, cam[7], -cam[10]));
        const float dz = fmaf(sx, cam[5], fmaf(sy, cam[8], -cam[11]));
        o[0] = fmaf(t, dx, cam[0]);
        o[1] = fmaf(t, dy, cam[1]);
        o[2] = fmaf(t, dz, cam[2]);
        if constexpr (COLORS) {
            const unsigned char *frame = sl == 0 ? A.rgb[0] : sl == 1 ? A.rgb[1] : A.rgb[2];
            const unsigned char *c3 = frame + (env_px + pix) * 3;
            // the stack's float32 element: one correctly rounded multiply by the float32 constant 1 / 255
            o[3] = (float)c3[0] * (1.0f / 255.0f);
            o[4] = (float)c3[1] * (1.0f / 255.0f);
            o[5] = (float)c3[2] * (1.0f / 255.0f);
        }
    }
}

}  // namespace

size_t lcr_cloud_lds_bytes(int slots, int pixels) {
    const size_t G = (size_t)slots * (size_t)(pixels / 16);
    return (G + LCR_CLOUD_SEG - 1) / LCR_CLOUD_SEG * LCR_CLOUD_SEG;
}

int lcr_launch_point_cloud(const LcrCloud &A, void *stream) {
    if (!A.out || !A.count || !A.source || !A.pose || A.n <= 0 || A.slots < 1 || A.slots > 3 || A.W <= 0 || A.H <= 0 || A.W > 512 || A.H > 512) return -1;
    if (((size_t)A.W * A.H) % 16 || A.points < 64 || A.points > 8192 || A.points % 64 || (A.channels != 3 && A.channels != 6)) return -1;
    if (A.ids == 0 || (A.ids & ~0x7feu)) return -1;
    for (int i = 0; i < A.slots; i++) {
        if (!A.seg[i] || !A.depth[i] || (A.channels == 6 && !A.rgb[i])) return -1;
        if (A.cam[i] < LCR_CLOUD_CAM_FRONT || A.cam[i] > LCR_CLOUD_CAM_WRIST) return -1;
        if (A.cam[i] == LCR_CLOUD_CAM_WRIST && !A.qpos) return -1;
        if (A.cam[i] != LCR_CLOUD_CAM_WRIST && A.var && !A.variant) return -1;
    }
    const size_t lds = lcr_cloud_lds_bytes(A.slots, A.W * A.H);
    if (lds > (size_t)MAX_SEG * LCR_CLOUD_SEG) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (A.channels == 6) hipLaunchKernelGGL(lcr_point_cloud_kernel<true>, dim3((unsigned)A.n), dim3(LCR_CLOUD_THREADS), lds, st, A);
    else hipLaunchKernelGGL(lcr_point_cloud_kernel<false>, dim3((unsigned)A.n), dim3(LCR_CLOUD_THREADS), lds, st, A);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
