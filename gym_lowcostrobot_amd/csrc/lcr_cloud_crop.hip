// lcr_cloud_crop.hip -- the point cloud inside a crop box (lcr_enable_point_cloud_cropped with a crop, include/lcr.h): the strided cloud and the cloud by farthest-point
// sampling, of the candidates whose POINT lies inside an axis-aligned box of the world frame.  A unit of its own: the six kernels without a box (lcr_cloud.hip,
// lcr_cloud_fps.hip) stay what they are, and a handle without a crop launches them.
//
// The mapping is that of lcr_cloud.hip (a workgroup of four waves is ONE env; a count byte per 16-pixel group, the segment prefix and the cameras in LDS), with what the
// box changes:
//   cameras first   pass 1 needs the poses, so the thread that writes them does so before pass 1 and every thread waits for it -- the device code of the kernels without a
//                   box, the wrist pose from the link chain included.
//   pass 1          a group's 16 segmentation bytes are loaded and id-tested as before; a group with at least one candidate by id loads its 16 depth floats (four 16-byte
//                   loads), forms the point of every pixel by the chain the header pins (pinned_point) and tests it against the box (crop_scan).  The count byte is the
//                   number of pixels that pass both.  Four rounds are in flight in the strided kernels (one in the farthest-point kernels, which pay for registers in the
//                   waves their greedy loop needs): their segmentation loads are issued before any byte is tested, their depth loads before any point is formed.  W is a multiple of 4, not of 16: a group may straddle image rows, so row and px are stepped per pixel from one division a group.
//   pass 2 / pool   the group and the rank inside it come from the walk as before; the group's ids and depths are loaded again and crop_scan run again, which returns the
//                   rank-th pixel that passes and ITS point: the point that goes out is the point that was tested.  O(P) (O(Q)) groups: the recomputation is cheap, and
//                   the LDS footprint stays that of lcr_cloud_lds_bytes.
// The point is pinned to the bit (include/lcr.h).  This unit is built with the project's flags, -ffast-math among them; every rounded intermediate of pinned_point
// (lcr_cloud_dev.h: the one copy the grid, the map and the normals use too) is made opaque to the optimiser, as fps_dist's are, and the fused steps are explicit fmaf
// calls.  Denormals are kept.
// The greedy loop of the farthest-point kernels is the text lcr_cloud_fps.hip runs (lcr_cloud_fps_loop.inc.h).
#include <hip/hip_runtime.h>

#include "../../include/lcr.h"
#include "lcr_cloud.h"
#include "lcr_cloud_dev.h"
#include "lcr_cloud_fps_dev.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));   // 16 B: four depths of a group

// The 16 pixels of a group that starts at (row, px): w its segmentation bytes, d its depths.  Returns how many are candidates by id AND have their point inside the box
// (float32 comparisons on the bits pinned_point gives, lcr_cloud_dev.h).  PICK: the `want`-th of them (from 0) leaves its place in the group in b and its point in p.
template <bool PICK>
__device__ __forceinline__ unsigned crop_scan(const v4u w, const v4f (&d)[4], unsigned ids, unsigned row, unsigned px, unsigned W, float hW, float hH, const float *camsh,
                                              const LcrCloudCrop &BX, unsigned want, unsigned &b, float (&p)[3]) {
    float cam[13];
#pragma unroll
    for (int k = 0; k < 13; k++) cam[k] = camsh[k];
    const unsigned ww[4] = {w.x, w.y, w.z, w.w};
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const unsigned hit = is_candidate(ww[k >> 2] >> (8 * (k & 3)), ids);
        float q[3];
        pinned_point(px, row, hW, hH, d[k >> 2][k & 3], cam, q);
        const bool in = hit && BX.lo[0] <= q[0] && q[0] <= BX.hi[0] && BX.lo[1] <= q[1] && q[1] <= BX.hi[1] && BX.lo[2] <= q[2] && q[2] <= BX.hi[2];
        if constexpr (PICK) {
            if (in && n == want) { b = (unsigned)k; p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
        }
        n += in ? 1u : 0u;
        if (++px == W) { px = 0; row++; }
    }
    return n;
}

template <bool COLORS>
__global__ __launch_bounds__(LCR_CLOUD_THREADS) void lcr_point_cloud_crop_kernel(const LcrCloudCrop BX) {
    __shared__ __attribute__((aligned(16))) unsigned segpre[MAX_SEG + 4];   // exclusive prefix of the segment totals; [nseg] = M
    __shared__ __attribute__((aligned(16))) float cams[3][16];              // ro, X, Y, Z, s of every slot
    extern __shared__ __attribute__((aligned(16))) unsigned char cnt[];     // [nseg][64] candidates of every group
    const LcrCloud &A = BX.c;

#define LCR_CLOUD_CROP_ROUNDS 4
#include "lcr_cloud_crop_pass1.inc.h"
#undef LCR_CLOUD_CROP_ROUNDS

    // ---- pass 2: one thread per point ----
    const unsigned P = (unsigned)A.points;
    constexpr int C = COLORS ? 6 : 3;
    float *const out = A.out + (size_t)env * P * C;
    int *const src = A.source + (size_t)env * P;
    for (unsigned j = tid; j < P; j += LCR_CLOUD_THREADS) {
        float *o = out + (size_t)j * C;
        if (M == 0) {
#pragma unroll
            for (int k = 0; k < C; k++) o[k] = 0.f;
            src[j] = -1;
            continue;
        }
#define LCR_CLOUD_SOURCE src[j]
#define LCR_CLOUD_COLORS COLORS
#include "lcr_cloud_crop_point.inc.h"
#undef LCR_CLOUD_SOURCE
#undef LCR_CLOUD_COLORS
    }
}

// The workgroups per CU asked of the compiler (7 / 6 / 5 / 3 for 2 / 4 / 8 / 16 pool entries a thread) are the most it reaches without scratch: the greedy loop hides its
// latencies behind other waves, and without the hint the registers of pass 1 and of the scan set the kernel's count (90 / 98 / 118 / 157: 5 / 4 / 4 / 3 waves a SIMD)
template <int EMAX>
__global__ __launch_bounds__(LCR_CLOUD_THREADS, EMAX <= 2 ? 7 : EMAX <= 4 ? 6 : EMAX <= 8 ? 5 : 3) void lcr_point_cloud_crop_fps_kernel(const LcrCloudCrop BX) {
    __shared__ __attribute__((aligned(16))) unsigned segpre[MAX_SEG + 4];   // exclusive prefix of the segment totals; [nseg] = M
    __shared__ __attribute__((aligned(16))) float cams[3][16];              // ro, X, Y, Z, s of every slot
    __shared__ __attribute__((aligned(16))) unsigned slot[2][4][8];         // [iteration & 1][wave]: key, pool index, x, y, z, source of the wave's winner
    extern __shared__ __attribute__((aligned(16))) unsigned char cnt[];     // [nseg][64] candidates of every group
    const LcrCloud &A = BX.c;

#define LCR_CLOUD_CROP_ROUNDS 1   // (one round in flight: every round more holds 16 depth registers, which the greedy loop would pay for in waves)
#include "lcr_cloud_crop_pass1.inc.h"
#undef LCR_CLOUD_CROP_ROUNDS

    const unsigned K = (unsigned)A.points, Q = (unsigned)BX.pool;
    const unsigned C = (unsigned)A.channels;
    float *const out = A.out + (size_t)env * K * C;
    int *const src = A.source + (size_t)env * K;
    if (M == 0) {   // (uniform: every thread has read the same LDS word behind a barrier; nothing below is reached, no barrier is left waiting)
        for (unsigned k = tid; k < K; k += LCR_CLOUD_THREADS) {
            for (unsigned c = 0; c < C; c++) out[(size_t)k * C + c] = 0.f;
            src[k] = -1;
        }
        return;
    }

    // ---- the pool, as in lcr_cloud_fps.hip: entries tid + 256 e, in registers; an entry beyond Q has key - 1 for good.  Its points are the bits the box was tested on.
    //      The entries are made in a loop that is NOT unrolled and put into their registers by a chain of selects: the scan of a group (crop_scan) is long, and one copy of
    //      it beside the pool keeps the kernel's registers -- and with them the waves that hide the greedy loop's latencies -- near those of the kernels without a box ----
    float x[EMAX], y[EMAX], z[EMAX];
    int key[EMAX];
    int source[EMAX];
    const unsigned E = min((Q + LCR_CLOUD_THREADS - 1) / LCR_CLOUD_THREADS, (unsigned)EMAX);   // entries per thread in use (uniform)
#pragma unroll
    for (int e = 0; e < EMAX; e++) {
        x[e] = y[e] = z[e] = 0.f;
        key[e] = KEY_CHOSEN;
        source[e] = -1;
    }
#pragma nounroll
    for (unsigned en = 0; en < E; en++) {
        const unsigned j = tid + LCR_CLOUD_THREADS * en;
        if (j < Q) {
            const unsigned P = Q;   // (the selection rule with Q in place of P)
            float o[3];
            int so;
#define LCR_CLOUD_SOURCE so
#define LCR_CLOUD_COLORS false
#include "lcr_cloud_crop_point.inc.h"
#undef LCR_CLOUD_SOURCE
#undef LCR_CLOUD_COLORS
#pragma unroll
            for (int e = 0; e < EMAX; e++)
                if (en == (unsigned)e) { x[e] = o[0]; y[e] = o[1]; z[e] = o[2]; source[e] = so; key[e] = KEY_INF; }
        }
    }
#include "lcr_cloud_fps_loop.inc.h"
}

}  // namespace

int lcr_launch_point_cloud_crop(const LcrCloudCrop &B, void *stream) {
    const LcrCloud &A = B.c;
    if (!lcr_cloud_args_ok(A)) return -1;
    if (B.pool != 0 && (B.pool % 64 || B.pool < A.points || B.pool > LCR_CLOUD_MAX_POOL)) return -1;
    for (int k = 0; k < 3; k++)
        if (!(B.lo[k] <= B.hi[k])) return -1;   // (a NaN fails the comparison too)
    for (int i = 0; i < A.slots; i++)
        if ((size_t)A.depth[i] % 16) return -1;   // pass 1 loads the depths 16 bytes at a time (the planes' allocation hands them out at 256-byte boundaries)
    const size_t lds = lcr_cloud_lds_bytes(A.slots, A.W * A.H);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)A.n), block(LCR_CLOUD_THREADS);
    if (B.pool == 0) {
        if (A.channels == 6) hipLaunchKernelGGL(lcr_point_cloud_crop_kernel<true>, grid, block, lds, st, B);
        else hipLaunchKernelGGL(lcr_point_cloud_crop_kernel<false>, grid, block, lds, st, B);
    }
    // the kernel built for the fewest pool entries per thread that hold Q, as lcr_launch_point_cloud_fps chooses it
    else if (B.pool <= 2 * LCR_CLOUD_THREADS) hipLaunchKernelGGL(lcr_point_cloud_crop_fps_kernel<2>, grid, block, lds, st, B);
    else if (B.pool <= 4 * LCR_CLOUD_THREADS) hipLaunchKernelGGL(lcr_point_cloud_crop_fps_kernel<4>, grid, block, lds, st, B);
    else if (B.pool <= 8 * LCR_CLOUD_THREADS) hipLaunchKernelGGL(lcr_point_cloud_crop_fps_kernel<8>, grid, block, lds, st, B);
    else hipLaunchKernelGGL(lcr_point_cloud_crop_fps_kernel<16>, grid, block, lds, st, B);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
