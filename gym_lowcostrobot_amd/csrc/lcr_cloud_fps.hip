// lcr_cloud_fps.hip -- the point cloud by farthest-point sampling (lcr_enable_point_cloud_sampled with LCR_CLOUD_SAMPLE_FPS, include/lcr.h): P points in greedy order out of a
// pool of Q candidates that the strided rule picks, in one kernel, behind the frame kernels on their stream.  The pool never goes to HBM.
//
// The mapping: a workgroup of four waves is ONE env, as in lcr_cloud.hip, whose pass 1 and prefix run here unchanged (the same text, lcr_cloud_dev.h).
//   pool    pass 2 of lcr_cloud.hip with Q in place of P: thread t builds the pool entries i = t + 256 e (e < ceil(Q / 256) <= 16) and KEEPS them in registers -- x, y, z,
//           the source index and a key.  The key is the entry's `mind` of the header as a signed integer that orders the same way: the float's bits while the entry can
//           still be chosen (mind >= 0: the bits of non-negative floats ascend with their values; + inf is 0x7f800000), - 1 once it has been (the header's - 1).  The signed
//           min(key, bits(dist)) is then the header's update for both kinds of entry: - 1 stays - 1.
//   loop    P iterations, every one by all 256 threads, with ONE barrier each:
//             every thread holds its best entry (largest key, lowest e) from the update before;
//             a wave-level argmax in two DPP reductions -- the largest key, then the lowest pool index among the lanes that hold it;
//             the lane that holds the wave's winner puts key, index, x y z and source into the wave's LDS slot (slots of odd and even iterations alternate: a wave that
//             is an iteration ahead writes the other set, and cannot be two ahead, since the barrier in between needs every wave);
//             behind the barrier every thread reads the four slots and takes the largest key, lowest index: the chosen point, the same in every thread;
//             thread k mod 256 writes point k and its source; the thread that owns the chosen entry sets its key to - 1; every thread updates its entries against the
//             chosen x y z and finds its next best.
//   colours after the loop, a thread per point: the source index says which pixel of which frame.  They never enter the distance.
// The distance is pinned to the bit (include/lcr.h).  This unit is built with the project's flags, -ffast-math among them, so that everything but the distance is the code the
// strided kernel and the wrist kernel run; the three differences and the product of the distance are made opaque to the optimiser (fps_dist), and the two fused steps are
// explicit fmaf calls.  Denormals are kept (the project passes no flag that flushes them; the kernel descriptors say FLOAT_DENORM_MODE_32 = 3).
// LDS: that of lcr_cloud.hip + 256 B of slots.  Registers: 5 per pool entry, 80 at Q = 4096.
#include <hip/hip_runtime.h>

#include "../../include/lcr.h"
#include "lcr_cloud.h"
#include "lcr_cloud_dev.h"   // shared with the strided kernels (lcr_cloud.hip), as are the two statement lists included below
#include "lcr_cloud_fps_dev.h"   // shared with the kernels of the crop box (lcr_cloud_crop.hip), as is the greedy loop included below

namespace {


template <int EMAX>
__global__ __launch_bounds__(LCR_CLOUD_THREADS) void lcr_point_cloud_fps_kernel(const LcrCloudFps F) {
    __shared__ __attribute__((aligned(16))) unsigned segpre[MAX_SEG + 4];   // exclusive prefix of the segment totals; [nseg] = M
    __shared__ __attribute__((aligned(16))) float cams[3][16];              // ro, X, Y, Z, s of every slot
    __shared__ __attribute__((aligned(16))) unsigned slot[2][4][8];         // [iteration & 1][wave]: key, pool index, x, y, z, source of the wave's winner
    extern __shared__ __attribute__((aligned(16))) unsigned char cnt[];     // [nseg][64] candidates of every group
    const LcrCloud &A = F.c;

#include "lcr_cloud_pass1.inc.h"

    const unsigned K = (unsigned)A.points, Q = (unsigned)F.pool;
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

    // ---- the pool: entries tid + 256 e, in registers.  An entry beyond Q has key - 1 for good: it is never chosen (while k < P <= Q an entry with a key >= 0 exists) ----
    float x[EMAX], y[EMAX], z[EMAX];
    int key[EMAX];
    int source[EMAX];
    const unsigned E = min((Q + LCR_CLOUD_THREADS - 1) / LCR_CLOUD_THREADS, (unsigned)EMAX);   // entries per thread in use (uniform)
#pragma unroll
    for (int e = 0; e < EMAX; e++) {
        x[e] = y[e] = z[e] = 0.f;
        key[e] = KEY_CHOSEN;
        source[e] = -1;
        const unsigned j = tid + LCR_CLOUD_THREADS * (unsigned)e;
        if (j < Q) {
            const unsigned P = Q;   // (the selection rule with Q in place of P)
            float o[3];
#define LCR_CLOUD_SOURCE source[e]
#define LCR_CLOUD_COLORS false
#include "lcr_cloud_point.inc.h"
#undef LCR_CLOUD_SOURCE
#undef LCR_CLOUD_COLORS
            x[e] = o[0]; y[e] = o[1]; z[e] = o[2];
            key[e] = KEY_INF;
        }
    }
#include "lcr_cloud_fps_loop.inc.h"
}

}  // namespace

int lcr_launch_point_cloud_fps(const LcrCloudFps &F, void *stream) {
    const LcrCloud &A = F.c;
    if (!lcr_cloud_args_ok(A)) return -1;
    if (F.pool % 64 || F.pool < A.points || F.pool > LCR_CLOUD_MAX_POOL) return -1;
    const size_t lds = lcr_cloud_lds_bytes(A.slots, A.W * A.H);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)A.n), block(LCR_CLOUD_THREADS);
    // the kernel built for the fewest pool entries per thread that hold Q: 2 (Q <= 512), 4 (<= 1024), 8 (<= 2048), 16 (<= 4096)
    if (F.pool <= 2 * LCR_CLOUD_THREADS) hipLaunchKernelGGL(lcr_point_cloud_fps_kernel<2>, grid, block, lds, st, F);
    else if (F.pool <= 4 * LCR_CLOUD_THREADS) hipLaunchKernelGGL(lcr_point_cloud_fps_kernel<4>, grid, block, lds, st, F);
    else if (F.pool <= 8 * LCR_CLOUD_THREADS) hipLaunchKernelGGL(lcr_point_cloud_fps_kernel<8>, grid, block, lds, st, F);
    else hipLaunchKernelGGL(lcr_point_cloud_fps_kernel<16>, grid, block, lds, st, F);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
