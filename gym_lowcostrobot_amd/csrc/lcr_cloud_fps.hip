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
    // this thread's best entry: the largest key, the lowest e among equals
    int bk = key[0];
    unsigned be = 0;

    // ---- the greedy loop: exactly K iterations, no exit that depends on data; its one barrier is reached by all 256 threads ----
    for (unsigned k = 0; k < K; k++) {
        // the wave's winner: largest key, lowest pool index
        const unsigned bi = tid + LCR_CLOUD_THREADS * be;
        const int wk = wave_max(bk);
        const unsigned wi = wave_min(bk == wk ? bi : 0xffffffffu);
        if (bi == wi) {   // one lane (pool indices are distinct; a lane with bk != wk has bi != wi, since the lane that gave wi has another tid or another e)
            const unsigned we = wi / LCR_CLOUD_THREADS;   // = be in this lane; uniform
            float sx = x[0], sy = y[0], sz = z[0];
            int ss = source[0];
#pragma unroll
            for (int e = 1; e < EMAX; e++)
                if (we == (unsigned)e) { sx = x[e]; sy = y[e]; sz = z[e]; ss = source[e]; }
            unsigned *s = slot[k & 1u][wave];
            s[0] = (unsigned)wk; s[1] = wi; s[2] = __float_as_uint(sx); s[3] = __float_as_uint(sy); s[4] = __float_as_uint(sz); s[5] = (unsigned)ss;
        }
        __syncthreads();
        // the chosen entry: largest key, lowest index of the four waves' (a wave without pool entries offers key - 1, which loses).  Every thread reads the same words: they
        // are taken as scalars
        const unsigned(*sl4)[8] = slot[k & 1u];
        int ck = __builtin_amdgcn_readfirstlane((int)sl4[0][0]);
        unsigned ci = (unsigned)__builtin_amdgcn_readfirstlane((int)sl4[0][1]), w = 0;
#pragma unroll
        for (unsigned v = 1; v < 4; v++) {
            const int vk = __builtin_amdgcn_readfirstlane((int)sl4[v][0]);
            const unsigned vi = (unsigned)__builtin_amdgcn_readfirstlane((int)sl4[v][1]);
            if (vk > ck || (vk == ck && vi < ci)) { ck = vk; ci = vi; w = v; }
        }
        const float cx = __uint_as_float(sl4[w][2]), cy = __uint_as_float(sl4[w][3]), cz = __uint_as_float(sl4[w][4]);
        if (tid == (k & (LCR_CLOUD_THREADS - 1u))) {
            float *o = out + (size_t)k * C;
            o[0] = cx; o[1] = cy; o[2] = cz;
            src[k] = (int)sl4[w][5];
        }
        // the chosen entry is never chosen again: its owner marks it (before the update, which leaves - 1 as it is)
        if (tid == (ci & (LCR_CLOUD_THREADS - 1u))) {
            const unsigned ce = ci / LCR_CLOUD_THREADS;   // (a scalar)
#pragma unroll
            for (int e = 0; e < EMAX; e++)
                if (ce == (unsigned)e) key[e] = KEY_CHOSEN;
        }
        // the update, and this thread's next best
        bk = KEY_CHOSEN; be = 0u;
#pragma unroll
        for (int e = 0; e < EMAX; e++) {
            if ((unsigned)e < E) {   // (uniform)
                key[e] = min(key[e], fps_dist(x[e], y[e], z[e], cx, cy, cz));
                if (key[e] > bk) { bk = key[e]; be = (unsigned)e; }
            }
        }
    }

    // ---- the colours of the chosen points, by the sources the loop wrote (other threads': behind the barrier, which orders the workgroup's global writes) ----
    if (C == 6) {
        __syncthreads();   // (uniform: C is an argument)
        for (unsigned k = tid; k < K; k += LCR_CLOUD_THREADS) {
            const unsigned s = (unsigned)src[k];
            const unsigned sl = min(s / pixels, (unsigned)A.slots - 1u), pix = min(s - sl * pixels, pixels - 1u);   // (in range by construction; the clamps keep the address inside the frames whatever was read)
            const unsigned char *frame = sl == 0 ? A.rgb[0] : sl == 1 ? A.rgb[1] : A.rgb[2];
            const unsigned char *c3 = frame + (env_px + pix) * 3;
            float *o = out + (size_t)k * C;
            // the stack's float32 element: one correctly rounded multiply by the float32 constant 1 / 255
            o[3] = (float)c3[0] * (1.0f / 255.0f);
            o[4] = (float)c3[1] * (1.0f / 255.0f);
            o[5] = (float)c3[2] * (1.0f / 255.0f);
        }
    }
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
