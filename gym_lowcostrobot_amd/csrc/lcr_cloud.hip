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
#include "lcr_cloud_dev.h"   // shared with the farthest-point kernels (lcr_cloud_fps.hip), as are the two statement lists included below

namespace {

template <bool COLORS>
__global__ __launch_bounds__(LCR_CLOUD_THREADS) void lcr_point_cloud_kernel(const LcrCloud A) {
    __shared__ __attribute__((aligned(16))) unsigned segpre[MAX_SEG + 4];   // exclusive prefix of the segment totals; [nseg] = M
    __shared__ __attribute__((aligned(16))) float cams[3][16];              // ro, X, Y, Z, s of every slot
    extern __shared__ __attribute__((aligned(16))) unsigned char cnt[];     // [nseg][64] candidates of every group

#include "lcr_cloud_pass1.inc.h"

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
#include "lcr_cloud_point.inc.h"
#undef LCR_CLOUD_SOURCE
#undef LCR_CLOUD_COLORS
    }
}

}  // namespace

size_t lcr_cloud_lds_bytes(int slots, int pixels) {
    const size_t G = (size_t)slots * (size_t)(pixels / 16);
    return (G + LCR_CLOUD_SEG - 1) / LCR_CLOUD_SEG * LCR_CLOUD_SEG;
}

bool lcr_cloud_args_ok(const LcrCloud &A) {
    if (!A.out || !A.count || !A.source || !A.pose || A.n <= 0 || A.slots < 1 || A.slots > 3 || A.W <= 0 || A.H <= 0 || A.W > 512 || A.H > 512) return false;
    if (((size_t)A.W * A.H) % 16 || A.points < 64 || A.points > 8192 || A.points % 64 || (A.channels != 3 && A.channels != 6)) return false;
    if (A.ids == 0 || (A.ids & ~0x7feu)) return false;
    for (int i = 0; i < A.slots; i++) {
        if (!A.seg[i] || !A.depth[i] || (A.channels == 6 && !A.rgb[i])) return false;
        if (A.cam[i] < LCR_CLOUD_CAM_FRONT || A.cam[i] > LCR_CLOUD_CAM_WRIST) return false;
        if (A.cam[i] == LCR_CLOUD_CAM_WRIST && !A.qpos) return false;
        if (A.cam[i] != LCR_CLOUD_CAM_WRIST && A.var && !A.variant) return false;
    }
    return lcr_cloud_lds_bytes(A.slots, A.W * A.H) <= (size_t)MAX_SEG * LCR_CLOUD_SEG;
}

int lcr_launch_point_cloud(const LcrCloud &A, void *stream) {
    if (!lcr_cloud_args_ok(A)) return -1;
    const size_t lds = lcr_cloud_lds_bytes(A.slots, A.W * A.H);
    hipStream_t st = (hipStream_t)stream;
    if (A.channels == 6) hipLaunchKernelGGL(lcr_point_cloud_kernel<true>, dim3((unsigned)A.n), dim3(LCR_CLOUD_THREADS), lds, st, A);
    else hipLaunchKernelGGL(lcr_point_cloud_kernel<false>, dim3((unsigned)A.n), dim3(LCR_CLOUD_THREADS), lds, st, A);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
