// lcr_flow.hip -- the motion vectors (lcr_enable_motion_vectors, include/lcr.h): one kernel that streams the selected cameras' segmentation planes and gives every pixel the
// backward optical flow of the surface point it shows -- current pixel position minus the position of the same point one control step ago --, as float16 x 2, behind the
// frame kernels on their stream.  A unit of its own: a handle without motion vectors launches nothing of this file.
//
// The mapping is that of lcr_normals.hip (a workgroup of four waves is ONE (env, camera slot); any n works, no workgroup spans envs or slots):
//   set-up    the last wave.  Its first lane obtains the slot's camera NOW (the one-slot form of the shared list lcr_obs_cameras.inc.h, as the normals kernel has it) and places
//             the nine opaque boxes from the pose snapshot the frames were drawn from (lcr_opaque_boxes.h).  Behind a barrier the wave's lanes load BEFORE -- the boxes and the
//             slot's pose of the previous step -- from the history, word by word, never recompute it, compare each word with its counterpart as uint32 and OR what differs
//             into one word of LDS: bit b box b moved (its 12 words c, X, Y, Z), bit 9 the camera moved (its 13 words).  The slot-0 workgroup writes the boxes and valid,
//             every workgroup its slot's pose: "now", what the host makes "before" ahead of the next launch.  The kernel reads only "before" and writes only "now".
//   scan      thread t of trip i takes the QUAD of four adjacent pixels 4 (256 i + t) ..: one dword of segmentation bytes, four trips in flight.  A pixel runs the chain of
//             the header iff bit `id` of an 11-bit mask made of the static word is set: the floor iff the camera moved, box b iff it or the camera moved.  Only lanes with
//             such a pixel load the 16 B of depth.  Both cameras are read from LDS at uniform addresses, the two box sets at a per-lane index (box stride 17 dwords).
//   output    one dword a pixel, one 16-byte store a quad.
//   restart   a run-time mode of the same kernel (every entry point that draws the frames but lcr_step): no history is read, "before" is written as a copy of "now", valid
//             is 0 and every quad stores zeros.  An env the step has auto-reset stores zeros in the same way.
// Nothing depends on the order lanes arrive in: every output word is a function of its own pixel and the set-up (the one LDS atomic ORs bits, which commutes).
// The rule is pinned to the bit (include/lcr.h).  THIS UNIT IS BUILT WITHOUT -ffast-math (build.py appends -fno-fast-math -ffp-contract=off): under it every spelling of the
// header's one correctly rounded division becomes a reciprocal and a multiply.  The shared helpers keep their opacity barriers, which cost nothing here.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lcr.h"
#include "lcr_flow.h"
#include "lcr_cloud_dev.h"      // store_cam, pinned_point, pinned_dot and the wrist pose: shared with the cloud kernels, the grid, the map and the normals
#include "lcr_opaque_boxes.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));   // 16 B: four depths

constexpr int BS = 17;                                 // dwords of a box in LDS: 15 used, an odd stride
constexpr unsigned SETUP = LCR_FLOW_THREADS - 64;      // the first lane of the last wave
constexpr unsigned BOX_WORDS = LCR_FLOW_BOXES * LCR_FLOW_BOX_FLOATS;
constexpr unsigned CAM_MOVED = 1u << LCR_FLOW_BOXES;   // bit 9 of the static word

// the flow word of pixel (row, px) with surface id `id` (1 .. 10) at depth t: the header's chain.  `cam` the pose now, `camp` before; `box`, `boxp` the nine boxes now and
// before in LDS
__device__ __forceinline__ unsigned flow_of(unsigned id, unsigned px, unsigned row, float hW, float hH, float t, const float (&cam)[13], const float (&camp)[13],
                                            const float *box, const float *boxp) {
    float p[3], q[3];
    pinned_point(px, row, hW, hH, t, cam, p);
    if (id == 1u) {   // the floor does not move
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    } else {
        const float *B = box + (id - 2u) * BS, *P = boxp + (id - 2u) * BS;
        const float u0 = p[0] - B[0], u1 = p[1] - B[1], u2 = p[2] - B[2];
        float l[3];
#pragma unroll
        for (int k = 0; k < 3; k++) l[k] = pinned_dot(u0, u1, u2, B[3 + 3 * k], B[4 + 3 * k], B[5 + 3 * k]);
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = __builtin_fmaf(l[0], P[3 + k], __builtin_fmaf(l[1], P[6 + k], __builtin_fmaf(l[2], P[9 + k], P[k])));
    }
    const float w0 = q[0] - camp[0], w1 = q[1] - camp[1], w2 = q[2] - camp[2];
    const float a = pinned_dot(w0, w1, w2, camp[3], camp[4], camp[5]);
    const float b = pinned_dot(w0, w1, w2, camp[6], camp[7], camp[8]);
    const float d = pinned_dot(w0, w1, w2, camp[9], camp[10], camp[11]);
    const float den = (-d) * camp[12];
    if (!(den > 0.0f)) return 0u;   // a point behind the previous camera
    const float gx = a / den, gy = b / den;   // ONE correctly rounded division each: this unit is built without -ffast-math
    const float hx = (float)px + 0.5f - hW, hy = (float)row + 0.5f - hH;   // (exact)
    const float fx = hx - gx, fy = hy + gy;
    const _Float16 x = (_Float16)fx, y = (_Float16)fy;   // to nearest even
    return (unsigned)__builtin_bit_cast(unsigned short, x) | (unsigned)__builtin_bit_cast(unsigned short, y) << 16;
}

__global__ __launch_bounds__(LCR_FLOW_THREADS) void lcr_flow_kernel(const LcrFlow A) {
    __shared__ __attribute__((aligned(16))) float cam_s[2][16];            // ro, X, Y, Z, s of the slot: now, before
    __shared__ float box_s[2][LCR_FLOW_BOXES * BS];                        // centre, X, Y, Z, half-extents of the nine boxes: now, before
    __shared__ unsigned moved_s;                                           // bit b: box b moved; bit 9: the camera moved

    constexpr int U = 4;                  // trips in flight
    const unsigned tid = threadIdx.x;
    const unsigned slots = (unsigned)A.slots, W = (unsigned)A.W;
    const unsigned slot = blockIdx.x % slots, env = blockIdx.x / slots;
    if (env >= (unsigned)A.n) return;   // (uniform; the grid is exact)
    const size_t n = (size_t)A.n;
    const unsigned pixels = (unsigned)A.W * (unsigned)A.H;
    const unsigned quads = pixels >> 2;   // (W is a multiple of 4: a quad lies in one row)
    const float hW = 0.5f * (float)A.W, hH = 0.5f * (float)A.H;   // (exact: W, H <= 512)
    const bool restart = A.restart != 0;
    const bool valid = !restart && A.flags[env] == 0;   // (uniform)

    // ---- set-up: the camera and the boxes NOW by one lane (the one-slot form of lcr_obs_cameras.inc.h, as lcr_normals.hip has it) ----
    if (tid == SETUP) {
        const int which = slot == 0 ? A.cam[0] : slot == 1 ? A.cam[1] : A.cam[2];
        LcrCam C;
        if (which == LCR_CLOUD_CAM_WRIST) {
            float q[6];
            for (int j = 0; j < 6; j++) q[j] = A.qpos[(size_t)j * n + env];
            ArmFrames F;
            arm_frames(q, F);
            wrist_camera(F, A.mount, C);
        } else if (A.var) {
            C = A.var[A.variant[env]].cam[which];
        } else {
            C = which == LCR_CLOUD_CAM_FRONT ? A.front : A.top;
        }
        store_cam(cam_s[0], C);
        OpaqueBoxes S;
        opaque_boxes(A.qpos, A.n, (int)env, A.ncube, S);
#pragma unroll
        for (int b = 0; b < LCR_FLOW_BOXES; b++) {
            float *B = box_s[0] + b * BS;
            B[0] = S.c[b].x; B[1] = S.c[b].y; B[2] = S.c[b].z;
            B[3] = S.X[b].x; B[4] = S.X[b].y; B[5] = S.X[b].z;
            B[6] = S.Y[b].x; B[7] = S.Y[b].y; B[8] = S.Y[b].z;
            B[9] = S.Z[b].x; B[10] = S.Z[b].y; B[11] = S.Z[b].z;
            B[12] = S.h[b].x; B[13] = S.h[b].y; B[14] = S.h[b].z;
        }
        moved_s = 0u;
    }
    __syncthreads();
    // ---- BEFORE from the history (on a restart: a copy of now), the words that moved, and what the model reads: boxes [2][9][15][n], pose [2][slots][13][n] ----
    if (tid >= SETUP) {
        const unsigned j = tid - SETUP;
        unsigned moved = 0u;
        for (unsigned i = j; i < BOX_WORDS; i += 64u) {
            const unsigned b = i / LCR_FLOW_BOX_FLOATS, k = i % LCR_FLOW_BOX_FLOATS;
            const float now = box_s[0][b * BS + k];
            float *g = A.boxes + (size_t)i * n + env;                  // [0][i][env]; [1] is BOX_WORDS n words on
            const float before = restart ? now : g[(size_t)BOX_WORDS * n];
            box_s[1][b * BS + k] = before;
            if (k < 12u && __float_as_uint(now) != __float_as_uint(before)) moved |= 1u << b;
            if (slot == 0) {
                g[0] = now;
                if (restart) g[(size_t)BOX_WORDS * n] = now;
            }
        }
        if (j < 13u) {
            const float now = cam_s[0][j];
            float *g = A.pose + ((size_t)slot * 13 + j) * n + env;     // [0][slot][j][env]; [1] is slots 13 n words on
            const float before = restart ? now : g[(size_t)slots * 13 * n];
            cam_s[1][j] = before;
            if (__float_as_uint(now) != __float_as_uint(before)) moved |= CAM_MOVED;
            g[0] = now;
            if (restart) g[(size_t)slots * 13 * n] = now;
        }
        if (moved) atomicOr(&moved_s, moved);
        if (slot == 0 && j == 0) A.valid[env] = valid ? 1 : 0;
    }
    __syncthreads();

    const size_t env_px = (size_t)env * pixels;
    unsigned *out = (slot == 0 ? A.out[0] : slot == 1 ? A.out[1] : A.out[2]) + env_px;
    if (!valid) {   // (uniform) a restart, or an env the step has auto-reset: the planes are zero
        for (unsigned g = tid; g < quads; g += LCR_FLOW_THREADS) *(v4u *)(out + (size_t)g * 4) = v4u{0u, 0u, 0u, 0u};
        return;
    }
    float cam[13], camp[13];
#pragma unroll
    for (int k = 0; k < 13; k++) { cam[k] = cam_s[0][k]; camp[k] = cam_s[1][k]; }
    // bit id: a pixel of surface id runs the chain -- the floor iff the camera moved, box b iff it or the camera moved
    const unsigned moved = moved_s;
    const unsigned chain = (moved & CAM_MOVED) ? 0x7FEu : (moved & 0x1FFu) << 2;
    const unsigned char *seg = (slot == 0 ? A.seg[0] : slot == 1 ? A.seg[1] : A.seg[2]) + env_px;
    const float *depth = (slot == 0 ? A.depth[0] : slot == 1 ? A.depth[1] : A.depth[2]) + env_px;

    // ---- scan ----
    for (unsigned g0 = tid; g0 < quads; g0 += LCR_FLOW_THREADS * U) {
        unsigned sw[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned g = g0 + (unsigned)u * LCR_FLOW_THREADS;
            sw[u] = g < quads ? *(const unsigned *)(seg + (size_t)g * 4) : 0u;   // (a quad beyond the plane's last: sky, no depth load, no store)
        }
        // the depths of the quads that hold a pixel that runs the chain, 16 B each: the loads of all trips in flight are issued before the first is used
        v4f d[U];
        bool runs[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned g = g0 + (unsigned)u * LCR_FLOW_THREADS;
            runs[u] = false;
#pragma unroll
            for (int j = 0; j < 4; j++) runs[u] |= (chain >> min((sw[u] >> (8 * j)) & 0x7Fu, 31u)) & 1u;   // (ids above 10 fall on clear bits)
            d[u] = v4f{0.f, 0.f, 0.f, 0.f};
            if (runs[u]) d[u] = *(const v4f *)(depth + (size_t)g * 4);   // (then g < quads)
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned g = g0 + (unsigned)u * LCR_FLOW_THREADS;
            if (g >= quads) continue;
            const unsigned first = g * 4u;
            v4u o = v4u{0u, 0u, 0u, 0u};
            if (runs[u]) {
                const unsigned row = first / W, px = first - row * W;   // (one division a quad, and only where something moves)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned id = (sw[u] >> (8 * j)) & 0x7Fu;   // the marker bit is ignored: the flow is that of the opaque surface the id names
                    if ((chain >> min(id, 31u)) & 1u) o[j] = flow_of(id, px + (unsigned)j, row, hW, hH, d[u][j], cam, camp, box_s[0], box_s[1]);
                }
            }
            *(v4u *)(out + (size_t)first) = o;
        }
    }
}

}  // namespace

int lcr_launch_flow(const LcrFlow &A, void *stream) {
    if (!A.boxes || !A.pose || !A.valid || !A.qpos || A.n <= 0 || A.slots < 1 || A.slots > 3 || A.W < 16 || A.H < 16 || A.W > 512 || A.H > 512) return -1;
    if (A.W % 4 || A.H % 4) return -1;   // a quad of four pixels lies in one row; every env's planes start at a 16-byte boundary
    if (A.ncube != 1 && A.ncube != 2) return -1;
    if (!A.restart && !A.flags) return -1;
    if ((size_t)A.n * A.slots > 0x7FFFFFFFu) return -1;
    for (int i = 0; i < A.slots; i++) {
        if (!A.seg[i] || !A.depth[i] || !A.out[i]) return -1;
        if ((size_t)A.seg[i] % 16 || (size_t)A.depth[i] % 16 || (size_t)A.out[i] % 16) return -1;   // 16-byte loads and stores (the allocations hand the planes out at 256-byte boundaries)
        if (A.cam[i] < LCR_CLOUD_CAM_FRONT || A.cam[i] > LCR_CLOUD_CAM_WRIST) return -1;
        if (A.cam[i] != LCR_CLOUD_CAM_WRIST && A.var && !A.variant) return -1;
    }
    hipLaunchKernelGGL(lcr_flow_kernel, dim3((unsigned)(A.n * A.slots)), dim3(LCR_FLOW_THREADS), 0, (hipStream_t)stream, A);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
