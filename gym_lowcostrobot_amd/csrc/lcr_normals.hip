// lcr_normals.hip -- the surface normals (lcr_enable_normals, include/lcr.h): one kernel that streams the selected cameras' segmentation planes and gives every pixel the unit
// normal of the surface it shows and the face of the box it belongs to, as int8 x 4 -- behind the frame kernels on their stream.  A unit of its own: a handle without
// normals launches nothing of this file.
//
// The mapping (a workgroup of four waves is ONE (env, camera slot); any n works, no workgroup spans envs or slots):
//   set-up    the last wave.  Its first lane obtains the slot's camera exactly as the voxel kernel does (fixed camera, the env's look variant's, or the wrist pose from the
//             link chain) and places the nine opaque boxes from the pose snapshot the frames were drawn from (lcr_opaque_boxes.h, a copy of build_scene's text); behind a
//             barrier 56 of its lanes quantise one vector each into the FACE TABLE in LDS: word 0 four zeros (sky), word 1 the floor, word 2 + 6 b + 2 axis + side the face
//             of box b.  At most 55 vectors per (env, slot) are ever quantised, each once, so a pixel's word is a table look-up.  The slot-0 workgroup writes the boxes,
//             every workgroup its slot's pose: what the numpy model reads.
//   scan      thread t of trip i takes the QUAD of four adjacent pixels 4 (256 i + t) ..: one dword of segmentation bytes, so the 16-byte stores of a wave are 1 KiB in a
//             row.  Four trips are in flight: their segmentation loads are issued before any byte is tested, their depth loads before any point is formed.  (The other
//             mapping that was tried, a lane owning a 16-pixel chunk as in lcr_boxes.hip, took 1.6 times as long at 240 x 320: profiles/surface_normals.txt has both.)
//             A lane whose bytes are all sky or floor -- most of a frame -- answers from the table without loading depth; only lanes with a box pixel load the depth words
//             and run the chain of the header: the pinned point (pinned_point, lcr_cloud_dev.h), u = p - c, the three box coordinates, e = |l| - h, the
//             largest e.  The box is read from LDS at a per-lane index (box stride 17 dwords: the nine boxes lie in different banks).
//   output    one dword a pixel, 16-byte stores.
// Nothing depends on the order lanes arrive in and there are no atomics: every output word is a function of its own pixel and the set-up.
// The rule is pinned to the bit (include/lcr.h).  This unit is built with the project's flags, -ffast-math among them; every rounded intermediate is made opaque to the
// optimiser (pinned_point; pinned_dot, quantise), and the fused steps are explicit fmaf calls.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lcr.h"
#include "lcr_normals.h"
#include "lcr_cloud_dev.h"      // store_cam, pinned_point, pinned_dot and the wrist pose: shared with the cloud kernels, the grid and the map
#include "lcr_opaque_boxes.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));   // 16 B: four depths

constexpr int BS = 17;                                    // dwords of a box in LDS: 15 used, an odd stride
constexpr int TAB = 2 + 6 * LCR_NORMALS_BOXES;            // sky, floor, six faces a box
constexpr unsigned SETUP = LCR_NORMALS_THREADS - 64;      // the first lane of the last wave

// the header's quantisation of one component: clamp((int)rintf(127 c), -127, 127), as a byte
__device__ __forceinline__ unsigned quantise(float c) {
    float m = 127.0f * c;
    asm("" : "+v"(m));
    const int q = max(-127, min(127, (int)rintf(m)));
    return (unsigned)q & 0xFFu;
}

// the table index of box pixel (row, px) with surface id `id` (2 .. 10) at depth t: 2 + 6 box + 2 axis + side.  `box`: the nine boxes in LDS
__device__ __forceinline__ unsigned face_of(unsigned id, unsigned px, unsigned row, float hW, float hH, float t, const float (&cam)[13], const float *box) {
    float p[3];
    pinned_point(px, row, hW, hH, t, cam, p);
    const unsigned b = id - 2u;
    const float *B = box + b * BS;
    float u[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float v = p[k] - B[k];
        asm("" : "+v"(v));
        u[k] = v;
    }
    float l[3], e[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float *Ak = B + 3 + 3 * k;
        l[k] = pinned_dot(u[0], u[1], u[2], Ak[0], Ak[1], Ak[2]);
        float v = __builtin_fabsf(l[k]) - B[12 + k];
        asm("" : "+v"(v));
        e[k] = v;
    }
    const unsigned axis = (e[0] >= e[1] && e[0] >= e[2]) ? 0u : (e[1] >= e[2]) ? 1u : 2u;
    const float la = axis == 0u ? l[0] : axis == 1u ? l[1] : l[2];
    const unsigned side = la < 0.0f ? 1u : 0u;
    return 2u + 6u * b + 2u * axis + side;   // (b <= 8, axis <= 2, side <= 1: below TAB whatever the floats are)
}

__global__ __launch_bounds__(LCR_NORMALS_THREADS) void lcr_normals_kernel(const LcrNormals A) {
    __shared__ __attribute__((aligned(16))) float cam_s[16];                 // ro, X, Y, Z, s of the slot
    __shared__ float box_s[LCR_NORMALS_BOXES * BS];                          // centre, X, Y, Z, half-extents of the nine boxes
    __shared__ unsigned tab[64];                                             // the face table: TAB words

    constexpr int U = 4;                  // trips in flight
    const unsigned tid = threadIdx.x;
    const unsigned slots = (unsigned)A.slots, W = (unsigned)A.W;
    const unsigned slot = blockIdx.x % slots, env = blockIdx.x / slots;
    if (env >= (unsigned)A.n) return;   // (uniform; the grid is exact)
    const unsigned pixels = (unsigned)A.W * (unsigned)A.H;
    const unsigned quads = pixels >> 2;   // (W is a multiple of 4: a quad lies in one row)
    const float hW = 0.5f * (float)A.W, hH = 0.5f * (float)A.H;   // (exact: W, H <= 512)

    // ---- set-up: the camera and the boxes by one lane, the table by its wave.  The camera is the ONE-SLOT form of the shared list lcr_obs_cameras.inc.h (a workgroup here
    //      is one slot, and A.cam[] is read through a select chain): the same arithmetic and the same pose bits, kept as its own text ----
    if (tid == SETUP) {
        const int which = slot == 0 ? A.cam[0] : slot == 1 ? A.cam[1] : A.cam[2];
        LcrCam C;
        if (which == LCR_CLOUD_CAM_WRIST) {
            float q[6];
            for (int j = 0; j < 6; j++) q[j] = A.qpos[(size_t)j * A.n + env];
            ArmFrames F;
            arm_frames(q, F);
            wrist_camera(F, A.mount, C);
        } else if (A.var) {
            C = A.var[A.variant[env]].cam[which];
        } else {
            C = which == LCR_CLOUD_CAM_FRONT ? A.front : A.top;
        }
        store_cam(cam_s, C);
        float *po = A.pose + (size_t)slot * 13 * A.n + env;
        for (int k = 0; k < 13; k++) po[(size_t)k * A.n] = cam_s[k];
        OpaqueBoxes S;
        opaque_boxes(A.qpos, A.n, (int)env, A.ncube, S);
#pragma unroll
        for (int b = 0; b < LCR_NORMALS_BOXES; b++) {
            float *B = box_s + b * BS;
            B[0] = S.c[b].x; B[1] = S.c[b].y; B[2] = S.c[b].z;
            B[3] = S.X[b].x; B[4] = S.X[b].y; B[5] = S.X[b].z;
            B[6] = S.Y[b].x; B[7] = S.Y[b].y; B[8] = S.Y[b].z;
            B[9] = S.Z[b].x; B[10] = S.Z[b].y; B[11] = S.Z[b].z;
            B[12] = S.h[b].x; B[13] = S.h[b].y; B[14] = S.h[b].z;
        }
    }
    __syncthreads();
    if (tid >= SETUP) {
        const unsigned j = tid - SETUP;
        if (slot == 0)   // the boxes as every workgroup of this env uses them: [9][15][n]
            for (unsigned i = j; i < LCR_NORMALS_BOXES * LCR_NORMALS_BOX_FLOATS; i += 64u)
                A.boxes[(size_t)i * A.n + env] = box_s[(i / LCR_NORMALS_BOX_FLOATS) * BS + i % LCR_NORMALS_BOX_FLOATS];
        if (j < (unsigned)TAB) {
            unsigned word = 0u;
            if (j >= 1u) {
                float n[3] = {0.f, 0.f, 1.f};   // the floor: the + Z face of the world
                unsigned w = 5u;
                if (j >= 2u) {
                    const unsigned b = (j - 2u) / 6u, f = (j - 2u) % 6u;
                    const float *Ak = box_s + b * BS + 3 + 3 * (f >> 1);
                    const bool negative = f & 1u;
                    for (int k = 0; k < 3; k++) n[k] = negative ? -Ak[k] : Ak[k];
                    w = 1u + f;
                }
                if (A.frame == LCR_NORMALS_CAMERA) {
                    float c[3];
                    for (int k = 0; k < 3; k++) c[k] = pinned_dot(n[0], n[1], n[2], cam_s[3 + 3 * k], cam_s[4 + 3 * k], cam_s[5 + 3 * k]);
                    for (int k = 0; k < 3; k++) n[k] = c[k];
                }
                word = quantise(n[0]) | quantise(n[1]) << 8 | quantise(n[2]) << 16 | w << 24;
            }
            tab[j] = word;
        }
    }
    __syncthreads();

    float cam[13];
#pragma unroll
    for (int k = 0; k < 13; k++) cam[k] = cam_s[k];
    const unsigned floor_word = tab[1];
    const size_t env_px = (size_t)env * pixels;
    const unsigned char *seg = (slot == 0 ? A.seg[0] : slot == 1 ? A.seg[1] : A.seg[2]) + env_px;
    const float *depth = (slot == 0 ? A.depth[0] : slot == 1 ? A.depth[1] : A.depth[2]) + env_px;
    unsigned *out = (slot == 0 ? A.out[0] : slot == 1 ? A.out[1] : A.out[2]) + env_px;

    // ---- scan ----
    for (unsigned g0 = tid; g0 < quads; g0 += LCR_NORMALS_THREADS * U) {
        unsigned sw[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned g = g0 + (unsigned)u * LCR_NORMALS_THREADS;
            sw[u] = g < quads ? *(const unsigned *)(seg + (size_t)g * 4) : 0u;   // (a quad beyond the plane's last: sky, no depth load, no store)
        }
        // the depths of the quads that hold a box pixel, 16 B each: the loads of all trips in flight are issued before the first is used
        v4f d[U];
        bool box[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned g = g0 + (unsigned)u * LCR_NORMALS_THREADS;
            box[u] = false;
#pragma unroll
            for (int j = 0; j < 4; j++) box[u] |= ((sw[u] >> (8 * j)) & 0x7Fu) - 2u <= 8u;
            d[u] = v4f{0.f, 0.f, 0.f, 0.f};
            if (box[u]) d[u] = *(const v4f *)(depth + (size_t)g * 4);   // (then g < quads)
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned g = g0 + (unsigned)u * LCR_NORMALS_THREADS;
            if (g >= quads) continue;
            const unsigned first = g * 4u;
            unsigned row = 0u, px = 0u;
            if (box[u]) { row = first / W; px = first - row * W; }   // (one division a quad, and only where a box shows)
            v4u o;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned id = (sw[u] >> (8 * j)) & 0x7Fu;   // the marker bit is ignored: the normal is that of the opaque surface the id names
                unsigned word = id == 1u ? floor_word : 0u;
                if (id - 2u <= 8u) word = tab[face_of(id, px + (unsigned)j, row, hW, hH, d[u][j], cam, box_s)];
                o[j] = word;
            }
            *(v4u *)(out + first) = o;
        }
    }
}

}  // namespace

int lcr_launch_normals(const LcrNormals &A, void *stream) {
    if (!A.boxes || !A.pose || !A.qpos || A.n <= 0 || A.slots < 1 || A.slots > 3 || A.W < 16 || A.H < 16 || A.W > 512 || A.H > 512) return -1;
    if (A.W % 4 || A.H % 4) return -1;   // a quad of four pixels lies in one row; every env's planes start at a 16-byte boundary
    if (A.frame != LCR_NORMALS_WORLD && A.frame != LCR_NORMALS_CAMERA) return -1;
    if (A.ncube != 1 && A.ncube != 2) return -1;
    if ((size_t)A.n * A.slots > 0x7FFFFFFFu) return -1;
    for (int i = 0; i < A.slots; i++) {
        if (!A.seg[i] || !A.depth[i] || !A.out[i]) return -1;
        if ((size_t)A.seg[i] % 16 || (size_t)A.depth[i] % 16 || (size_t)A.out[i] % 16) return -1;   // 16-byte loads and stores (the allocations hand the planes out at 256-byte boundaries)
        if (A.cam[i] < LCR_CLOUD_CAM_FRONT || A.cam[i] > LCR_CLOUD_CAM_WRIST) return -1;
        if (A.cam[i] != LCR_CLOUD_CAM_WRIST && A.var && !A.variant) return -1;
    }
    hipLaunchKernelGGL(lcr_normals_kernel, dim3((unsigned)(A.n * A.slots)), dim3(LCR_NORMALS_THREADS), 0, (hipStream_t)stream, A);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
