// lcr_voxel.hip -- the voxel grid (lcr_enable_voxel_grid, include/lcr.h): one kernel that turns the selected cameras' segmentation, depth and colour planes into a dense
// occupancy (and colour) grid over a fixed box of the world frame per env, behind the frame kernels on their stream.  A unit of its own: a handle without a grid launches
// nothing of this file.  What it has in common with the cloud's kernels is in lcr_cloud_dev.h, once.
//
// The mapping is the cloud's (a workgroup of four waves is ONE env; any n works, no workgroup spans envs):
//   cameras   the thread that writes the poses does so first and every thread waits for it: the statement list of the cloud kernels (lcr_obs_cameras.inc.h), the wrist pose from the link chain included.
//   scan      thread t of round r takes the 16-pixel GROUP g = 256 r + t of the env's slots x H W / 16 groups (camera slot major).  Its 16 segmentation bytes are one 16-byte
//             load; a group with at least one candidate by id loads its 16 depth floats (four 16-byte loads), forms the point of every pixel by the chain the header pins
//             (pinned_point) and the voxel of the point (cell_axis).  One or four rounds are in flight (ROUNDS): their segmentation loads are issued before any
//             byte is tested, their depth loads before any point is formed.  A candidate inside the grid takes atomicMin(global pixel index) on its voxel's word in LDS --
//             an order-independent minimum: the grid does not depend on the order lanes arrive in -- and is counted.
//   output    behind a barrier each thread takes four voxels along x: one 16-byte LDS read; a dword of uint8 occupancy or 16 B of float32; the colour bytes gathered through
//             the source index; the four words themselves as `source` (an empty word, 0xFFFFFFFF, is - 1); a popcount for `occupied`.
// LDS: one word a voxel.  V <= 16 384 is at most 64 KiB of dynamic LDS.  A larger grid is made in passes over the planes, one z-slab of at most 16 384 voxels each (the
// default), or held whole in a build with 128 KiB of static LDS, one workgroup a CU (LCR_VOXEL_LDS=slab|big; the A/B is in profiles/voxel_grid.txt).
// The point and the voxel are pinned to the bit (include/lcr.h).  This unit is built with the project's flags, -ffast-math among them; every rounded intermediate is made
// opaque to the optimiser (pinned_point, cell_axis: lcr_cloud_dev.h), and the fused steps are explicit fmaf calls.  Denormals are kept.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lcr.h"
#include "lcr_voxel.h"
#include "lcr_cloud_dev.h"   // is_candidate, count_word, store_cam, pinned_point, cell_axis, elem, wave_sum and the wrist pose: shared with the cloud kernels and the map

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));   // 16 B: four depths of a group, four float32 elements of the grid

constexpr unsigned EMPTY = 0xFFFFFFFFu;

// ROUNDS: the rounds of the scan in flight.  Four hold 16 depth registers each (185 VGPRs: two workgroups a CU), one keeps the kernel at 81 (five): four where the grid's words
// leave room for two workgroups anyway, one where they leave room for more (lcr_launch_voxel_grid; the A/B is in profiles/voxel_grid.txt)
template <bool F32, bool RGB, bool BIG, int ROUNDS>
__global__ __launch_bounds__(LCR_VOXEL_THREADS) void lcr_voxel_grid_kernel(const LcrVoxel A, const unsigned zs) {
    __shared__ __attribute__((aligned(16))) float cams[3][16];                          // ro, X, Y, Z, s of every slot
    __shared__ unsigned tot[2];                                                         // count, occupied
    __shared__ __attribute__((aligned(16))) unsigned whole[BIG ? LCR_VOXEL_MAX_CELLS : 4];   // the 128 KiB build: the grid's words, static
    extern __shared__ __attribute__((aligned(16))) unsigned slab[];                     // every other build: the words of a pass, dynamic
    unsigned *const vox = BIG ? whole : slab;

    const unsigned tid = threadIdx.x;
    const unsigned env = blockIdx.x;
    if (env >= (unsigned)A.n) return;   // (uniform; the grid is exact)
    const unsigned pixels = (unsigned)A.W * (unsigned)A.H;
    const unsigned gpc = pixels >> 4;                                  // groups per camera
    const unsigned G = gpc * (unsigned)A.slots;                        // groups of the env
    const unsigned rounds = (G + LCR_VOXEL_THREADS - 1) / LCR_VOXEL_THREADS;
    const size_t env_px = (size_t)env * pixels;
    const float hW = 0.5f * (float)A.W, hH = 0.5f * (float)A.H;        // (exact: W, H <= 512)
    const unsigned Dx = (unsigned)A.D[0], Dy = (unsigned)A.D[1], Dz = (unsigned)A.D[2], DxDy = Dx * Dy;
    const size_t V = (size_t)DxDy * Dz;
    const float fDx = (float)A.D[0], fDy = (float)A.D[1], fDz = (float)A.D[2];

    // ---- the cameras: one thread, the statement list of the cloud kernels (the pose bits are the cloud's); the scan needs them, so every thread waits ----
    if (tid == 0) tot[0] = tot[1] = 0u;
    if (tid == LCR_VOXEL_THREADS - 64) {
#include "lcr_obs_cameras.inc.h"
    }
    __syncthreads();

    unsigned cnt = 0, occ = 0;
    constexpr int UNROLL = ROUNDS;
    for (unsigned z0 = 0; z0 < Dz; z0 += zs) {   // one pass, or one per z-slab
        const unsigned nz = min(zs, Dz - z0), words = DxDy * nz;
        for (unsigned i = tid; i < (words >> 2); i += LCR_VOXEL_THREADS) *(v4u *)(vox + 4u * i) = v4u{EMPTY, EMPTY, EMPTY, EMPTY};   // (Dx is a multiple of 4)
        __syncthreads();

        // ---- scan: candidates by id whose voxel lies in this pass take the minimum of their global pixel index ----
        for (unsigned r0 = 0; r0 < rounds; r0 += UNROLL) {
            v4u w[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const unsigned g = (r0 + u) * LCR_VOXEL_THREADS + tid;
                w[u] = v4u{0u, 0u, 0u, 0u};
                if (g < G) {
                    const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
                    const unsigned char *plane = sl == 0 ? A.seg[0] : sl == 1 ? A.seg[1] : A.seg[2];
                    w[u] = *(const v4u *)(plane + env_px + (size_t)gi * 16);
                }
            }
            // the depths of the groups that hold a candidate by id, 64 B each: the loads of all UNROLL rounds are issued before the first is used.  (A group beyond the
            // env's last has zero bytes: no candidate, no load)
            v4f d[UNROLL][4];
            unsigned byid[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const unsigned g = (r0 + u) * LCR_VOXEL_THREADS + tid;
                byid[u] = count_word(w[u].x, A.ids) + count_word(w[u].y, A.ids) + count_word(w[u].z, A.ids) + count_word(w[u].w, A.ids);
#pragma unroll
                for (int q = 0; q < 4; q++) d[u][q] = v4f{0.f, 0.f, 0.f, 0.f};
                if (byid[u]) {   // (then g < G)
                    const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
                    const float *dplane = sl == 0 ? A.depth[0] : sl == 1 ? A.depth[1] : A.depth[2];
                    const v4f *d4 = (const v4f *)(dplane + env_px + (size_t)gi * 16);
#pragma unroll
                    for (int q = 0; q < 4; q++) d[u][q] = d4[q];
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                if (!byid[u]) continue;
                const unsigned g = (r0 + u) * LCR_VOXEL_THREADS + tid;
                const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
                unsigned row = (gi * 16u) / (unsigned)A.W, px = gi * 16u - row * (unsigned)A.W;   // (one division a group; W is a multiple of 4, not of 16: a group may straddle rows)
                const unsigned g0 = sl * pixels + gi * 16u;                                        // the global pixel index of the group's first pixel
                float cam[13];
#pragma unroll
                for (int k = 0; k < 13; k++) cam[k] = cams[sl][k];
                const unsigned ww[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const unsigned hit = is_candidate(ww[k >> 2] >> (8 * (k & 3)), A.ids);
                    float p[3];
                    pinned_point(px, row, hW, hH, d[u][k >> 2][k & 3], cam, p);
                    unsigned ix, iy, iz;
                    const bool inx = cell_axis(p[0], A.lo[0], A.inv[0], fDx, ix);
                    const bool iny = cell_axis(p[1], A.lo[1], A.inv[1], fDy, iy);
                    const bool inz = cell_axis(p[2], A.lo[2], A.inv[2], fDz, iz);
                    const unsigned lz = iz - z0;                       // (wraps below the slab: then >= nz)
                    const unsigned idx = lz * DxDy + iy * Dx + ix;
                    // (idx < words follows from the three tests; the integer test keeps the LDS address inside the pass whatever a float compare makes of a NaN)
                    if (hit && inx && iny && inz && lz < nz && idx < words) {
                        atomicMin(&vox[idx], g0 + (unsigned)k);
                        cnt++;
                    }
                    if (++px == (unsigned)A.W) { px = 0; row++; }
                }
            }
        }
        __syncthreads();

        // ---- output: four voxels along x a thread ----
        const unsigned quads = words >> 2;   // (Dx is a multiple of 4)
        constexpr int C = RGB ? 4 : 1;
        for (unsigned q = tid; q < quads; q += LCR_VOXEL_THREADS) {
            const v4u g4 = *(const v4u *)(vox + 4u * q);
            const unsigned gg[4] = {g4.x, g4.y, g4.z, g4.w};
            const size_t v = (size_t)z0 * DxDy + 4u * q;   // the quad's first voxel in the env's grid
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) m |= (gg[j] != EMPTY ? 1u : 0u) << j;
            occ += __popc(m);
            if (A.source) *(v4u *)(A.source + (size_t)env * V + v) = g4;   // (an empty word is - 1)
            unsigned ch[C][4];   // the elements' source bytes: occupancy 255 or 0, then r, g, b of the source pixel
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool on = (m >> j) & 1u;
                ch[0][j] = on ? 255u : 0u;
                if constexpr (RGB) {
                    ch[1][j] = ch[2][j] = ch[3][j] = 0u;
                    if (on) {
                        const unsigned sl = (gg[j] >= pixels) + (gg[j] >= 2 * pixels), pix = gg[j] - sl * pixels;
                        const unsigned char *frame = sl == 0 ? A.rgb[0] : sl == 1 ? A.rgb[1] : A.rgb[2];
                        const unsigned char *c3 = frame + (env_px + pix) * 3;
                        ch[1][j] = c3[0]; ch[2][j] = c3[1]; ch[3][j] = c3[2];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < C; c++) {
                const size_t e = ((size_t)env * C + c) * V + v;   // a multiple of 4
                if constexpr (F32) *(v4f *)((float *)A.out + e) = v4f{elem(ch[c][0]), elem(ch[c][1]), elem(ch[c][2]), elem(ch[c][3])};
                else *(unsigned *)((unsigned char *)A.out + e) = ch[c][0] | ch[c][1] << 8 | ch[c][2] << 16 | ch[c][3] << 24;
            }
        }
        __syncthreads();   // (the next pass fills the words again)
    }

    // ---- count and occupied: a wave reduction each, the four waves added in LDS ----
    cnt = wave_sum(cnt);
    occ = wave_sum(occ);
    if ((tid & 63u) == 0) { atomicAdd(&tot[0], cnt); atomicAdd(&tot[1], occ); }
    __syncthreads();
    if (tid == 0) { A.count[env] = (int)tot[0]; A.occupied[env] = (int)tot[1]; }
}

template <bool F32, bool RGB, bool BIG>
void launch(const LcrVoxel &A, unsigned zs, size_t lds, hipStream_t st) {
    // 160 KiB of LDS a CU: words of more than a third of it leave room for two workgroups, which is what the registers of four rounds in flight allow as well
    const bool two = BIG || lds + 256 > (size_t)160 * 1024 / 3;
    if (two) hipLaunchKernelGGL((lcr_voxel_grid_kernel<F32, RGB, BIG, 4>), dim3((unsigned)A.n), dim3(LCR_VOXEL_THREADS), lds, st, A, zs);
    else hipLaunchKernelGGL((lcr_voxel_grid_kernel<F32, RGB, false, 1>), dim3((unsigned)A.n), dim3(LCR_VOXEL_THREADS), lds, st, A, zs);
}

bool finite(const float *v) { unsigned b; __builtin_memcpy(&b, v, sizeof b); return (b & 0x7f800000u) != 0x7f800000u; }   // (by the bits, read as an integer: -ffast-math)

}  // namespace

int lcr_launch_voxel_grid(const LcrVoxel &A, void *stream) {
    if (!A.out || !A.count || !A.occupied || !A.pose || A.n <= 0 || A.slots < 1 || A.slots > 3 || A.W <= 0 || A.H <= 0 || A.W > 512 || A.H > 512) return -1;
    if (((size_t)A.W * A.H) % 16 || (A.channels != 1 && A.channels != 4) || A.ids == 0 || (A.ids & ~0x7feu)) return -1;
    for (int k = 0; k < 3; k++)
        if (A.D[k] < 1 || A.D[k] > 64 || !finite(&A.lo[k]) || !finite(&A.inv[k]) || !(A.inv[k] > 0.f)) return -1;
    const size_t V = (size_t)A.D[0] * A.D[1] * A.D[2];
    if (A.D[0] % 4 || V > LCR_VOXEL_MAX_CELLS) return -1;
    if ((size_t)A.out % 16 || (size_t)A.source % 16) return -1;   // the output pass stores 16 bytes at a time
    for (int i = 0; i < A.slots; i++) {
        if (!A.seg[i] || !A.depth[i] || (A.channels == 4 && !A.rgb[i])) return -1;
        if ((size_t)A.seg[i] % 16 || (size_t)A.depth[i] % 16) return -1;   // the scan loads both 16 bytes at a time (the planes' allocation hands them out at 256-byte boundaries)
        if (A.cam[i] < LCR_CLOUD_CAM_FRONT || A.cam[i] > LCR_CLOUD_CAM_WRIST) return -1;
        if (A.cam[i] == LCR_CLOUD_CAM_WRIST && !A.qpos) return -1;
        if (A.cam[i] != LCR_CLOUD_CAM_WRIST && A.var && !A.variant) return -1;
    }
    // how the grid's words are held: whole in dynamic LDS up to 64 KiB; beyond that whole in the 128 KiB build, or a z-slab of at most 64 KiB a pass
    const unsigned DxDy = (unsigned)(A.D[0] * A.D[1]);
    bool big = false;
    unsigned zs = (unsigned)A.D[2];
    if (V > LCR_VOXEL_SMALL_CELLS) {
        if (A.lds == LCR_VOXEL_LDS_BIG) {
            big = true;
        } else {   // (the default: measured faster than the 128 KiB build at 84 x 84 and at 240 x 320, profiles/voxel_grid.txt)
            for (unsigned s = 2; DxDy * zs > LCR_VOXEL_SMALL_CELLS; s++) zs = ((unsigned)A.D[2] + s - 1) / s;   // (Dx Dy <= 4096: ends at zs >= 4)
        }
    }
    const size_t lds = big ? 0 : (size_t)DxDy * zs * sizeof(unsigned);
    hipStream_t st = (hipStream_t)stream;
    const int which = (A.f32 ? 4 : 0) | (A.channels == 4 ? 2 : 0) | (big ? 1 : 0);
    switch (which) {
    case 0: launch<false, false, false>(A, zs, lds, st); break;
    case 1: launch<false, false, true>(A, zs, lds, st); break;
    case 2: launch<false, true, false>(A, zs, lds, st); break;
    case 3: launch<false, true, true>(A, zs, lds, st); break;
    case 4: launch<true, false, false>(A, zs, lds, st); break;
    case 5: launch<true, false, true>(A, zs, lds, st); break;
    case 6: launch<true, true, false>(A, zs, lds, st); break;
    default: launch<true, true, true>(A, zs, lds, st); break;
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
