// lcr_heightmap.hip -- the heightmap (lcr_enable_heightmap, include/lcr.h): one kernel that turns the selected cameras' segmentation, depth and colour planes into an
// orthographic top-down map per env -- the height of the highest surface above every cell of a fixed box of the world frame and, with rgb, its colour -- behind the frame
// kernels on their stream.  A unit of its own: a handle without a map launches nothing of this file.  What it has in common with the cloud's and the grid's kernels is in
// lcr_cloud_dev.h, once.
//
// The mapping is the voxel grid's (a workgroup of four waves is ONE env; any n works, no workgroup spans envs):
//   cameras   the thread that writes the poses does so first and every thread waits for it: the statement list of the cloud kernels (lcr_obs_cameras.inc.h), the wrist pose from the link chain included.
//   scan      thread t of round r takes the 16-pixel GROUP g = 256 r + t of the env's slots x H W / 16 groups (camera slot major).  Its 16 segmentation bytes are one 16-byte
//             load; a group with at least one candidate by id loads its 16 depth floats (four 16-byte loads), forms the point of every pixel by the chain the header pins
//             (pinned_point), the cell of the point along x and y (cell_axis) and the height word along z (height_word).  One or four
//             rounds are in flight (ROUNDS): their segmentation loads are issued before any byte is tested, their depth loads before any point is formed.  A candidate inside
//             the box takes ONE atomicMax of its 64-bit key -- height word high, 0xFFFFFFFF - global pixel index low -- on its cell's key in LDS, a single ds_max_u64: an
//             order-independent maximum, so the map does not depend on the order lanes arrive in -- and is counted.
//   output    behind a barrier each thread takes four cells along x: two 16-byte LDS reads; the four high words as 16 B of float32 heights; the colour bytes gathered through
//             0xFFFFFFFF - low word; those four differences themselves as `source` (an empty key, 0, gives - 1); a popcount for `filled`.
// LDS: one 8-byte key a cell.  Up to 8 192 cells are at most 64 KiB of dynamic LDS and one pass.  A larger map is made in the fewest passes over the planes, equal slabs of
// WHOLE ROWS of y of at most 8 192 cells each; the bytes are the same for any slab count.
// The point, the cell and the height are pinned to the bit (include/lcr.h).  This unit is built with the project's flags, -ffast-math among them; every rounded intermediate
// is made opaque to the optimiser (pinned_point, cell_axis: lcr_cloud_dev.h; height_word), and the fused steps are explicit fmaf calls.  Denormals are kept.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/lcr.h"
#include "lcr_heightmap.h"
#include "lcr_cloud_dev.h"   // is_candidate, count_word, store_cam, pinned_point, cell_axis, elem, wave_sum and the wrist pose: shared with the cloud kernels and the grid

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));   // 16 B: four depths of a group
typedef unsigned long long u64;

constexpr unsigned ALL = 0xFFFFFFFFu;   // a key's low word is ALL - g: never 0, since g < 2^32 - 1

// The header's height of a point: u = p - lo, one opaque float32 subtraction; inside iff u >= 0 && p <= hi (both faces belong to the box); the height word is the bit
// pattern of u with the sign bit cleared (u = - 0.0 passes the test and is the height + 0.0), which orders as the heights do
__device__ __forceinline__ bool height_word(float p, float lo, float hi, unsigned &hb) {
    float u = p - lo;
    asm("" : "+v"(u));
    hb = __float_as_uint(u) & 0x7fffffffu;
    return u >= 0.0f && p <= hi;
}

// ROUNDS: the rounds of the scan in flight, as the grid's kernel has them: four hold 16 depth registers each, one keeps the kernel small enough for five workgroups a CU
// (lcr_launch_heightmap chooses; the A/B is in profiles/heightmap.txt)
template <bool RGB, int ROUNDS>
__global__ __launch_bounds__(LCR_HEIGHTMAP_THREADS) void lcr_heightmap_kernel(const LcrHeightmap A, const unsigned ys) {
    __shared__ __attribute__((aligned(16))) float cams[3][16];   // ro, X, Y, Z, s of every slot
    __shared__ unsigned tot[2];                                  // count, filled
    extern __shared__ __attribute__((aligned(16))) u64 keys[];   // the keys of a pass

    const unsigned tid = threadIdx.x;
    const unsigned env = blockIdx.x;
    if (env >= (unsigned)A.n) return;   // (uniform; the grid is exact)
    const unsigned pixels = (unsigned)A.W * (unsigned)A.H;
    const unsigned gpc = pixels >> 4;                                  // groups per camera
    const unsigned G = gpc * (unsigned)A.slots;                        // groups of the env
    const unsigned rounds = (G + LCR_HEIGHTMAP_THREADS - 1) / LCR_HEIGHTMAP_THREADS;
    const size_t env_px = (size_t)env * pixels;
    const float hW = 0.5f * (float)A.W, hH = 0.5f * (float)A.H;        // (exact: W, H <= 512)
    const unsigned Hx = (unsigned)A.D[0], Hy = (unsigned)A.D[1];
    const size_t M = (size_t)Hx * Hy;
    const float fHx = (float)A.D[0], fHy = (float)A.D[1];

    // ---- the cameras: one thread, the statement list of the cloud kernels (the pose bits are the cloud's); the scan needs them, so every thread waits ----
    if (tid == 0) tot[0] = tot[1] = 0u;
    if (tid == LCR_HEIGHTMAP_THREADS - 64) {
#include "lcr_obs_cameras.inc.h"
    }
    __syncthreads();

    unsigned cnt = 0, fil = 0;
    constexpr int UNROLL = ROUNDS;
    for (unsigned y0 = 0; y0 < Hy; y0 += ys) {   // one pass, or one per slab of rows
        const unsigned ny = min(ys, Hy - y0), cells = Hx * ny;
        for (unsigned i = tid; i < (cells >> 1); i += LCR_HEIGHTMAP_THREADS) *(v4u *)(keys + 2u * i) = v4u{0u, 0u, 0u, 0u};   // (Hx is a multiple of 4)
        __syncthreads();

        // ---- scan: candidates by id whose cell lies in this pass take the maximum of their key ----
        for (unsigned r0 = 0; r0 < rounds; r0 += UNROLL) {
            v4u w[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                const unsigned g = (r0 + u) * LCR_HEIGHTMAP_THREADS + tid;
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
                const unsigned g = (r0 + u) * LCR_HEIGHTMAP_THREADS + tid;
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
                const unsigned g = (r0 + u) * LCR_HEIGHTMAP_THREADS + tid;
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
                    unsigned ix, iy, hb;
                    const bool inx = cell_axis(p[0], A.lo[0], A.inv[0], fHx, ix);
                    const bool iny = cell_axis(p[1], A.lo[1], A.inv[1], fHy, iy);
                    const bool inz = height_word(p[2], A.lo[2], A.hi_z, hb);
                    const unsigned ly = iy - y0;                       // (wraps below the slab: then >= ny)
                    const unsigned idx = ly * Hx + ix;
                    // (idx < cells follows from the tests; the integer tests keep the LDS address inside the pass whatever a float compare makes of a NaN)
                    if (hit && inx && iny && inz && ly < ny && ix < Hx && idx < cells) {
                        atomicMax(&keys[idx], ((u64)hb << 32) | (u64)(ALL - (g0 + (unsigned)k)));
                        cnt++;
                    }
                    if (++px == (unsigned)A.W) { px = 0; row++; }
                }
            }
        }
        __syncthreads();

        // ---- output: four cells along x a thread ----
        const unsigned quads = cells >> 2;   // (Hx is a multiple of 4)
        for (unsigned q = tid; q < quads; q += LCR_HEIGHTMAP_THREADS) {
            const v4u k01 = *(const v4u *)(keys + 4u * q), k23 = *(const v4u *)(keys + 4u * q + 2u);   // (little-endian: low word, high word)
            const unsigned low[4] = {k01.x, k01.z, k23.x, k23.z};
            const size_t c = (size_t)y0 * Hx + 4u * q;   // the quad's first cell in the env's map
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) m |= (low[j] != 0u ? 1u : 0u) << j;
            fil += __popc(m);
            const size_t e0 = (size_t)env * (RGB ? 4 : 1) * M + c;   // a multiple of 4
            *(v4u *)(A.out + e0) = v4u{k01.y, k01.w, k23.y, k23.w};   // the height words are the float32 bits; + 0.0 where empty
            if (A.source) *(v4u *)(A.source + (size_t)env * M + c) = v4u{ALL - low[0], ALL - low[1], ALL - low[2], ALL - low[3]};   // (an empty key gives - 1)
            if constexpr (RGB) {
                unsigned ch[3][4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    ch[0][j] = ch[1][j] = ch[2][j] = 0u;
                    if ((m >> j) & 1u) {
                        const unsigned gg = ALL - low[j];
                        const unsigned sl = (gg >= pixels) + (gg >= 2 * pixels), pix = gg - sl * pixels;
                        const unsigned char *frame = sl == 0 ? A.rgb[0] : sl == 1 ? A.rgb[1] : A.rgb[2];
                        const unsigned char *c3 = frame + (env_px + pix) * 3;
                        ch[0][j] = c3[0]; ch[1][j] = c3[1]; ch[2][j] = c3[2];
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; k++) *(v4f *)(A.out + e0 + (size_t)(k + 1) * M) = v4f{elem(ch[k][0]), elem(ch[k][1]), elem(ch[k][2]), elem(ch[k][3])};
            }
        }
        __syncthreads();   // (the next pass zeroes the keys again)
    }

    // ---- count and filled: a wave reduction each, the four waves added in LDS ----
    cnt = wave_sum(cnt);
    fil = wave_sum(fil);
    if ((tid & 63u) == 0) { atomicAdd(&tot[0], cnt); atomicAdd(&tot[1], fil); }
    __syncthreads();
    if (tid == 0) { A.count[env] = (int)tot[0]; A.filled[env] = (int)tot[1]; }
}

template <bool RGB>
void launch(const LcrHeightmap &A, unsigned ys, size_t lds, hipStream_t st) {
    // 160 KiB of LDS a CU: keys of more than a third of it leave room for two workgroups, which is what the registers of four rounds in flight allow as well
    const bool four = A.rounds ? A.rounds == 4 : lds + 256 > (size_t)160 * 1024 / 3;
    if (four) hipLaunchKernelGGL((lcr_heightmap_kernel<RGB, 4>), dim3((unsigned)A.n), dim3(LCR_HEIGHTMAP_THREADS), lds, st, A, ys);
    else hipLaunchKernelGGL((lcr_heightmap_kernel<RGB, 1>), dim3((unsigned)A.n), dim3(LCR_HEIGHTMAP_THREADS), lds, st, A, ys);
}

bool finite(const float *v) { unsigned b; __builtin_memcpy(&b, v, sizeof b); return (b & 0x7f800000u) != 0x7f800000u; }   // (by the bits, read as an integer: -ffast-math)

}  // namespace

int lcr_launch_heightmap(const LcrHeightmap &A, void *stream) {
    if (!A.out || !A.count || !A.filled || !A.pose || A.n <= 0 || A.slots < 1 || A.slots > 3 || A.W <= 0 || A.H <= 0 || A.W > 512 || A.H > 512) return -1;
    if (((size_t)A.W * A.H) % 16 || (A.channels != 1 && A.channels != 4) || A.ids == 0 || (A.ids & ~0x7feu)) return -1;
    if (A.rounds != 0 && A.rounds != 1 && A.rounds != 4) return -1;
    for (int k = 0; k < 3; k++)
        if (!finite(&A.lo[k])) return -1;
    if (!finite(&A.hi_z)) return -1;
    for (int k = 0; k < 2; k++)
        if (A.D[k] < 1 || A.D[k] > LCR_HEIGHTMAP_MAX_DIM || !finite(&A.inv[k]) || !(A.inv[k] > 0.f)) return -1;
    const size_t M = (size_t)A.D[0] * A.D[1];
    if (A.D[0] % 4 || M > LCR_HEIGHTMAP_MAX_CELLS) return -1;
    if ((size_t)A.out % 16 || (size_t)A.source % 16) return -1;   // the output pass stores 16 bytes at a time
    for (int i = 0; i < A.slots; i++) {
        if (!A.seg[i] || !A.depth[i] || (A.channels == 4 && !A.rgb[i])) return -1;
        if ((size_t)A.seg[i] % 16 || (size_t)A.depth[i] % 16) return -1;   // the scan loads both 16 bytes at a time (the planes' allocation hands them out at 256-byte boundaries)
        if (A.cam[i] < LCR_CLOUD_CAM_FRONT || A.cam[i] > LCR_CLOUD_CAM_WRIST) return -1;
        if (A.cam[i] == LCR_CLOUD_CAM_WRIST && !A.qpos) return -1;
        if (A.cam[i] != LCR_CLOUD_CAM_WRIST && A.var && !A.variant) return -1;
    }
    // how the keys are held: whole in dynamic LDS up to 64 KiB; beyond that in the fewest equal slabs of whole rows of at most 64 KiB a pass
    const unsigned Hx = (unsigned)A.D[0], Hy = (unsigned)A.D[1];
    unsigned ys = Hy;
    for (unsigned s = 2; Hx * ys > LCR_HEIGHTMAP_PASS_CELLS; s++) ys = (Hy + s - 1) / s;   // (Hx <= 256: ends at ys >= 32)
    const size_t lds = (size_t)Hx * ys * sizeof(u64);
    hipStream_t st = (hipStream_t)stream;
    if (A.channels == 4) launch<true>(A, ys, lds, st);
    else launch<false>(A, ys, lds, st);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
