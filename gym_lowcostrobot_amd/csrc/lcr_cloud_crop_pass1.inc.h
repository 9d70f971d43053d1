// lcr_cloud_crop_pass1.inc.h -- a statement list, included inside the body of a point-cloud kernel with a crop box (lcr_cloud_crop.hip): lcr_cloud_pass1.inc.h with the
// cameras BEFORE pass 1 and the inside test in it.  Pass 1 and the prefix are a copy of that list's text, not a parameter of it: the kernels without a box stay
// instruction for instruction what they are (lcr_cloud_dev.h).  The cameras are the one list both include (lcr_obs_cameras.inc.h).
// In scope before it: `A` (an LcrCloud), `BX` (an LcrCloudCrop: the box), the macro LCR_CLOUD_CROP_ROUNDS (how many rounds of pass 1 are in flight), and the LDS arrays `segpre` [MAX_SEG + 4], `cams` [3][16] and `cnt` (dynamic, lcr_cloud_lds_bytes).
// It returns from the kernel for a workgroup beyond the last env; behind it, and behind a barrier: tid, lane, wave, env, pixels, gpc, G, nseg, env_px, hW, hH and M are
// defined, cams, cnt and segpre are filled (segpre[nseg] = M), and the camera poses and count[env] are written.
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned env = blockIdx.x;
    if (env >= (unsigned)A.n) return;   // (uniform; the grid is exact)
    const unsigned pixels = (unsigned)A.W * (unsigned)A.H;
    const unsigned gpc = pixels >> 4;                                  // groups per camera
    const unsigned G = gpc * (unsigned)A.slots;                        // groups of the env
    const unsigned nseg = (G + LCR_CLOUD_SEG - 1) / LCR_CLOUD_SEG;
    const unsigned rounds = (G + LCR_CLOUD_THREADS - 1) / LCR_CLOUD_THREADS;
    const size_t env_px = (size_t)env * pixels;
    const float hW = 0.5f * (float)A.W, hH = 0.5f * (float)A.H;        // (exact: W, H <= 512)

    // ---- the cameras: one thread, the statement list lcr_cloud_pass1.inc.h includes (the pose bits are those of a handle without a box); pass 1 needs them, so every
    //      thread waits here ----
    if (tid == LCR_CLOUD_THREADS - 64) {
#include "lcr_obs_cameras.inc.h"
    }
    __syncthreads();

    // ---- pass 1: candidates per group -- by id AND inside the box --, UNROLL rounds in flight; then the totals per segment ----
    constexpr int UNROLL = LCR_CLOUD_CROP_ROUNDS;
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
        // the depths of the groups that hold a candidate by id, 64 B each: the loads of all UNROLL rounds are issued before the first is used.  (A group beyond the env's
        // last has zero bytes: no candidate, no load)
        v4f d[UNROLL][4];
        unsigned byid[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const unsigned g = (r0 + u) * LCR_CLOUD_THREADS + tid;
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
            const unsigned g = (r0 + u) * LCR_CLOUD_THREADS + tid;
            unsigned c = 0;
            if (byid[u]) {
                const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
                const unsigned row = (gi * 16u) / (unsigned)A.W, px = gi * 16u - row * (unsigned)A.W;   // (one division a group; the scan steps row and px per pixel)
                unsigned b;
                float p[3];
                c = crop_scan<false>(w[u], d[u], A.ids, row, px, (unsigned)A.W, hW, hH, cams[sl], BX, 0u, b, p);
            }
            if (g < ngrp) cnt[g] = (unsigned char)c;
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
