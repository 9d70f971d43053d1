// lcr_cloud_pass1.inc.h -- a statement list, included inside the body of a point-cloud kernel (lcr_cloud_dev.h says why it is no function).
// In scope before it: `A` (an LcrCloud), and the LDS arrays `segpre` [MAX_SEG + 4], `cams` [3][16] and `cnt` (dynamic, lcr_cloud_lds_bytes).
// It returns from the kernel for a workgroup beyond the last env; behind it, and behind a barrier: tid, lane, wave, env, pixels, gpc, G, nseg, env_px and M are defined,
// cams, cnt and segpre are filled (segpre[nseg] = M), and the camera poses and count[env] are written.
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
#include "lcr_obs_cameras.inc.h"
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
