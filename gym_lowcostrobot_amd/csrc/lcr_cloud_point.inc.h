// lcr_cloud_point.inc.h -- a statement list, included inside the body of a point-cloud kernel behind lcr_cloud_pass1.inc.h (lcr_cloud_dev.h says why it is no function).
// In scope before it: M > 0, `j` and `P` -- the point is entry j of P by the header's selection rule --, `o` (float *: x y z and, with colours, r g b go to o[0 .. 5]) and
// the macros LCR_CLOUD_SOURCE (the lvalue the source index is stored to) and LCR_CLOUD_COLORS (a constant expression: whether o takes colours).
// Behind it: cand, sl and pix are the candidate's number, camera slot and pixel.
        const unsigned cand = (unsigned)(((unsigned long long)(2u * j + 1u) * (unsigned long long)M) / (unsigned long long)(2u * P));   // < M
        const unsigned *cntw = (const unsigned *)cnt;
        // the segment: the last s with segpre[s] <= cand (segpre[nseg] = M > cand)
        unsigned lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const unsigned mid = (lo + hi) >> 1;
            if (segpre[mid] <= cand) lo = mid; else hi = mid;
        }
        unsigned rem = cand - segpre[lo];   // < the segment's total
        // the group inside the segment: four count bytes at a time, then the bytes of that dword
        unsigned wi = lo * (LCR_CLOUD_SEG / 4), word = cntw[wi], ws = byte_sum(word);
        for (int k = 1; k < LCR_CLOUD_SEG / 4 && rem >= ws; k++) { rem -= ws; word = cntw[++wi]; ws = byte_sum(word); }
        unsigned g = wi * 4;
        for (int k = 0; k < 3 && rem >= (word & 0xffu); k++) { rem -= word & 0xffu; word >>= 8; g++; }
        g = min(g, G - 1u);   // (cand < M puts the group among the env's own; the clamp keeps every address below inside the planes whatever the counts hold)
        // its rem-th candidate
        const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
        const unsigned char *plane = sl == 0 ? A.seg[0] : sl == 1 ? A.seg[1] : A.seg[2];
        const v4u w = *(const v4u *)(plane + env_px + (size_t)gi * 16);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
        unsigned b = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned hit = is_candidate(ww[k >> 2] >> (8 * (k & 3)), A.ids);
            if (hit && rem == 0) b = k;
            rem -= hit;   // (wraps below zero once the candidate is found: never 0 again within 16 steps)
        }
        const unsigned pix = gi * 16 + b;
        const unsigned row = pix / (unsigned)A.W, px = pix - row * (unsigned)A.W;
        LCR_CLOUD_SOURCE = (int)(sl * pixels + pix);
        const float *cam = cams[sl];
        const float *dplane = sl == 0 ? A.depth[0] : sl == 1 ? A.depth[1] : A.depth[2];
        const float t = dplane[env_px + pix];
        // the ray of the planes: d = sx X + sy Y - Z, sx and sy as the frame kernels form them (exact half-integers times s: one rounding each)
        const float sx = ((float)px + 0.5f - 0.5f * (float)A.W) * cam[12];
        const float sy = -((float)row + 0.5f - 0.5f * (float)A.H) * cam[12];
        const float dx = fmaf(sx, cam[3], fmaf(sy, cam[6], -cam[9]));
        const float dy = fmaf(sx, cam[4], fmaf(sy, cam[7], -cam[10]));
        const float dz = fmaf(sx, cam[5], fmaf(sy, cam[8], -cam[11]));
        o[0] = fmaf(t, dx, cam[0]);
        o[1] = fmaf(t, dy, cam[1]);
        o[2] = fmaf(t, dz, cam[2]);
        if constexpr (LCR_CLOUD_COLORS) {
            const unsigned char *frame = sl == 0 ? A.rgb[0] : sl == 1 ? A.rgb[1] : A.rgb[2];
            const unsigned char *c3 = frame + (env_px + pix) * 3;
            // the stack's float32 element: one correctly rounded multiply by the float32 constant 1 / 255
            o[3] = (float)c3[0] * (1.0f / 255.0f);
            o[4] = (float)c3[1] * (1.0f / 255.0f);
            o[5] = (float)c3[2] * (1.0f / 255.0f);
        }
