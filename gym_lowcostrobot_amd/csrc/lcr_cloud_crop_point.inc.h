// lcr_cloud_crop_point.inc.h -- a statement list, included inside the body of a point-cloud kernel with a crop box behind lcr_cloud_crop_pass1.inc.h: lcr_cloud_point.inc.h
// for candidates that are candidates by id AND inside the box (a copy of its text, for the reason lcr_cloud_crop_pass1.inc.h gives).
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
        // its rem-th candidate: the group's ids and depths again, and the inside bits by the device function pass 1 counted them with -- the arithmetic is pinned, so both
        // passes decide alike.  The point that goes out is the point that was tested
        const unsigned sl = (g >= gpc) + (g >= 2 * gpc), gi = g - sl * gpc;
        const unsigned char *plane = sl == 0 ? A.seg[0] : sl == 1 ? A.seg[1] : A.seg[2];
        const float *dplane = sl == 0 ? A.depth[0] : sl == 1 ? A.depth[1] : A.depth[2];
        const v4u w = *(const v4u *)(plane + env_px + (size_t)gi * 16);
        const v4f *d4 = (const v4f *)(dplane + env_px + (size_t)gi * 16);
        const v4f d[4] = {d4[0], d4[1], d4[2], d4[3]};
        const unsigned row0 = (gi * 16u) / (unsigned)A.W, px0 = gi * 16u - row0 * (unsigned)A.W;
        unsigned b = 0;
        float p3[3] = {0.f, 0.f, 0.f};
        (void)crop_scan<true>(w, d, A.ids, row0, px0, (unsigned)A.W, hW, hH, cams[sl], BX, rem, b, p3);
        const unsigned pix = gi * 16 + b;
        LCR_CLOUD_SOURCE = (int)(sl * pixels + pix);
        o[0] = p3[0];
        o[1] = p3[1];
        o[2] = p3[2];
        if constexpr (LCR_CLOUD_COLORS) {
            const unsigned char *frame = sl == 0 ? A.rgb[0] : sl == 1 ? A.rgb[1] : A.rgb[2];
            const unsigned char *c3 = frame + (env_px + pix) * 3;
            // the stack's float32 element: one correctly rounded multiply by the float32 constant 1 / 255
            o[3] = (float)c3[0] * (1.0f / 255.0f);
            o[4] = (float)c3[1] * (1.0f / 255.0f);
            o[5] = (float)c3[2] * (1.0f / 255.0f);
        }
