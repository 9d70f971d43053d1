// lcr_cloud_fps_loop.inc.h -- a statement list, included inside the body of a farthest-point kernel behind its pool (lcr_cloud_dev.h says why it is no function): the greedy
// loop and the colours, to the end of the kernel.
// In scope before it: M > 0 and everything lcr_cloud_pass1.inc.h leaves, the LDS array `slot` [2][4][8], K, Q, C, E, out, src, and the pool in registers -- x, y, z, key and
// source [EMAX], an entry beyond Q with key KEY_CHOSEN.
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
