// lcr_boxes.hip -- the object boxes (lcr_enable_object_boxes, include/lcr.h): one kernel that reads every byte of the selected cameras' segmentation planes once and gives,
// per env, camera slot and object, the tight box, the pixel count, the coordinate sums and the nearest depth word of the matching pixels -- behind the frame kernels on their
// stream.  A unit of its own: a handle without boxes launches nothing of this file.
//
// The mapping (a workgroup of four waves is ONE (env, camera slot); any n works, no workgroup spans envs or slots):
//   scan      thread t of trip i takes the 16-pixel CHUNK q = 256 i + t of the plane's H W / 16 chunks: one 16-byte load.  A chunk none of whose bytes matches the union of
//             the masks is dropped there -- most of a frame is sky and floor, and a wave whose 64 chunks are all dropped branches over the rest.  A chunk of 16 EQUAL bytes,
//             which most chunks of sky and floor are, is decided by one byte.  W H is a multiple of 16, W need not be: row and column of the chunk's first pixel come from
//             one division, and a chunk that crosses a row end (W >= 16: at most one) is two SEGMENTS.
//   object    per object the chunk's matching pixels are a 16-bit word; a segment's minimum and maximum column, its count and its column sum are ctz, clz and population
//             counts of that word, no loop over pixels.  The 16 depth words are loaded (four 16-byte loads) only by lanes whose chunk has a matching pixel.
//   table     the lane then adds to the object's eight words in LDS with one atomicMin / atomicMax / atomicAdd a field.  They are INTEGER atomics: minimum, maximum and sum of
//             integers do not depend on the order they are taken in, so the record does not depend on the order lanes arrive in -- the same bytes on every run.  The table
//             is kept in COPIES copies, a lane adding to copy (lane mod COPIES), copies of a word in consecutive LDS banks: 64 lanes on ONE word take their turns one
//             after the other, on 32 words in 32 banks they do not wait for each other (profiles/object_boxes.txt has both).
//   output    behind a barrier n_objects 8 lanes fold the copies of their word -- again minima, maxima and sums of integers -- and, behind another, write the record, all
//             zero where the count is.
// Everything is integer arithmetic: nothing here depends on the floating-point flags of the build.
#include <hip/hip_runtime.h>

#include "../../include/lcr.h"
#include "lcr_boxes.h"

namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));   // 16 B: the 16 segmentation bytes of a chunk, or four of its depth words

constexpr unsigned IDS = 0x7FEu;   // the surface ids a mask may select (bits 1 .. 10)
constexpr unsigned COPIES = LCR_BOXES_COPIES;

// sum of the positions of the set bits of a 16-bit word
__device__ __forceinline__ unsigned bit_positions(unsigned s) {
    return __popc(s & 0xAAAAu) + 2u * __popc(s & 0xCCCCu) + 4u * __popc(s & 0xF0F0u) + 8u * __popc(s & 0xFF00u);
}

__global__ __launch_bounds__(LCR_BOXES_THREADS) void lcr_object_boxes_kernel(const LcrBoxes A) {
    extern __shared__ __attribute__((aligned(16))) unsigned tab[];   // [n_objects][8][COPIES]: x0 y0 x1 y1 count sum_x sum_y nearest per object, COPIES of each
    __shared__ unsigned rec[LCR_BOXES_MAX_OBJECTS * 8];                // the folded records
    const unsigned tid = threadIdx.x;
    const unsigned slots = (unsigned)A.slots, O = (unsigned)A.n_objects, W = (unsigned)A.W;
    const unsigned slot = blockIdx.x % slots, env = blockIdx.x / slots;
    const size_t pixels = (size_t)A.W * A.H;
    const unsigned chunks = (unsigned)(pixels >> 4);
    for (unsigned i = tid; i < O * 8u * COPIES; i += LCR_BOXES_THREADS) {
        const unsigned f = (i / COPIES) & 7u;
        tab[i] = (f < 2u || f == 7u) ? 0xFFFFFFFFu : 0u;   // the minima start at the top, the maxima and the sums at 0
    }
    const unsigned copy = tid % COPIES;
    unsigned any_ids = 0, any_marker = 0;
    for (unsigned o = 0; o < O; o++) { any_ids |= A.masks[o] & IDS; any_marker |= A.masks[o] & LCR_BOXES_MARKER; }
    const unsigned char *seg = A.seg[slot] + (size_t)env * pixels;
    const unsigned *depth = A.depth[slot] ? A.depth[slot] + (size_t)env * pixels : nullptr;
    __syncthreads();

    for (unsigned q = tid; q < chunks; q += LCR_BOXES_THREADS) {
        const v4u s = *(const v4u *)(seg + ((size_t)q << 4));
        // does any byte match the union of the masks?  16 equal bytes: one byte says
        const unsigned b0 = s[0] & 0xFFu;
        unsigned hit = 0;
        if (s[0] == b0 * 0x01010101u && s[1] == s[0] && s[2] == s[0] && s[3] == s[0]) {
            hit = ((any_ids >> min(b0 & 0x7Fu, 31u)) & 1u) | (any_marker ? b0 >> 7 : 0u);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const unsigned b = (s[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                hit |= ((any_ids >> min(b & 0x7Fu, 31u)) & 1u) | (any_marker ? b >> 7 : 0u);
            }
        }
        if (!hit) continue;
        // per pixel of the chunk: the id as a shift (ids of 31 and more select no bit of a mask) and the marker bit
        unsigned sh[16], marked = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const unsigned b = (s[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            sh[j] = min(b & 0x7Fu, 31u);
            marked |= (b >> 7) << j;
        }
        // the chunk's first pixel, and how many of its pixels lie in that row
        const unsigned p = q << 4, r = p / W, c0 = p - r * W, k = W - c0;
        unsigned w[16];
        if (depth) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const v4u d = *(const v4u *)(depth + p + 4 * i);
                w[4 * i] = d[0]; w[4 * i + 1] = d[1]; w[4 * i + 2] = d[2]; w[4 * i + 3] = d[3];
            }
        }
        for (unsigned o = 0; o < O; o++) {
            const unsigned m = A.masks[o], ids = m & IDS;
            unsigned pm = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) pm |= ((ids >> sh[j]) & 1u) << j;
            if (m & LCR_BOXES_MARKER) pm |= marked;
            if (!pm) continue;
            // segment a: row r from column c0; segment b: row r + 1 from column 0
            const unsigned a = k < 16u ? pm & ((1u << k) - 1u) : pm, b = k < 16u ? pm >> k : 0u;
            const unsigned na = __popc(a), nb = __popc(b);
            unsigned x0 = 0xFFFFFFFFu, x1 = 0;
            if (a) { x0 = c0 + (unsigned)__builtin_ctz(a); x1 = c0 + 32u - (unsigned)__builtin_clz(a); }
            if (b) { x0 = min(x0, (unsigned)__builtin_ctz(b)); x1 = max(x1, 32u - (unsigned)__builtin_clz(b)); }
            unsigned *t = tab + o * 8u * COPIES + copy;
            atomicMin(t + 0 * COPIES, x0);
            atomicMin(t + 1 * COPIES, a ? r : r + 1u);
            atomicMax(t + 2 * COPIES, x1);
            atomicMax(t + 3 * COPIES, b ? r + 2u : r + 1u);
            atomicAdd(t + 4 * COPIES, na + nb);
            atomicAdd(t + 5 * COPIES, c0 * na + bit_positions(a) + bit_positions(b));
            atomicAdd(t + 6 * COPIES, r * na + (r + 1u) * nb);
            if (depth) {
                unsigned near = 0xFFFFFFFFu;
#pragma unroll
                for (int j = 0; j < 16; j++) near = min(near, (pm >> j) & 1u ? w[j] : 0xFFFFFFFFu);
                atomicMin(t + 7 * COPIES, near);
            }
        }
    }
    __syncthreads();

    if (tid < O * 8u) {   // fold the copies of word tid; lane t starts at copy t, so the lanes of a wave read COPIES different banks at a time
        const unsigned f = tid & 7u;
        unsigned v = tab[tid * COPIES + copy];
        for (unsigned k = 1; k < COPIES; k++) {
            const unsigned x = tab[tid * COPIES + ((copy + k) % COPIES)];
            v = (f < 2u || f == 7u) ? min(v, x) : f < 4u ? max(v, x) : v + x;
        }
        rec[tid] = v;
    }
    __syncthreads();
    if (tid < O * 8u) {
        const unsigned count = rec[(tid & ~7u) + 4u];
        const unsigned v = count && (depth || (tid & 7u) != 7u) ? rec[tid] : 0u;   // no matching pixel: all eight zero; without the depth plane `nearest` is 0
        A.out[(size_t)blockIdx.x * (O * 8u) + tid] = (int)v;
    }
}

}  // namespace

int lcr_launch_object_boxes(const LcrBoxes &A, void *stream) {
    if (!A.out || A.n <= 0 || A.slots < 1 || A.slots > 3 || A.W < 16 || A.H < 16 || A.W > 512 || A.H > 512) return -1;
    if (((size_t)A.W * A.H) % 16 || A.n_objects < 1 || A.n_objects > LCR_BOXES_MAX_OBJECTS) return -1;
    if ((size_t)A.n * A.slots > 0x7FFFFFFFu) return -1;
    for (int o = 0; o < A.n_objects; o++)
        if (A.masks[o] == 0 || (A.masks[o] & ~(0x7FEu | LCR_BOXES_MARKER))) return -1;
    for (int i = 0; i < A.slots; i++) {
        if (!A.seg[i] || (size_t)A.seg[i] % 16 || (size_t)A.depth[i] % 16) return -1;   // the scan loads both 16 bytes at a time (the planes' allocation hands them out at 256-byte boundaries)
        if (!A.depth[i] != !A.depth[0]) return -1;                                      // the depth words of every slot, or of none
    }
    const size_t lds = (size_t)A.n_objects * 8 * LCR_BOXES_COPIES * sizeof(unsigned);   // 1 KiB an object: 16 KiB at most
    hipLaunchKernelGGL(lcr_object_boxes_kernel, dim3((unsigned)(A.n * A.slots)), dim3(LCR_BOXES_THREADS), lds, (hipStream_t)stream, A);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
