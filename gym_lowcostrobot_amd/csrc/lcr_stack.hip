// lcr_stack.hip -- the observation stack (lcr_enable_obs_stack, include/lcr.h): one kernel that turns the cameras' uint8 frames [n][H][W][3] into the newest slot of the
// channels-first stack [n][K][C][H][W] (uint8 / float16 / float32) and, in the same pass, moves the older slots down (a step), leaves them (a redraw) or refills them (a reset).
//
// Purely memory-bound: per element of a frame a push reads one source byte and K - 1 elements and writes K elements.  The mapping:
//   - a workgroup is ONE wave and takes one tile of LCR_STACK_TILE = 1024 consecutive pixels of one camera of one env (the last tile of a frame holds what is left, a multiple
//     of 16 as H W is).  The operation is uniform per workgroup -- it is decided per env from the flag byte -- and any n works: no workgroup spans envs.
//   - the tile's 3072 source bytes (r g b interleaved) come in as three coalesced 16-B loads per lane and go to LDS as they are.
//   - a lane then takes GROUPS of G consecutive pixels, G = 16 / sizeof(element) = 16, 8, 4, so that a group is exactly 16 B of ONE channel plane: lane l of pass q takes group
//     64 q + l, and every global load and store of the stack is 16 B per lane, consecutive lanes consecutive 16-B vectors (H W % 16 == 0 keeps every plane of every slot 16-B
//     aligned in all three element types).
//   - the group's 3 G interleaved bytes are read back from LDS at a lane stride of 48 / 24 / 12 B (12 / 6 / 3 dwords).  As compiled: three ds_read_b128 (uint8), a ds_read2_b64
//     and a ds_read_b64 (float16), a ds_read2_b32 and a ds_read_b32 (float32) per lane and pass.  In units of the access (16-B slot, 8-B pair, dword) the stride is 3, which is
//     odd: the 16 lanes of a ds_read_b128 group or of a ds_read2_b64 access fall on 16 distinct slots / pairs (3 l mod 16), the 32 lanes of a ds_read_b64 or dword-read half on
//     32 distinct pairs / banks (3 l mod 32): conflict-free without padding or swizzle.
//     The de-interleave is byte extraction in registers.
// Terminal stacks (lcr_enable_obs_stack_terminal) are two more builds of the same kernel, chosen by the template parameter MODE (lcr_stack.h): SAVE adds K - 1 vector loads and
// stores per channel to the refill of an env the step has reset, TERMINAL gathers those vectors back beside the terminal frames.  The mapping above is unchanged in both.
// The depth channel (lcr_enable_obs_stack_planes with the depth bit) is one more template parameter, D: a camera then has four channel planes, r g b d, and slot and camera
// strides follow.  The depth plane is planar float32 already, so the G depths of a group are 64 / 32 / 16 contiguous bytes: they come straight from global memory as 4 / 2 / 1
// 16-B loads per lane, without an LDS stage, and go through the element rule of include/lcr.h in registers.  D = 0 is the kernel as it was, statement for statement.
#include <hip/hip_runtime.h>

#include "../../include/lcr.h"
#include "lcr_stack.h"

namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));   // 16 B: what every global load and store of the kernel moves per lane
typedef float v4f __attribute__((ext_vector_type(4)));      // 16 B: four depths

// byte k of the words w[] a lane has read from LDS (k is a compile-time constant wherever this is called: the loops around it are unrolled)
__device__ __forceinline__ unsigned byte_of(const unsigned *w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// the element of source byte x (include/lcr.h): float32 is ONE correctly rounded multiply by the float32 constant 1 / 255 -- not a division --, float16 that value rounded to
// nearest even.  -ffast-math has nothing to reassociate in a conversion followed by one multiply.
__device__ __forceinline__ unsigned f32_bits(unsigned x) { return __float_as_uint((float)x * (1.0f / 255.0f)); }
__device__ __forceinline__ unsigned f16_bits(unsigned x) {
    const _Float16 h = (_Float16)((float)x * (1.0f / 255.0f));   // (fptrunc: v_cvt_f16_f32, round to nearest even; every value but 0 is a normal float16)
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

// the 16 B of channel c made of the G pixels whose 3 G interleaved bytes are w[]
template <int DT>
__device__ __forceinline__ v4u channel_vec(const unsigned *w, int c) {
    unsigned o[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        if constexpr (DT == LCR_STACK_UINT8)
            o[m] = byte_of(w, 3 * (4 * m) + c) | (byte_of(w, 3 * (4 * m + 1) + c) << 8) | (byte_of(w, 3 * (4 * m + 2) + c) << 16) | (byte_of(w, 3 * (4 * m + 3) + c) << 24);
        else if constexpr (DT == LCR_STACK_FLOAT16)
            o[m] = f16_bits(byte_of(w, 3 * (2 * m) + c)) | (f16_bits(byte_of(w, 3 * (2 * m + 1) + c)) << 16);
        else
            o[m] = f32_bits(byte_of(w, 3 * m + c));
    }
    return v4u{o[0], o[1], o[2], o[3]};
}

// The element of depth d (include/lcr.h), to the bit: float32 is ONE rounded multiply by inv_far, then the clamp to 1; float16 that value rounded to nearest even; uint8 ONE
// fused multiply-add d s255 + 0.5, truncated, then the clamp to 255.  This unit is built with -ffast-math: the empty asm statements hide each rounded result from the
// optimiser, which may otherwise re-associate or contract across them (the way lcr_cloud_crop.hip pins its point), and the fused step is an explicit fmaf call.
__device__ __forceinline__ float depth_unit(float d, float inv_far) {
    float m = d * inv_far;
    asm("" : "+v"(m));
    return __builtin_fminf(m, 1.0f);
}
__device__ __forceinline__ unsigned depth_u8(float d, float s255) {
    float t = __builtin_fmaf(d, s255, 0.5f);
    asm("" : "+v"(t));
    const int i = (int)t;   // (v_cvt_i32_f32: toward zero; d >= 0, so t >= 0.5)
    return (unsigned)(i < 255 ? i : 255);
}
__device__ __forceinline__ unsigned depth_f16(float d, float inv_far) {
    const _Float16 h = (_Float16)depth_unit(d, inv_far);
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

// the 16 B of the depth channel made of the G pixels whose depths lie at d (G / 4 aligned 16-B vectors)
template <int DT>
__device__ __forceinline__ v4u depth_vec(const v4f *d, float inv_far, float s255) {
    unsigned o[4];
    if constexpr (DT == LCR_STACK_UINT8) {
        v4f x[4];
#pragma unroll
        for (int m = 0; m < 4; m++) x[m] = d[m];
#pragma unroll
        for (int m = 0; m < 4; m++) o[m] = depth_u8(x[m][0], s255) | (depth_u8(x[m][1], s255) << 8) | (depth_u8(x[m][2], s255) << 16) | (depth_u8(x[m][3], s255) << 24);
    } else if constexpr (DT == LCR_STACK_FLOAT16) {
        const v4f x0 = d[0], x1 = d[1];
        o[0] = depth_f16(x0[0], inv_far) | (depth_f16(x0[1], inv_far) << 16);
        o[1] = depth_f16(x0[2], inv_far) | (depth_f16(x0[3], inv_far) << 16);
        o[2] = depth_f16(x1[0], inv_far) | (depth_f16(x1[1], inv_far) << 16);
        o[3] = depth_f16(x1[2], inv_far) | (depth_f16(x1[3], inv_far) << 16);
    } else {
        const v4f x0 = d[0];
#pragma unroll
        for (int m = 0; m < 4; m++) o[m] = __float_as_uint(depth_unit(x0[m], inv_far));
    }
    return v4u{o[0], o[1], o[2], o[3]};
}

// MODE (lcr_stack.h): LCR_STACK_MODE_PLAIN is the kernel as it has always been.  LCR_STACK_MODE_SAVE is what lcr_step launches on a handle that keeps terminal stacks: an env
// whose flag byte is set first copies its slots 1 .. K - 1 to A.history[env] and is then refilled.  LCR_STACK_MODE_TERMINAL assembles terminal stacks over a view of
// A.n listed envs: slots 0 .. K - 2 come from A.history[A.ids[env]], slot K - 1 from the view's (terminal) frames; the live stack is not touched.
// D: 1 adds the depth channel behind r g b of every camera (A.depth, A.inv_far, A.s255; CPC = 4 channel planes per camera), 0 is the colour stack.
template <int DT, int K, int MODE, int D>
__global__ __launch_bounds__(64) void lcr_obs_stack_kernel(const LcrStack A, const unsigned tiles) {
    constexpr int G = DT == LCR_STACK_UINT8 ? 16 : DT == LCR_STACK_FLOAT16 ? 8 : 4;   // pixels of one channel in 16 B
    constexpr int PASSES = LCR_STACK_TILE / (64 * G);
    constexpr int NW = 3 * G / 4;                                                     // dwords of a group's interleaved bytes
    constexpr int CPC = 3 + D;                                                        // channel planes per camera
    __shared__ v4u stage[3 * LCR_STACK_TILE / 16];

    const unsigned lane = threadIdx.x;
    const unsigned tile = blockIdx.x % tiles, ec = blockIdx.x / tiles, cam = ec % (unsigned)A.ncam, env = ec / (unsigned)A.ncam;
    if (env >= (unsigned)A.n) return;   // (uniform; the grid is exact)
    const unsigned np = min((unsigned)LCR_STACK_TILE, (unsigned)A.pixels - tile * LCR_STACK_TILE);   // pixels of this tile, a multiple of 16

    // in: 3 np bytes = 3 np / 16 vectors, lane l takes vectors l, 64 + l, 128 + l
    const unsigned char *frames = cam == 0 ? A.src[0] : cam == 1 ? A.src[1] : A.src[2];
    const v4u *src = (const v4u *)(frames + ((size_t)env * (size_t)A.pixels + (size_t)tile * LCR_STACK_TILE) * 3);
    const unsigned nvec = np * 3 / 16;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const unsigned v = i * 64 + lane;
        if (v < nvec) stage[v] = src[v];
    }
    __syncthreads();

    int op = A.op;
    if (A.flags && A.flags[env]) op = LCR_STACK_REFILL;

    const size_t pv = (size_t)(A.pixels / G);       // a channel plane, in 16-B vectors
    const size_t sv = pv * CPC * (size_t)A.ncam;    // a slot
    v4u *const tile0 = (v4u *)A.dst + (size_t)env * K * sv + (size_t)cam * CPC * pv + (size_t)tile * (LCR_STACK_TILE / G);
    const unsigned *words = (const unsigned *)stage;
    const float *dtile = nullptr;   // D: the tile's depths, [np] float32
    if constexpr (D) dtile = (cam == 0 ? A.depth[0] : cam == 1 ? A.depth[1] : A.depth[2]) + (size_t)env * (size_t)A.pixels + (size_t)tile * LCR_STACK_TILE;

#pragma unroll
    for (int q = 0; q < PASSES; q++) {
        const unsigned g = q * 64 + lane;
        if (g * G >= np) continue;   // (np is a multiple of 16 and G divides 16: a group lies wholly inside the tile or wholly outside)
        unsigned w[NW];
#pragma unroll
        for (int i = 0; i < NW; i++) w[i] = words[g * NW + i];
        v4u fresh[CPC];
#pragma unroll
        for (int c = 0; c < 3; c++) fresh[c] = channel_vec<DT>(w, c);
        if constexpr (D) fresh[3] = depth_vec<DT>((const v4f *)(dtile + g * G), A.inv_far, A.s255);

        v4u *const p = tile0 + g;   // this lane's vector of channel 0 in slot 0; channel c: + c pv, slot j: + j sv
        if constexpr (MODE == LCR_STACK_MODE_TERMINAL) {
            if constexpr (K > 1) {
                // the history of env id holds what its slots 1 .. K - 1 were, at the offsets they had: [K - 1][C][pixels]; read only, and this lane alone writes p + ...
                const v4u *const h = (const v4u *)A.history + (size_t)A.ids[env] * (K - 1) * sv + (size_t)cam * CPC * pv + (size_t)tile * (LCR_STACK_TILE / G) + g;
                v4u old[CPC][K - 1];
#pragma unroll
                for (int j = 0; j < K - 1; j++)
#pragma unroll
                    for (int c = 0; c < CPC; c++) old[c][j] = h[c * pv + (size_t)j * sv];
#pragma unroll
                for (int j = 0; j < K - 1; j++)
#pragma unroll
                    for (int c = 0; c < CPC; c++) p[c * pv + (size_t)j * sv] = old[c][j];
            }
#pragma unroll
            for (int c = 0; c < CPC; c++) p[c * pv + (size_t)(K - 1) * sv] = fresh[c];
            continue;
        }
        if constexpr (MODE == LCR_STACK_MODE_SAVE && K > 1) {
            if (op == LCR_STACK_REFILL) {
                // The episode of this env has ended: what its slots 1 .. K - 1 hold goes to the same offsets of history[env] before the refill below overwrites it.  The
                // ownership argument of the push holds here too -- these offsets of the stack and of the history are this lane's alone -- and every load comes before
                // every store, of the history and of the refill: nothing to synchronise.
                v4u *const h = (v4u *)A.history + (size_t)env * (K - 1) * sv + (size_t)cam * CPC * pv + (size_t)tile * (LCR_STACK_TILE / G) + g;
                v4u old[CPC][K - 1];
#pragma unroll
                for (int j = 0; j < K - 1; j++)
#pragma unroll
                    for (int c = 0; c < CPC; c++) old[c][j] = p[c * pv + (size_t)(j + 1) * sv];
#pragma unroll
                for (int j = 0; j < K - 1; j++)
#pragma unroll
                    for (int c = 0; c < CPC; c++) h[c * pv + (size_t)j * sv] = old[c][j];
            }
        }
        if (op == LCR_STACK_PUSH) {
            if constexpr (K > 1) {
                // In place, without a second buffer: this lane -- and no other lane of any workgroup -- owns the vectors p + c pv + j sv, j = 0 .. K - 1, the SAME offsets
                // in all K slots.  It loads every slot j + 1 before it stores any slot j (all loads below come before all stores), so a slot is read before it is overwritten,
                // and since nobody else reads or writes these offsets there is no hazard across lanes, waves or workgroups and nothing to synchronise.
                v4u old[CPC][K - 1];
#pragma unroll
                for (int j = 0; j < K - 1; j++)
#pragma unroll
                    for (int c = 0; c < CPC; c++) old[c][j] = p[c * pv + (size_t)(j + 1) * sv];
#pragma unroll
                for (int j = 0; j < K - 1; j++)
#pragma unroll
                    for (int c = 0; c < CPC; c++) p[c * pv + (size_t)j * sv] = old[c][j];
            }
        } else if (op == LCR_STACK_REFILL) {
            const unsigned keep = A.zero_fill ? 0u : ~0u;   // (zero in every element type is all bits clear)
#pragma unroll
            for (int j = 0; j < K - 1; j++)
#pragma unroll
                for (int c = 0; c < CPC; c++) p[c * pv + (size_t)j * sv] = fresh[c] & keep;
        }
        // every operation: the newest slot takes the new frames
#pragma unroll
        for (int c = 0; c < CPC; c++) p[c * pv + (size_t)(K - 1) * sv] = fresh[c];
    }
}

template <int DT, int MODE, int D>
void launch_frames_of(const LcrStack &A, unsigned tiles, unsigned blocks, hipStream_t st) {
#define LCR_STACK_CASE(k) case k: hipLaunchKernelGGL((lcr_obs_stack_kernel<DT, k, MODE, D>), dim3(blocks), dim3(64), 0, st, A, tiles); break
    switch (A.frames) {
        LCR_STACK_CASE(1); LCR_STACK_CASE(2); LCR_STACK_CASE(3); LCR_STACK_CASE(4);
        LCR_STACK_CASE(5); LCR_STACK_CASE(6); LCR_STACK_CASE(7); LCR_STACK_CASE(8);
    }
#undef LCR_STACK_CASE
}

template <int MODE, int D>
void launch_dtype_of(const LcrStack &A, unsigned tiles, unsigned blocks, hipStream_t st) {
    if (A.dtype == LCR_STACK_UINT8) launch_frames_of<LCR_STACK_UINT8, MODE, D>(A, tiles, blocks, st);
    else if (A.dtype == LCR_STACK_FLOAT16) launch_frames_of<LCR_STACK_FLOAT16, MODE, D>(A, tiles, blocks, st);
    else launch_frames_of<LCR_STACK_FLOAT32, MODE, D>(A, tiles, blocks, st);
}

template <int MODE>
void launch_mode_of(const LcrStack &A, unsigned tiles, unsigned blocks, hipStream_t st) {
    if (A.cpc == 4) launch_dtype_of<MODE, 1>(A, tiles, blocks, st);
    else launch_dtype_of<MODE, 0>(A, tiles, blocks, st);
}

}  // namespace

int lcr_launch_obs_stack(const LcrStack &A, void *stream) {
    if (!A.dst || A.n <= 0 || A.ncam < 1 || A.ncam > 3 || A.pixels <= 0 || A.pixels % 16 || A.frames < 1 || A.frames > 8) return -1;
    if (A.dtype != LCR_STACK_UINT8 && A.dtype != LCR_STACK_FLOAT16 && A.dtype != LCR_STACK_FLOAT32) return -1;
    if (A.op != LCR_STACK_PUSH && A.op != LCR_STACK_NEWEST && A.op != LCR_STACK_REFILL) return -1;
    if (A.cpc != 3 && A.cpc != 4) return -1;
    for (int i = 0; i < A.ncam; i++)
        if (!A.src[i] || (A.cpc == 4 && !A.depth[i])) return -1;
    const unsigned tiles = (unsigned)((A.pixels + LCR_STACK_TILE - 1) / LCR_STACK_TILE);
    const unsigned long long blocks = (unsigned long long)A.n * (unsigned)A.ncam * tiles;
    if (blocks > 0x7fffffffull) return -1;
    // the save needs somewhere to save to and somebody to say who was reset; the assembly the ids of the view's envs and, with older slots, their history
    if (A.mode != LCR_STACK_MODE_PLAIN && A.mode != LCR_STACK_MODE_SAVE && A.mode != LCR_STACK_MODE_TERMINAL) return -1;
    if (A.mode == LCR_STACK_MODE_SAVE && (!A.history || !A.flags || A.op != LCR_STACK_PUSH || A.frames < 2)) return -1;
    if (A.mode == LCR_STACK_MODE_TERMINAL && (!A.ids || (A.frames > 1 && !A.history))) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (A.mode == LCR_STACK_MODE_SAVE) launch_mode_of<LCR_STACK_MODE_SAVE>(A, tiles, (unsigned)blocks, st);
    else if (A.mode == LCR_STACK_MODE_TERMINAL) launch_mode_of<LCR_STACK_MODE_TERMINAL>(A, tiles, (unsigned)blocks, st);
    else launch_mode_of<LCR_STACK_MODE_PLAIN>(A, tiles, (unsigned)blocks, st);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
