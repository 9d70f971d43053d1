// lcr_stack.h -- the observation stack (lcr_enable_obs_stack, include/lcr.h): the arguments of its kernel and its launcher (lcr_stack.hip).
// A header of its own: lcr_device.h and every kernel that knows nothing of the stack stay as they are.
#ifndef LCR_STACK_H
#define LCR_STACK_H
#include <stddef.h>

// what the kernel does with an env.  An env whose flag byte is set is always refilled; `op` is what happens to the others (and to all without flags).
enum { LCR_STACK_PUSH = 0, LCR_STACK_NEWEST = 1, LCR_STACK_REFILL = 2 };

// which build of the kernel runs (a template parameter: the plain build is the kernel of a handle that keeps no terminal stacks, with nothing added to it).
//   SAVE      lcr_step on a handle that keeps terminal stacks (op PUSH, flags = did_reset or its snapshot): an env whose flag is set first copies its slots 1 .. K - 1 to
//             history[env], then is refilled.
//   TERMINAL  the assembly of lcr_obs_stack_terminal over a view of n listed envs: dst[e] takes slots 0 .. K - 2 from history[ids[e]] and slot K - 1 from src; flags and op
//             are not looked at.
enum { LCR_STACK_MODE_PLAIN = 0, LCR_STACK_MODE_SAVE = 1, LCR_STACK_MODE_TERMINAL = 2 };

#define LCR_STACK_TILE 1024   // pixels of one camera of one env a wave takes (the last tile of a frame may hold fewer, a multiple of 16)

struct LcrStack {
    const unsigned char *src[3];   // the selected cameras' frames in channel order, [n][pixels][3] each; src[i >= ncam] unused
    void *dst;                     // [n][frames][cpc ncam][pixels] of the element type
    const unsigned char *flags;    // [n] or null
    int n, ncam, pixels;           // pixels = img_h * img_w, a multiple of 16
    int frames;                    // K, 1 .. 8
    int dtype;                     // lcr_obs_stack_dtype
    int op;                        // LCR_STACK_*
    int zero_fill;                 // a refill writes zeros (not the new frames) to slots 0 .. K - 2
    int mode;                      // LCR_STACK_MODE_*
    void *history;                 // [N][frames - 1][3 ncam][pixels] of the element type (SAVE: written, TERMINAL: read), or null
    const int *ids;                // TERMINAL: [n] env ids of the view's envs, the rows of `history`
    // the depth channel (lcr_enable_obs_stack_planes with the depth bit): cpc = 4 channel planes per camera, r g b d -- dst and history are then [..][4 ncam][pixels] --,
    // 3 without it (nothing below is looked at, and the kernel that runs is the colour stack's)
    int cpc;
    const float *depth[3];         // the selected cameras' depth planes in channel order, [n][pixels] float32 each
    float inv_far, s255;           // (float)(1.0 / (double)depth_far), (float)(255.0 / (double)depth_far): the constants of the element rule (include/lcr.h)
};

// 0, or the hipError_t of the launch; -1: arguments the kernel is not built for (nothing is launched)
int lcr_launch_obs_stack(const LcrStack &A, void *stream);

#endif
