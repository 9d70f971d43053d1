// lcr_flow.h -- the motion vectors (lcr_enable_motion_vectors, include/lcr.h): the arguments of their kernel and its launcher (lcr_flow.hip).
// A header of its own, as lcr_normals.h is: lcr_device.h and every kernel that knows nothing of the motion vectors stay as they are.
#ifndef LCR_FLOW_H
#define LCR_FLOW_H
#include <stddef.h>

#include "../../include/lcr.h"
#include "lcr_cloud.h"           // LCR_CLOUD_CAM_*: a slot's pose comes from where the cloud's does

#define LCR_FLOW_THREADS 256   // a workgroup: one (env, camera slot), four waves
#define LCR_FLOW_BOXES 9       // the opaque boxes: surface ids 2 .. 10
#define LCR_FLOW_BOX_FLOATS 15 // centre, X, Y, Z, half-extents

struct LcrFlow {
    // per camera slot (the selected cameras in the order front, top, wrist); [i >= slots] unused
    const unsigned char *seg[3];   // [n][H][W]
    const float *depth[3];         // [n][H][W]
    unsigned *out[3];              // [n][H][W]: float16 x 2 packed, fx | fy << 16
    int cam[3];                    // LCR_CLOUD_CAM_*: where the slot's pose comes from
    int slots, n, W, H;            // W and H multiples of 4
    int ncube;                     // 1 | 2: the boxes of a second cube the task does not have are zeros
    int restart;                   // 1: no history is read, "before" becomes a copy of "now", every plane is zero and valid is 0
    float *boxes;                  // [2][9][15][n]: [0] now, [1] before -- centre, X, Y, Z, half-extents as the kernel used them
    float *pose;                   // [2][slots][13][n]: ro, X, Y, Z, s
    unsigned char *valid;          // [n]
    const unsigned char *flags;    // [n]: did_reset of the step that is measured (unused on a restart)
    // the cameras, as LcrCloud has them
    LcrCam front, top;
    const LcrLookVar *var;         // [K] or null
    const int *variant;            // [n] (with var)
    LcrWristMount mount;
    const float *qpos;             // [nq][n]: the pose snapshot the frames were drawn from
};

// 0, or the hipError_t of the launch; -1: arguments the kernel is not built for (nothing is launched)
int lcr_launch_flow(const LcrFlow &A, void *stream);

#endif
