// lcr_normals.h -- the surface normals (lcr_enable_normals, include/lcr.h): the arguments of their kernel and its launcher (lcr_normals.hip).
// A header of its own, as lcr_boxes.h is: lcr_device.h and every kernel that knows nothing of the normals stay as they are.
#ifndef LCR_NORMALS_H
#define LCR_NORMALS_H
#include <stddef.h>

#include "../../include/lcr.h"   // LCR_NORMALS_WORLD, LCR_NORMALS_CAMERA
#include "lcr_cloud.h"           // LCR_CLOUD_CAM_*: a slot's pose comes from where the cloud's does

#define LCR_NORMALS_THREADS 256   // a workgroup: one (env, camera slot), four waves
#define LCR_NORMALS_BOXES 9       // the opaque boxes: surface ids 2 .. 10
#define LCR_NORMALS_BOX_FLOATS 15 // centre, X, Y, Z, half-extents

struct LcrNormals {
    // per camera slot (the selected cameras in the order front, top, wrist); [i >= slots] unused
    const unsigned char *seg[3];   // [n][H][W]
    const float *depth[3];         // [n][H][W]
    unsigned *out[3];              // [n][H][W]: int8 x 4 packed, nx | ny << 8 | nz << 16 | w << 24
    int cam[3];                    // LCR_CLOUD_CAM_*: where the slot's pose comes from
    int slots, n, W, H;            // W and H multiples of 4
    int frame;                     // LCR_NORMALS_WORLD | LCR_NORMALS_CAMERA
    int ncube;                     // 1 | 2: the boxes of a second cube the task does not have are zeros
    float *boxes;                  // [9][15][n]: centre, X, Y, Z, half-extents as the kernel used them
    float *pose;                   // [slots][13][n]: ro, X, Y, Z, s
    // the cameras, as LcrCloud has them
    LcrCam front, top;
    const LcrLookVar *var;         // [K] or null
    const int *variant;            // [n] (with var)
    LcrWristMount mount;
    const float *qpos;             // [nq][n]: the pose snapshot the frames were drawn from
};

// 0, or the hipError_t of the launch; -1: arguments the kernel is not built for (nothing is launched)
int lcr_launch_normals(const LcrNormals &A, void *stream);

#endif
