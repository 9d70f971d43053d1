// lcr_voxel.h -- the voxel grid (lcr_enable_voxel_grid, include/lcr.h): the arguments of its kernel and its launcher (lcr_voxel.hip).
// A header of its own, as lcr_cloud.h is: lcr_device.h, LcrCloud and every kernel that knows nothing of the grid stay as they are.
#ifndef LCR_VOXEL_H
#define LCR_VOXEL_H
#include <stddef.h>

#include "../../include/lcr.h"   // LCR_VOXEL_MAX_CELLS
#include "lcr_cloud.h"           // LCR_CLOUD_CAM_*: a slot's pose comes from where the cloud's does

#define LCR_VOXEL_THREADS 256          // a workgroup: one env, four waves
#define LCR_VOXEL_SMALL_CELLS 16384    // V a workgroup holds in 64 KiB of LDS, one word a voxel

enum { LCR_VOXEL_LDS_AUTO = 0, LCR_VOXEL_LDS_BIG = 1, LCR_VOXEL_LDS_SLAB = 2 };

struct LcrVoxel {
    // per camera slot (the selected cameras in the order front, top, wrist); [i >= slots] unused
    const unsigned char *seg[3];   // [n][pixels]
    const float *depth[3];         // [n][pixels]
    const unsigned char *rgb[3];   // [n][pixels][3]
    int cam[3];                    // LCR_CLOUD_CAM_*: where the slot's pose comes from
    int slots, n, W, H;            // pixels = W * H, a multiple of 16
    unsigned ids;                  // bit i: surface id i is a candidate (bits 1 .. 10)
    float lo[3], inv[3];           // the box's lower corner and the reported cells per metre, x y z
    int D[3];                      // Dx (a multiple of 4), Dy, Dz: each 1 .. 64, V = Dx Dy Dz <= LCR_VOXEL_MAX_CELLS
    int channels;                  // 1: occupancy; 4: occupancy, r, g, b
    int f32;                       // 0: uint8 elements; 1: float32 by the stack's rule
    int lds;                       // LCR_VOXEL_LDS_*: how a grid of more than LCR_VOXEL_SMALL_CELLS voxels is held (AUTO: the launcher's choice)
    void *out;                     // [n][channels][Dz][Dy][Dx]
    int *source;                   // [n][Dz][Dy][Dx], or null
    int *count;                    // [n]: candidates inside the grid
    int *occupied;                 // [n]: occupied voxels
    float *pose;                   // [slots][13][n]: ro, X, Y, Z, s
    // the cameras, as LcrCloud has them
    LcrCam front, top;
    const LcrLookVar *var;         // [K] or null
    const int *variant;            // [n] (with var)
    LcrWristMount mount;
    const float *qpos;             // [nq][n]: the pose snapshot the frames were drawn from
};

// 0, or the hipError_t of the launch; -1: arguments the kernel is not built for (nothing is launched)
int lcr_launch_voxel_grid(const LcrVoxel &A, void *stream);

#endif
