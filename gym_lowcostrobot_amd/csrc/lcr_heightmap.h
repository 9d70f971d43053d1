// lcr_heightmap.h -- the heightmap (lcr_enable_heightmap, include/lcr.h): the arguments of its kernel and its launcher (lcr_heightmap.hip).
// A header of its own, as lcr_voxel.h is: lcr_device.h, LcrCloud, LcrVoxel and every kernel that knows nothing of the map stay as they are.
#ifndef LCR_HEIGHTMAP_H
#define LCR_HEIGHTMAP_H
#include <stddef.h>

#include "../../include/lcr.h"   // LCR_HEIGHTMAP_MAX_CELLS
#include "lcr_cloud.h"           // LCR_CLOUD_CAM_*: a slot's pose comes from where the cloud's does

#define LCR_HEIGHTMAP_THREADS 256         // a workgroup: one env, four waves
#define LCR_HEIGHTMAP_PASS_CELLS 8192     // cells a workgroup holds in 64 KiB of LDS, an 8-byte key a cell

struct LcrHeightmap {
    // per camera slot (the selected cameras in the order front, top, wrist); [i >= slots] unused
    const unsigned char *seg[3];   // [n][pixels]
    const float *depth[3];         // [n][pixels]
    const unsigned char *rgb[3];   // [n][pixels][3]
    int cam[3];                    // LCR_CLOUD_CAM_*: where the slot's pose comes from
    int slots, n, W, H;            // pixels = W * H, a multiple of 16
    unsigned ids;                  // bit i: surface id i is a candidate (bits 1 .. 10)
    float lo[3], hi_z, inv[2];     // the box's lower corner, its upper face along z and the reported cells per metre along x, y
    int D[2];                      // Hx (a multiple of 4), Hy: each 1 .. 256, Hx Hy <= LCR_HEIGHTMAP_MAX_CELLS
    int channels;                  // 1: height; 4: height, r, g, b
    int rounds;                    // rounds of the scan in flight: 1, 4, or 0 for the launcher's choice
    float *out;                    // [n][channels][Hy][Hx]
    int *source;                   // [n][Hy][Hx], or null
    int *count;                    // [n]: candidates inside the box
    int *filled;                   // [n]: non-empty cells
    float *pose;                   // [slots][13][n]: ro, X, Y, Z, s
    // the cameras, as LcrCloud has them
    LcrCam front, top;
    const LcrLookVar *var;         // [K] or null
    const int *variant;            // [n] (with var)
    LcrWristMount mount;
    const float *qpos;             // [nq][n]: the pose snapshot the frames were drawn from
};

// 0, or the hipError_t of the launch; -1: arguments the kernel is not built for (nothing is launched)
int lcr_launch_heightmap(const LcrHeightmap &A, void *stream);

#endif
