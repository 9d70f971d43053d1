// lcr_cloud.h -- the point cloud (lcr_enable_point_cloud, include/lcr.h): the arguments of its kernel and its launcher (lcr_cloud.hip).
// A header of its own, as lcr_stack.h is: lcr_device.h and every kernel that knows nothing of the cloud stay as they are.
#ifndef LCR_CLOUD_H
#define LCR_CLOUD_H
#include <stddef.h>

#include "lcr_device.h"

#define LCR_CLOUD_THREADS 256   // a workgroup: one env, four waves
#define LCR_CLOUD_SEG 64        // 16-pixel groups per segment of the prefix: what one wave counts per round

enum { LCR_CLOUD_CAM_FRONT = 0, LCR_CLOUD_CAM_TOP = 1, LCR_CLOUD_CAM_WRIST = 2 };

struct LcrCloud {
    // per camera slot (the selected cameras in the order front, top, wrist); [i >= slots] unused
    const unsigned char *seg[3];   // [n][pixels]
    const float *depth[3];         // [n][pixels]
    const unsigned char *rgb[3];   // [n][pixels][3]
    int cam[3];                    // LCR_CLOUD_CAM_*: where the slot's pose comes from
    int slots, n, W, H;            // pixels = W * H, a multiple of 16
    int points, channels;          // P (a multiple of 64), C = 3 or 6
    unsigned ids;                  // bit i: surface id i is a candidate (bits 1 .. 10)
    float *out;                    // [n][P][C]
    int *count;                    // [n]
    int *source;                   // [n][P]
    float *pose;                   // [slots][13][n]: ro, X, Y, Z, s
    // the cameras: front / top of the handle, or -- var != null -- of the env's look variant; the wrist camera from the link chain of `qpos`
    LcrCam front, top;
    const LcrLookVar *var;         // [K] or null
    const int *variant;            // [n] (with var)
    LcrWristMount mount;
    const float *qpos;             // [nq][n]: the pose snapshot the frames were drawn from
};

// bytes of dynamic LDS a workgroup takes: one count byte per 16-pixel group, rounded up to whole segments
size_t lcr_cloud_lds_bytes(int slots, int pixels);
// whether the point-cloud kernels are built for these arguments (what both launchers check before they launch)
bool lcr_cloud_args_ok(const LcrCloud &A);
// 0, or the hipError_t of the launch; -1: arguments the kernel is not built for (nothing is launched)
int lcr_launch_point_cloud(const LcrCloud &A, void *stream);

// Farthest-point sampling (lcr_enable_point_cloud_sampled with LCR_CLOUD_SAMPLE_FPS; lcr_cloud_fps.hip): the cloud's arguments and the pool.  A struct of its own: LcrCloud
// and the kernel arguments of the strided kernels stay as they are.
struct LcrCloudFps {
    LcrCloud c;   // c.points = P, the points that go out
    int pool;     // Q: a multiple of 64, P <= Q <= LCR_CLOUD_MAX_POOL
};
// as lcr_launch_point_cloud
int lcr_launch_point_cloud_fps(const LcrCloudFps &F, void *stream);

// The cloud inside a crop box (lcr_enable_point_cloud_cropped with a crop; lcr_cloud_crop.hip): the cloud's arguments, the box and the pool.  A struct of its own, as
// LcrCloudFps is: LcrCloud and the kernel arguments of the six kernels without a box stay as they are.
struct LcrCloudCrop {
    LcrCloud c;             // c.points = P, the points that go out
    float lo[3], hi[3];     // the box, WORLD frame: lo[k] <= hi[k], each finite or an infinity (an open side), never NaN
    int pool;               // 0: the strided selection; Q under farthest-point sampling, as LcrCloudFps::pool
};
// as lcr_launch_point_cloud
int lcr_launch_point_cloud_crop(const LcrCloudCrop &B, void *stream);

#endif
