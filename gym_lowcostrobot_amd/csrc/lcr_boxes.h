// lcr_boxes.h -- the object boxes (lcr_enable_object_boxes, include/lcr.h): the arguments of their kernel and its launcher (lcr_boxes.hip).
// A header of its own, as lcr_heightmap.h is: lcr_device.h and every kernel that knows nothing of the boxes stay as they are.
#ifndef LCR_BOXES_H
#define LCR_BOXES_H
#include <stddef.h>

#include "../../include/lcr.h"   // LCR_BOXES_MAX_OBJECTS, LCR_BOXES_MARKER

#define LCR_BOXES_THREADS 256   // a workgroup: one (env, camera slot), four waves
#ifndef LCR_BOXES_COPIES
#define LCR_BOXES_COPIES 32     // copies of the LDS table, one a bank: a lane adds to copy (lane mod 32)
#endif

// A VIEW of n envs: planes, sizes, masks and where the records go.  Nothing of the handle is in it, so the same launch can later run over staged planes, as launch_cloud
// takes a view
struct LcrBoxes {
    // per camera slot (the selected cameras in the order front, top, wrist); [i >= slots] unused
    const unsigned char *seg[3];                 // [n][H][W]
    const unsigned *depth[3];                    // [n][H][W], the depth planes' 32-bit words; all null: `nearest` is 0
    int slots, n, W, H;                          // W H a multiple of 16
    int n_objects;                               // 1 .. LCR_BOXES_MAX_OBJECTS
    unsigned masks[LCR_BOXES_MAX_OBJECTS];       // bits 1 .. 10: surface ids; LCR_BOXES_MARKER: the marker bit of the byte
    int *out;                                    // [n][slots][n_objects][8]
};

// 0, or the hipError_t of the launch; -1: arguments the kernel is not built for (nothing is launched)
int lcr_launch_object_boxes(const LcrBoxes &A, void *stream);

#endif
