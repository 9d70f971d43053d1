// lcr_wrist_pose.h -- world pose of the wrist camera (lcr_enable_wrist_camera, include/lcr.h) from the chain of link frames.  Device code shared by the kernels that draw
// the wrist frames (lcr_render.hip) and the point-cloud kernel (lcr_cloud.hip), which unprojects the wrist depth with the pose the frames were drawn from.
#pragma once
#include "lcr_arm.h"
#include "lcr_device.h"

namespace lcrdev {

// world pose of the mounted camera, from the chain of link frames that places the arm's boxes: ro = p_link + R_link pos, axes = R_link axes (link 0: the numbers themselves).
// The batched kernel, the single-frame kernel and the point-cloud kernel share it
DEV void wrist_camera(const ArmFrames &F, const LcrWristMount &M, LcrCam &C) {
    C.s = M.s;
    if (M.link == 0) {
        C.px = M.px; C.py = M.py; C.pz = M.pz;
        C.xx = M.xx; C.xy = M.xy; C.xz = M.xz; C.yx = M.yx; C.yy = M.yy; C.yz = M.yz; C.zx = M.zx; C.zy = M.zy; C.zz = M.zz;
        return;
    }
    f3 p, X, Y, Z;   // (literal indices: the chain stays in registers)
    switch (M.link) {
    case 1: p = F.p[0]; X = F.X[0]; Y = F.Y[0]; Z = F.Z[0]; break;
    case 2: p = F.p[1]; X = F.X[1]; Y = F.Y[1]; Z = F.Z[1]; break;
    case 3: p = F.p[2]; X = F.X[2]; Y = F.Y[2]; Z = F.Z[2]; break;
    case 4: p = F.p[3]; X = F.X[3]; Y = F.Y[3]; Z = F.Z[3]; break;
    case 5: p = F.p[4]; X = F.X[4]; Y = F.Y[4]; Z = F.Z[4]; break;
    default: p = F.p[5]; X = F.X[5]; Y = F.Y[5]; Z = F.Z[5]; break;
    }
    const f3 ro = axpy(M.px, X, axpy(M.py, Y, axpy(M.pz, Z, p)));
    const f3 cx = axpy(M.xx, X, axpy(M.xy, Y, M.xz * Z)), cy = axpy(M.yx, X, axpy(M.yy, Y, M.yz * Z)), cz = axpy(M.zx, X, axpy(M.zy, Y, M.zz * Z));
    C.px = ro.x; C.py = ro.y; C.pz = ro.z;
    C.xx = cx.x; C.xy = cx.y; C.xz = cx.z; C.yx = cy.x; C.yy = cy.y; C.yz = cy.z; C.zx = cz.x; C.zy = cz.y; C.zz = cz.z;
}

}  // namespace lcrdev
