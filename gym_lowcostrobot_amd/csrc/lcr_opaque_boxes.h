// lcr_opaque_boxes.h -- where the nine OPAQUE boxes of an env stand: the seven arm boxes (base_link, link_1 .. link_6), the cube and the second cube (StackTwoCubes), in the
// order of the surface ids 2 .. 10 of the segmentation plane.  Device code for the kernels that need the boxes behind the frame kernels (lcr_normals.hip).
// It is build_scene's placement of lcr_render.hip as a COPY of its text -- base_box, arm_frames + local_point with the lcrm::ARMB* constants, quat_to_cols --: the render
// kernels are not touched, so lcr_render.hip stays instruction for instruction what it is.  Colours, the translucent marker and the per-camera constants are not in it.
#pragma once
#include "lcr_arm.h"

namespace lcrdev {

constexpr int OPAQUE_ARM = 7;     // base_link, link_1 .. link_6 as the bounding boxes of their collision hulls (lcr_model_gen.h ARMB*)
constexpr int OPAQUE_BOXES = 9;   // the arm boxes, then cube, second cube: box b is surface id b + 2

struct OpaqueBoxes {
    f3 c[OPAQUE_BOXES], X[OPAQUE_BOXES], Y[OPAQUE_BOXES], Z[OPAQUE_BOXES], h[OPAQUE_BOXES];
};

DEV void opaque_arm_box(int i, f3 &c, f3 &h) {
    const float bc[OPAQUE_ARM][3] = {{lcrm::ARMB0cx, lcrm::ARMB0cy, lcrm::ARMB0cz}, {lcrm::ARMB1cx, lcrm::ARMB1cy, lcrm::ARMB1cz}, {lcrm::ARMB2cx, lcrm::ARMB2cy, lcrm::ARMB2cz},
                                     {lcrm::ARMB3cx, lcrm::ARMB3cy, lcrm::ARMB3cz}, {lcrm::ARMB4cx, lcrm::ARMB4cy, lcrm::ARMB4cz}, {lcrm::ARMB5cx, lcrm::ARMB5cy, lcrm::ARMB5cz},
                                     {lcrm::ARMB6cx, lcrm::ARMB6cy, lcrm::ARMB6cz}};
    const float bh[OPAQUE_ARM][3] = {{lcrm::ARMB0hx, lcrm::ARMB0hy, lcrm::ARMB0hz}, {lcrm::ARMB1hx, lcrm::ARMB1hy, lcrm::ARMB1hz}, {lcrm::ARMB2hx, lcrm::ARMB2hy, lcrm::ARMB2hz},
                                     {lcrm::ARMB3hx, lcrm::ARMB3hy, lcrm::ARMB3hz}, {lcrm::ARMB4hx, lcrm::ARMB4hy, lcrm::ARMB4hz}, {lcrm::ARMB5hx, lcrm::ARMB5hy, lcrm::ARMB5hz},
                                     {lcrm::ARMB6hx, lcrm::ARMB6hy, lcrm::ARMB6hz}};
    c = mk(bc[i][0], bc[i][1], bc[i][2]); h = mk(bh[i][0], bh[i][1], bh[i][2]);
}

// the boxes of env `env` of n from the pose snapshot qpos ([nq][n]); ncube 1 or 2.  A second cube the task does not have is all zeros
DEV void opaque_boxes(const float *qpos, int n, int env, int ncube, OpaqueBoxes &S) {
    float q[6];
    for (int j = 0; j < 6; j++) q[j] = qpos[(size_t)j * n + env];
    ArmFrames F;
    arm_frames(q, F);
    {   // the base box (body frame of base_link: Rz(-90 deg) at the origin)
        S.X[0] = mk(0.f, -1.f, 0.f); S.Y[0] = mk(1.f, 0.f, 0.f); S.Z[0] = mk(0.f, 0.f, 1.f);
        f3 lc;
        opaque_arm_box(0, lc, S.h[0]);
        S.c[0] = axpy(lc.x, S.X[0], axpy(lc.y, S.Y[0], lc.z * S.Z[0]));
    }
    for (int i = 1; i < OPAQUE_ARM; i++) {   // link_i: frame i - 1 of the chain
        f3 lc;
        opaque_arm_box(i, lc, S.h[i]);
        S.c[i] = local_point(F, i - 1, lc.x, lc.y, lc.z);
        S.X[i] = F.X[i - 1]; S.Y[i] = F.Y[i - 1]; S.Z[i] = F.Z[i - 1];
    }
    for (int c = 0; c < 2; c++) {
        const int nb = OPAQUE_ARM + c;
        if (c >= ncube) {
            S.c[nb] = S.X[nb] = S.Y[nb] = S.Z[nb] = S.h[nb] = mk(0.f, 0.f, 0.f);
            continue;
        }
        const float *qp = qpos + (size_t)(6 + 7 * c) * n + env;
        float cq[4] = {qp[3 * (size_t)n], qp[4 * (size_t)n], qp[5 * (size_t)n], qp[6 * (size_t)n]};
        CubeRot R = quat_to_cols(cq);
        S.c[nb] = mk(qp[0], qp[n], qp[2 * (size_t)n]);
        S.X[nb] = R.X; S.Y[nb] = R.Y; S.Z[nb] = R.Z;
        S.h[nb] = mk(0.015f, 0.015f, 0.015f);
    }
}

}  // namespace lcrdev
