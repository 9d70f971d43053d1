// lcr_obs_cameras.inc.h -- a statement list, included inside the body of a kernel of a depth-plane observation (the cloud's two pass-1 lists, lcr_voxel.hip,
// lcr_heightmap.hip), in the ONE thread that obtains the cameras (lcr_cloud_dev.h says why it is no function).
// In scope before it: `A` (an argument struct with n, slots, cam[], qpos, mount, var, variant, front, top and pose: LcrCloud, LcrVoxel, LcrHeightmap), the LDS array
// `cams` [3][16] and `env`.
// Behind it: cams[sl] holds ro, X, Y, Z, s of every selected slot (store_cam) -- the wrist pose from the link chain, the env's look variant's camera, or the handle's --
// and pose[sl][13][n] of the env is written.  The including kernel places the barrier the other threads wait at.
        for (int sl = 0; sl < A.slots; sl++) {
            LcrCam C;
            if (A.cam[sl] == LCR_CLOUD_CAM_WRIST) {
                float q[6];
                for (int j = 0; j < 6; j++) q[j] = A.qpos[(size_t)j * A.n + env];
                ArmFrames F;
                arm_frames(q, F);
                wrist_camera(F, A.mount, C);
            } else if (A.var) {
                C = A.var[A.variant[env]].cam[A.cam[sl]];
            } else {
                C = A.cam[sl] == LCR_CLOUD_CAM_FRONT ? A.front : A.top;
            }
            store_cam(cams[sl], C);
            float *po = A.pose + (size_t)sl * 13 * A.n + env;
            for (int k = 0; k < 13; k++) po[(size_t)k * A.n] = cams[sl][k];
        }
