// lcr_device.h -- kernel argument block shared by the C ABI (lcr_capi.hip) and the kernels (lcr_kernels.hip).
#pragma once
#include <stdint.h>

#define LCR_OBS_DIM 18

constexpr int LCR_DEV_NWARM = 124;   // floats per env in LcrDev::warm (layout: lcr_kernels.hip WARM_*; = LCR_NWARM of include/lcr.h)

struct LcrDev {
    int n;            // envs on this device
    int k;            // action components
    int task;         // lcr_task
    int n_substeps;
    int max_steps;    // TimeLimit, <=0 disabled
    int pgs_iters;
    int auto_reset;
    int gripper_active;   // lift / pick_place / stack
    int reward_type;
    int has_target;
    unsigned compat;
    int _pad0;
    long long env_off;
    float dist_thr, height_thr, inv_impratio;
    float cube_mass, cube_minv, cube_iinv;
    // friction of the cube geom (reach_cube.xml:26: 0.5 / torsional 0.005; push_cube_loop.xml:31: 1.5 / 1.5) and of the
    // finger<->cube pair (max rule): ratios used by the elliptic-cone regularisation and projection
    float rt_cube;       // mu_tan^2 / mu_tors^2 of cube contacts
    float inv_mu_c2;     // 1 / mu_tan^2
    float inv_mu_ct2;    // 1 / mu_tors^2
    float rt_fc;         // finger<->cube: mu_tan^2 / mu_tors^2
    float inv_mu_fct2;   // finger<->cube: 1 / mu_tors^2
    int walls;           // PushCubeLoop rails
    int arm_collision;   // link-proxy spheres collide (D3)
    int diag;            // write active_mask / active_count / max_sweeps
    float pgs_tol;       // converged mode (pgs_iters < 0): sweep until max |df| <= pgs_tol (1 + max |f|)
    // reset sampling boxes, fp64 exactly as the reference builds them (reach_cube_env.py:132-139, push:141-148)
    double cube_lo[3], cube_rng[3], tgt_lo[3], tgt_rng[3];
    // state, SoA [component][n]
    float *qpos;      // [nq][n]
    float *qvel;      // [nv][n]
    float *ee_lag;    // [3][n]
    float *target;    // [3][n]
    int *elapsed;     // [n]
    unsigned long long *rng;  // [4][n]  PCG64 state_hi, state_lo, inc_hi, inc_lo
    int *goal;        // [n]  PushCubeLoop current_goal (persists across resets)
    double *sim_time; // [n]  accumulated simulation time (data.time is never reset by the reference)
    // step outputs
    float *reward;
    unsigned char *terminated, *truncated, *is_success, *did_reset;
    float *term_obs;  // [18][n]
    float *term_quat; // [8][n]  cube quaternion(s) of the terminal state (valid where did_reset)
    unsigned *active_mask, *active_count, *max_sweeps, *choice;  // [n] each, diagnostics of the last step (diag != 0)
    float *ctrl_out;  // [6][n] actuator targets of the last step (diag != 0)
    float *scratch;   // one-wave Stack kernels: g rows of the arm-link proxy slot, [12][n] float2; two-wave kernels at two waves per SIMD: Wm records, [groups][64][36]
    // image observations
    unsigned char *img_front, *img_top;  // [n][img_h][img_w][3] or null
    unsigned char *img_bg;               // [2][img_h][img_w][3] env-independent background of camera_front / camera_top, or null
    // (appended: the offsets of everything above are what the tuned default kernels were compiled against)
    float rr_fc;         // finger<->cube: mu_tan^2 / mu_roll^2   (ROLL kernels: lcr_config.finger_cube_condim = 6)
    float inv_mu_fcr2;   // finger<->cube: 1 / mu_roll^2
    int roll;            // 1: finger<->cube slots carry the two rolling rows
    float *warm;         // [LCR_NWARM][n] constraint forces carried from one control step to the next (warm start), or null
    int cc8;             // Stack: eight-point cube<->cube manifold (lcr_config.cc_points = 8; two-wave kernels only)
    int coop;            // 0: one wave per 64 envs (lcr_kernels.hip); 1 / 2: two cooperating waves per 64 envs (lcr_kernels2.hip) compiled for
                         // one / two waves per SIMD (<= 512 / <= 256 registers per lane)
    int big_lds;         // Stack: the shard has at most three waves per CU -> the variant that keeps every g row in LDS (46 / 52 KiB per wave)
    // squared friction coefficients (round 4: the contact blocks take a projected-gradient step in the variables f_j / mu_j, lcr_step_common.h soc_step)
    float mu_c2, mu_ct2;             // cube geom: tangential, torsional
    float mu_fc2, mu_fct2, mu_fcr2;  // finger<->cube pair (max rule): tangential, torsional, rolling
    // the faithful preset (round 5): Newton on the primal (lcr_newton.h), six-row finger contacts against cube AND floor
    int newton;                      // 1: lcr_config.solver = LCR_SOLVER_NEWTON
    int newton_iters, ls_iters;      // most Newton iterations per substep / most evaluations of phi' per line search
    float newton_tol, ls_tol;
    int coop_max;                    // Newton kernels: a wave solves up to this many coupled (arm on cube, cube on cube) envs one by one with all its lanes (lcr_newton_coop.h); more: the 12-dimensional SIMT solve
    int coop_share;                  // one-cube Newton kernel: who solves a wave's coupled envs -- 0 the owning wave only, 1 any wave of the workgroup, the owner first,
                                     // 2 never the owner, 3 as 1 and waves without a coupled env help the waves behind them mid-step (default) (lcr_config.coop_share - 1; lcr_kernels.hip: CoopQueue)
    int img_w, img_h;                // size of the image observations (lcr_config.image_width / image_height; 320 x 240 by default)
    int img_epw;                     // frame kernel: envs per workgroup (1, 2 or 4), chosen from the frame size at lcr_create (lcr_render.hip)
};

// The one-cube Newton kernel as a pair of launches (lcr_kernels.hip: STEP_FAST_ONLY): the kernel with the fast substep copy alone, then the kernel with both copies for
// the waves the first one flagged.  A kernel argument of its own, as LcrPlanes is: LcrDev, and with it the code of every other kernel, stays as it is
struct LcrRedo {
    int *flags;   // [ceil(n / 64) rounded up to the workgroup's four waves] 1: the wave bailed out of the last step's first launch; null: a kernel without the pair
    int gate;     // 1: the pair (default); 0: the kernel with both copies alone, ungated (LCR_REDO_KERNEL=0)
};

// pinhole camera: position, world axes (camera looks along -Z), s = 2 tan(fovy/2) / height
struct LcrCam {
    float px, py, pz;
    float xx, xy, xz, yx, yy, yz, zx, zy, zz;
    float s;
};

// depth / segmentation planes of the image observations (lcr_enable_image_planes).  A kernel argument of its own: LcrDev -- and with it every kernel that draws no planes -- stays as it is
struct LcrPlanes {
    float *depth_front, *depth_top;        // [n][img_h][img_w] metres along the optical axis, clipped at `far`; null: plane not enabled
    unsigned char *seg_front, *seg_top;    // [n][img_h][img_w] ids (include/lcr.h); null: plane not enabled
    float *bg_depth;                       // [2][img_h][img_w] env-independent background (floor, sky, the arm's base) of camera_front / camera_top: what img_bg is for the colours
    unsigned char *bg_seg;                 // [2][img_h][img_w]
    float far;
};

// the look of the image observations (lcr_enable_look).  One variant: everything the cached background depends on -- the two observation cameras, floor, sky, light, the arm's colours
struct LcrLookVar {
    LcrCam cam[2];                         // camera_front, camera_top of this variant (s = 2 tan(fovy / 2) / img_h)
    float ambient, diffuse, _pad[2];       // (16 floats from cam[1] on: what a wave of the frame kernel fetches with one load)
    float floor_rgb[2][3];                 // checker cells: odd, even
    float sky_rgb[3], sky_slope[3];
    float arm_rgb[3], finger_rgb[3];
};
// A kernel argument of its own, as LcrPlanes is: LcrDev and every kernel that draws without a look stay as they are
struct LcrLook {
    const LcrLookVar *var;                 // [K]
    const unsigned char *bg;               // [K][2][img_h][img_w][3] cached backgrounds, one pair per variant
    const int *variant;                    // [n] variant of every env
    const float *rgb;                      // [9][n] cube, second cube, target marker
};
// the sampler of lcr_enable_look as the redraw kernel takes it
struct LcrLookSampler {
    unsigned long long seed;
    float lo[9], rng[9], hi[9];            // cube, second cube, marker: value = min(lo + u rng, hi)
    int on, K;
};

// the wrist camera (lcr_enable_wrist_camera): its mount in the frame of a link, axes finished on the host.  A kernel argument of its own, as LcrPlanes and LcrLook are
struct LcrWristMount {
    int link;                              // 0: world frame, 1 .. 6: body frame of link_1 .. link_6
    float px, py, pz;                      // position in that frame
    float xx, xy, xz, yx, yy, yz, zx, zy, zz;   // axes in that frame (the camera looks along -Z)
    float s;                               // 2 tan(fovy / 2) / height of the frame it is asked to draw
};
struct LcrWrist {
    LcrWristMount mount;
    unsigned char *img;                    // [n][img_h][img_w][3]
    float *depth;                          // [n][img_h][img_w] or null
    unsigned char *seg;                    // [n][img_h][img_w] or null
    float far;
};

// launchers implemented in lcr_kernels.hip / lcr_render.hip (plain C++ linkage, same shared object)
int lcr_launch_step(const LcrDev &P, const float *action_dev, int ee_mode, void *stream, const LcrRedo &redo);
// the Newton kernels of the faithful preset (lcr_kernels.hip, unit LCR_PART = 4)
int lcr_launch_step_newton(const LcrDev &P, const float *action_dev, int ee_mode, void *stream, const LcrRedo &redo);   // (the pair of launches, or the second kernel alone: LcrRedo)
int lcr_launch_step_newton_stack(const LcrDev &P, const float *action_dev, int ee_mode, void *stream);   // (unit LCR_PART = 5)
int lcr_launch_step_loop_newton(const LcrDev &P, const float *action_dev, int ee_mode, void *stream);    // (PushCubeLoop: one wave per 64 envs, unit LCR_PART = 7)
// two-cooperating-waves family (lcr_kernels2.hip); occ = waves per SIMD the variant is compiled for
int lcr_launch_step2_one_cube(const LcrDev &P, const float *action_dev, int ee_mode, int occ, void *stream);
int lcr_launch_step2_stack(const LcrDev &P, const float *action_dev, int ee_mode, int occ, void *stream);
int lcr_launch_step2_stack_cc8(const LcrDev &P, const float *action_dev, int ee_mode, int occ, void *stream);
int lcr_launch_reset(const LcrDev &P, const unsigned char *mask_dev, const unsigned long long *seeds_dev, int seed_from_base,
                     unsigned long long base_seed, void *stream);
int lcr_launch_fill_actions(float *action_dev, int n, int k, long long env_off, unsigned long long seed,
                            unsigned long long step, void *stream);
int lcr_launch_render_obs(const LcrDev &P, const LcrCam &front, const LcrCam &top, void *stream);
int lcr_render_envs_per_workgroup(int W, int H);   // the frame kernel's mapping for a frame size
int lcr_launch_gather_terminal(const LcrDev &P, const int *ids_dev, int count, float *qpos_out, float *target_out, void *stream);
int lcr_launch_render_bg(const LcrDev &P, const LcrCam &front, const LcrCam &top, void *stream);
int lcr_launch_render_single(const LcrDev &P, const LcrCam &cam, int env, int W, int H, unsigned char *out_dev, void *stream);
// the planes (lcr_render.hip, unit LCR_RENDER_PART = 3): colour frames + enabled planes in one launch / their cached background / one env, one ray per pixel
int lcr_launch_render_obs_planes(const LcrDev &P, const LcrCam &front, const LcrCam &top, const LcrPlanes &PL, void *stream);
int lcr_launch_render_bg_planes(const LcrDev &P, const LcrCam &front, const LcrCam &top, const LcrPlanes &PL, void *stream);
int lcr_launch_render_single_planes(const LcrDev &P, const LcrCam &cam, int env, int W, int H, float far, float *depth_dev, unsigned char *seg_dev, void *stream);
int lcr_launch_calib_copy(const float *src, float *dst, size_t n, void *stream);
// the look (lcr_render.hip, unit LCR_RENDER_PART = 4): frames (+ planes when PL is given) / the K cached backgrounds / their planes / one env, one ray per pixel /
// the redraw of the envs a step or a reset has reset / the gather of the terminal looks of listed envs
int lcr_launch_render_obs_look(const LcrDev &P, const LcrLook &LK, const LcrPlanes *PL, void *stream);
int lcr_launch_render_bg_look(const LcrDev &P, const LcrLook &LK, int K, void *stream);
int lcr_launch_render_bg_planes_look(const LcrDev &P, const LcrLook &LK, int K, const LcrPlanes &PL, void *stream);
int lcr_launch_render_single_look(const LcrDev &P, const LcrCam &cam, int env, int W, int H, unsigned char *out_dev, const LcrLook &LK, int look_env, int look_n, void *stream);
// mode 0: envs with flag[e] != 0 (null: all) count an episode and draw its look, `term` (or null) receives the look they had; 1: every env draws the look of episode 0
int lcr_launch_look_redraw(int n, long long env_off, const unsigned char *flag, int mode, const LcrLookSampler &SM, int *cur, unsigned *episode, int *term, void *stream);
int lcr_launch_look_gather(const int *ids_dev, int count, int n, const int *look, int *out, void *stream);
// the wrist camera (lcr_render.hip, unit LCR_RENDER_PART = 5): the batched frames (+ the planes WR points at; LK: with the envs' looks, or null) / one env, one ray per
// pixel into any of rgb_dev, depth_dev, seg_dev (look_env >= 0: with the look of env look_env of LK)
int lcr_launch_render_wrist(const LcrDev &P, const LcrWrist &WR, const LcrLook *LK, void *stream);
int lcr_launch_render_single_wrist(const LcrDev &P, const LcrWristMount &M, int env, int W, int H, float far, unsigned char *rgb_dev, float *depth_dev, unsigned char *seg_dev,
                                   const LcrLook *LK, int look_env, int look_n, void *stream);
