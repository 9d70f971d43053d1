/*
 * lcr.h -- C ABI of the MI355X-native batched low-cost-robot simulator (liblcr_hip.so).
 *
 * Drop-in boundary for the ONE hot path of perezjln/gym-lowcostrobot: batched reset()/step() of the
 * ReachCube / LiftCube / PushCube / PickPlaceCube / StackTwoCubes environments.  Each entry point
 * cites the reference interface it replaces (paths relative to /root/reference/gym_lowcostrobot/).
 *
 * Conventions
 *   - one handle (lcr_sim) per GPU; a handle is NOT thread-safe, distinct handles may be driven from
 *     distinct threads / processes (one process per GPU is the intended multi-GPU mode, no collectives).
 *   - every function returns 0 on success or a negative lcr_status; nothing throws across the boundary;
 *     lcr_last_error() gives a thread-local message for the last failure.
 *   - "dev" pointers are HIP device pointers on the handle's device; "host" pointers are ordinary memory.
 *   - all per-env arrays are SoA  [component][env]  with env fastest (coalesced: lane == env), fp32.
 *   - work is enqueued on the handle's HIP stream (lcr_set_stream) and is asynchronous unless stated.
 *   - there is NO CPU fallback: without a gfx950 device lcr_create fails with LCR_ERR_NO_DEVICE.
 */
#ifndef LCR_H
#define LCR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCR_ABI_VERSION 7

typedef enum lcr_status {
    LCR_OK = 0,
    LCR_ERR_INVALID = -1,     /* bad argument / config (maps to ValueError in the Python facade) */
    LCR_ERR_NO_DEVICE = -2,   /* no HIP device / wrong architecture */
    LCR_ERR_HIP = -3,         /* a HIP runtime call failed (message has hipGetErrorString) */
    LCR_ERR_OOM = -4,
    LCR_ERR_UNSUPPORTED = -5
} lcr_status;

/* gym_lowcostrobot/__init__.py:9-43 registry ids */
typedef enum lcr_task {
    LCR_TASK_REACH = 0,       /* ReachCube-v0       envs/reach_cube_env.py */
    LCR_TASK_LIFT = 1,        /* LiftCube-v0        envs/lift_cube_env.py */
    LCR_TASK_PUSH = 2,        /* PushCube-v0        envs/push_cube_env.py */
    LCR_TASK_PICK_PLACE = 3,  /* PickPlaceCube-v0   envs/pick_place_cube_env.py */
    LCR_TASK_STACK = 4,       /* StackTwoCubes-v0   envs/stack_two_cubes_env.py */
    LCR_TASK_PUSH_LOOP = 5    /* PushCubeLoop-v0    envs/push_cube_loop_env.py */
} lcr_task;

enum { LCR_ACTION_JOINT = 0, LCR_ACTION_EE = 1 };            /* action_mode   reach_cube_env.py:80 */
enum { LCR_OBS_IMAGE = 0, LCR_OBS_STATE = 1, LCR_OBS_BOTH = 2 }; /* observation_mode reach_cube_env.py:79 */
enum { LCR_REWARD_SPARSE = 0, LCR_REWARD_DENSE = 1 };        /* reward_type   reach_cube_env.py:81 */

/* compat bits: every reference quirk is reproduced when the bit is CLEAR */
enum {
    LCR_COMPAT_ZERO_QVEL_ON_RESET = 1u << 0, /* set: zero qvel in reset (deviates from reach_cube_env.py:297-311) */
    LCR_COMPAT_COLD_SOLVE_EACH_STEP = 1u << 1 /* set: the contact solver starts every control step from zero forces, so that a step is a pure
                                                 function of (qpos, qvel, action).  Clear (default): the forces of the last substep warm-start
                                                 the next control step, as MuJoCo's mjData.qacc_warmstart does across env.step calls (the
                                                 reference never resets it); lcr_reset / auto-reset / lcr_set_state clear them */
};

/* the default size of the image observations (the reference's, reach_cube_env.py:288-292): lcr_config.image_width = image_height = 0 */
#define LCR_IMG_H 240
#define LCR_IMG_W 320

/* Constructor kwargs of the reference env classes (reach_cube_env.py:77-87, lift_cube_env.py:77-88,
 * push_cube_env.py:79-90, pick_place_cube_env.py:79-91, stack_two_cubes_env.py:78-88) plus the batch
 * / device placement the reference does not have. */
typedef struct lcr_config {
    uint32_t struct_size;      /* = sizeof(lcr_config), ABI check */
    int32_t task;              /* lcr_task */
    int32_t n_envs;            /* envs on this GPU, 1 .. 67 108 864 (2^26) per handle */
    int32_t device;            /* HIP device ordinal */
    int64_t env_id_offset;     /* global id of env 0 (sharding: GPU g owns [g*N/G, (g+1)*N/G)) */
    int32_t action_mode;
    int32_t obs_mode;
    int32_t reward_type;
    int32_t block_gripper;     /* -1 = task default (reach/push: 1, others: 0) */
    double distance_threshold; /* 0.05  (doubles: the reset sampling boxes are built in fp64 exactly as the */
    double cube_xy_range;      /* 0.3    reference does, reach_cube_env.py:132-139)                        */
    double target_xy_range;    /* 0.3 */
    double goal_z_range;       /* 0.1  (pick_place) */
    double height_threshold;   /* 0.1  (lift) */
    double impratio;           /* 100, follower.xml:3 */
    int32_t n_substeps;        /* 20 */
    int32_t max_episode_steps; /* 50, gymnasium TimeLimit configured at __init__.py:12-42; <=0 disables */
    int32_t pgs_iters;         /* warm-started PGS sweeps per substep, 4; < 0: "converged" mode -- sweep until the largest force
                                  change of a sweep is <= pgs_tol (1 + largest |force|) in every env of the wave, at most 50 sweeps */
    uint32_t compat;
    int32_t auto_reset;        /* 1: SB3 VecEnv semantics fused in the step kernel */
    int32_t arm_collision;     /* 1 (default): the arm links collide with the floor / cube through sphere proxies (follower.xml:10,13:
                                  every arm geom collides in the reference); 0: finger tips only */
    uint64_t base_seed;        /* envs never explicitly seeded use SeedSequence(base_seed + global env id) */
    double pgs_tol;            /* 1e-6; used when pgs_iters < 0 */
    int32_t diagnostics;       /* 0 | 1: lcr_out_view.active_mask / active_count / max_sweeps / choice / ctrl are written by every step (the decision
                                  signature).  2, 3: profiling aids -- the same arrays carry per-wave cycle counters instead (2: one-wave kernels,
                                  which it also selects; 3: phases of the two-wave kernels).  Anything else: LCR_ERR_INVALID */
    int32_t finger_cube_condim; /* rows of a finger<->cube contact.  6 = MuJoCo's: normal, two tangents, torsion, two rolling (follower.xml:15
                                  condim="6" wins the max rule over the cube's 4; rolling coefficient = max of both geoms).  4 = without the
                                  rolling rows (sweep kernels only, 8-12 % faster there).  lcr_config_default (= LCR_PRESET_FAITHFUL): 6 on every task,
                                  4 is LCR_ERR_UNSUPPORTED under LCR_SOLVER_NEWTON.  LCR_PRESET_FAST: 6 for PushCubeLoop (coefficient 1.5 m) and
                                  StackTwoCubes (light cubes), 4 for the other tasks (deviation D4).  0 = the preset's default */
    int32_t step_kernel;       /* LCR_SOLVER_PGS (LCR_PRESET_FAST) only -- the Newton kernels of the default preset are ONE family (one wave per 64 envs; 2 is
                                  LCR_ERR_UNSUPPORTED with them).  Which step-kernel family runs lcr_step: 0 = by task and JOB size (global_envs below, never the shard size n_envs): two
                                  cooperating waves per 64 envs for ReachCube / LiftCube / PushCube / PickPlaceCube at every size and for StackTwoCubes
                                  jobs of <= 32 envs per SIMD of the device (MI355X: 32 768 envs), one wave per 64 envs for larger Stack jobs -- the faster family when the job runs as ONE shard
                                  on an MI355X; 1 = one wave per 64 envs always; 2 = two cooperating waves always (the faster family on shards of
                                  <= 32 768 envs whatever the job size: a Stack job sharded that finely pins 2).  PushCubeLoop has ONE kernel (one wave
                                  per 64 envs, its own row-wise solver): 0 and 1 run it, 2 is LCR_ERR_UNSUPPORTED.  The families
                                  regroup the same arithmetic and agree to fp32 rounding (~1e-7 per control step), not bit for bit; WITHIN a family
                                  results are bit-identical for every sharding.  Because 0 looks at the job and not at the shard, every sharding of a
                                  job whose shards declare the same global_envs runs the same family and gives identical bits; which
                                  build of the family a shard runs (one / two waves per SIMD, rows in LDS / global scratch) does follow its size and
                                  does not change a bit.  The Stack family boundary is counted in SIMDs of the device the handle lives on: a job replayed on
                                  another part may pick the other family (fp32 rounding apart, not bit for bit). */
    int32_t cc_points;         /* StackTwoCubes: cube<->cube manifold points kept per substep.  4 (default, 0 = default): the extremes along the diagonals
                                  of the reference face; 8: also the extremes along its two axes -- as many points as MuJoCo's box-box
                                  collider may return (stack_two_cubes.xml:25-35; narrows deviation D5).  8 runs on the
                                  two-cooperating-waves kernels (step_kernel = 1 with it: LCR_ERR_UNSUPPORTED); other tasks: LCR_ERR_INVALID */
    int64_t global_envs;       /* ABI v4: number of envs of the whole JOB this handle is one shard of (all GPUs together); 0 = n_envs (the handle is
                                  the job).  Must be >= env_id_offset + n_envs.  The reference has one independent MjData per env
                                  (reach_cube_env.py:89-90), so how a batch is cut into shards must not show in the results: every sharding of a job
                                  gives identical bits PROVIDED the shards are cut at wave boundaries -- a wave (64 consecutive env ids) skips work no
                                  lane needs, solves its coupled envs cooperatively and leaves the solver loops for all its lanes at once, so an env's
                                  low-order bits depend on its 63 wave-mates.  lcr_create therefore refuses (LCR_ERR_INVALID) a handle whose
                                  env_id_offset is not a multiple of 64 and a shard that, not being the job's last (env_id_offset + n_envs <
                                  global_envs), does not hold a multiple of 64 envs.  The step_kernel = 0 dispatch reads global_envs as well (see there) */
    /* ABI v5 (round 5): the solver of the constraint problem and the rows of a finger<->floor contact.  See lcr_config_preset. */
    int32_t solver;            /* lcr_solver.  LCR_SOLVER_NEWTON: Newton's method on the primal problem, all accelerations at once, warm-started from the carried
                                  constraint forces -- MuJoCo's default solver (follower.xml:3 names none); reaches the optimum of MuJoCo's convex constraint problem to
                                  float rounding (tools/kkt_distance.py).  LCR_SOLVER_PGS: pgs_iters warm-started sweeps of a block projected-gradient step on the dual
                                  problem (rounds 1-4; p90 2e-4 / p99 1e-2 rad per control step away from that optimum at four sweeps). */
    int32_t newton_iters;      /* LCR_SOLVER_NEWTON: most iterations per substep (30: what bounds a cold start on a hard contact set -- a finger set 5 mm into the floor -- warm-started, an env needs one on average and seven at the 99th percentile); a wave leaves the loop when every one of its envs has converged */
    int32_t ls_iters;          /* ... most evaluations of phi' per line search (8) */
    int32_t finger_floor_condim; /* rows of a finger<->floor contact: 6 = MuJoCo's (follower.xml:15 condim="6": + two rolling rows, coefficient 1e-4 m), 4 = without
                                  them.  0 = the preset's default.  6 is implemented by the Newton kernels (LCR_SOLVER_PGS with 6: LCR_ERR_UNSUPPORTED) */
    double newton_tol;         /* LCR_SOLVER_NEWTON: an env has converged when its Newton decrement -g'dx <= newton_tol^2 (1 + |a0|_M^2)   (1e-6) */
    double ls_tol;             /* ... its line search stops when |phi'(al)| <= ls_tol |phi'(0)|   (1e-2: MuJoCo's default ls_tolerance), plus a rounding floor 1e-5 (|M-part| + |force part|) of the two sums phi' is the difference of */
    /* ABI v6 */
    int32_t coop_share;        /* LCR_SOLVER_NEWTON, one-cube tasks: who solves the coupled envs of a wave (arm on its cube; four per pass with the whole wave).  The kernel runs
                                  four waves per workgroup; a wave stages its coupled envs into a queue in LDS before its small solves, and 2 = shared: any wave of the
                                  workgroup claims them, the owner its own first, and a wave that has finished its step keeps serving the queue; 1 = owner only; 3 = always hand
                                  off (another wave solves them: tests); 4 = ahead: shared, and a wave that has no coupled env in a substep makes one pass over the queued envs of waves
                                  that are at an earlier substep; 5 = early (0 = default): ahead, and every wave, coupled envs of its own or not, makes such a pass before its small
                                  solves, between them and when its own coupled envs are solved as well.  A/B switch only: the results are bit-identical under all five.  Other values: LCR_ERR_INVALID */
    /* ABI v7 */
    int32_t image_width;       /* image_width x image_height: size of the image observations (observation_mode image / both; checked whatever the mode).  0, 0 = LCR_IMG_W x LCR_IMG_H (320 x 240, the
                                  reference's).  Otherwise each a multiple of 4 in [16, 512]: a band of 4 rows is 12 W bytes, a multiple of 16 exactly when W % 4 == 0, so every
                                  band and every frame (3 W H bytes) stays 16-byte aligned for the frame kernel's 16-B stores; W <= 512 keeps its mask of 16-pixel tile columns
                                  in one 32-bit word.  One zero and one non-zero, or anything else: LCR_ERR_INVALID */
    int32_t image_height;
} lcr_config;

typedef enum lcr_solver { LCR_SOLVER_PGS = 0, LCR_SOLVER_NEWTON = 1 } lcr_solver;
/* LCR_PRESET_FAITHFUL (what lcr_config_default fills in): the reference's contact model as its MJCF states it -- six-row finger contacts against cube AND floor
 * (follower.xml:15), up to eight box-box points (stack_two_cubes.xml:25-35), elliptic cones -- solved by Newton's method (follower.xml:3).
 * What remains approximate under it: finger pads are boxes fitted to the hull tips and the other arm hulls five sphere proxies (deviation D3), each finger has one
 * world contact (floor or rail), Newton is capped at newton_iters = 30 iterations per substep, fp32 arithmetic.
 * LCR_PRESET_FAST: the rounds 1-4 configuration -- four block projected-gradient sweeps, rolling rows only where they change a step by more than the fp32
 * parity tolerance, four box-box points -- 8 x (ReachCube, PushCubeLoop) to 13 x (StackTwoCubes) the throughput of the default (measured per task: profiles/r06_quick_times.txt)
 * at p90 2e-4 / p99 1e-2 rad per control step from the optimum.  Options of the sweep kernels (step_kernel = 2, pgs_iters < 0,
 * diagnostics = 3, finger_cube_condim = 4) are refused under LCR_SOLVER_NEWTON: set them on a config filled by lcr_config_preset(.., LCR_PRESET_FAST). */
typedef enum lcr_preset { LCR_PRESET_FAITHFUL = 0, LCR_PRESET_FAST = 1 } lcr_preset;

typedef struct lcr_sim lcr_sim;

/* Read-only device views.  arm_qpos/arm_qvel/cube_pos (and cube_blue_pos for Stack) alias the state
 * arrays themselves (get_observation() reach_cube_env.py:281-295 returns exactly those qpos/qvel
 * slices cast to float32); target_pos aliases the per-env target (push_cube_env.py:297). */
typedef struct lcr_obs_view {
    int32_t n_envs;
    int32_t has_aux;            /* 1 if aux_pos is meaningful (push/pick_place: target_pos; stack: cube_blue_pos) */
    const float *arm_qpos;      /* [6][N] */
    const float *arm_qvel;      /* [6][N] */
    const float *cube_pos;      /* [3][N]  (stack: cube_red_pos) */
    const float *aux_pos;       /* [3][N]  or NULL */
    const uint8_t *image_front; /* [N][H][W][3] at the configured size, or NULL (observation_mode image/both); approximate ray-cast, see lcr_render.hip */
    const uint8_t *image_top;   /* [N][H][W][3] or NULL */
    int32_t image_width;        /* ABI v7: the size in use, image_width x image_height (320, 240 by default; 0, 0 without images) */
    int32_t image_height;
} lcr_obs_view;

/* step() return values (reach_cube_env.py:313-333) + SB3 auto-reset bookkeeping */
typedef struct lcr_out_view {
    int32_t n_envs;
    int32_t _pad;
    const float *reward;        /* [N] */
    const uint8_t *terminated;  /* [N] */
    const uint8_t *truncated;   /* [N]  TimeLimit */
    const uint8_t *is_success;  /* [N]  info["is_success"] (lift: always 0, reference returns info={}) */
    const uint8_t *did_reset;   /* [N]  1 where the env was auto-reset at the end of this step */
    const float *terminal_obs;  /* [18][N] arm_qpos6, arm_qvel6, cube_pos3, aux3 -- valid where did_reset */
    const float *terminal_quat; /* [8][N]  cube quaternion(s) of the terminal state (with terminal_obs: the full terminal pose) */
    const double *timestamp;    /* [N]  accumulated simulation time = info["timestamp"] of PushCubeLoop-v0 (push_cube_loop_env.py:328) */
    const int32_t *current_goal;/* [N]  PushCubeLoop-v0 goal side (0|1), persists across resets (push_cube_loop_env.py:136,341) */
    /* solver diagnostics of the last step, valid when lcr_config.diagnostics != 0 (else NULL): bit s of active_mask = constraint
     * slot s was active in some substep (0-7 floor<->cube, 8-11 cube<->cube / rails, 12-13 finger<->cube, 14-15 finger<->floor,
     * 16 arm-link proxies, 18+j joint limit j); active_count = number of (slot, substep) activations;
     * max_sweeps = most PGS sweeps of a substep; choice = wrapping sum over substeps s (weight 2s+1) and active constraints of
     * (slot + 1)(sel + 1) 2654435761 with sel the discrete choice behind the contact (vertex index, manifold candidate, box
     * face, proxy member, limit side) + 0x9E3779B1 x executed IK iterations: two runs that agree in these four words went
     * through the same sequence of discrete decisions */
    const uint32_t *active_mask, *active_count, *max_sweeps, *choice; /* [N] each */
    const float *ctrl;          /* [6][N] actuator targets data.ctrl as apply_action left them (reach_cube_env.py:273); diagnostics only */
} lcr_out_view;

/* Host-side mirror of everything a host vector env needs after a step (lcr_fetch_host): pointers into a pinned buffer owned
 * by the handle, SoA [component][N] like the device views, valid until the next lcr_fetch_host / lcr_destroy. */
typedef struct lcr_host_view {
    int32_t n_envs;
    int32_t any_reset;          /* 1 if some env was auto-reset in the last step (terminal_obs is then current) */
    const float *arm_qpos;      /* [6][N] */
    const float *arm_qvel;      /* [6][N] */
    const float *cube_pos;      /* [3][N] */
    const float *aux_pos;       /* [3][N] or NULL */
    const float *reward;        /* [N] */
    const uint8_t *terminated, *truncated, *is_success, *did_reset; /* [N] each */
    const float *terminal_obs;  /* [18][N], copied only when any_reset */
} lcr_host_view;

/* Environment variables the library reads (measurement / A-B overrides, none needed in production; all read at lcr_create unless stated):
 *   LCR_COOP_MAX=n        Newton kernels: coupled envs per wave solved cooperatively before the wave falls back to the coupled SIMT solves (default 8; 16 for
 *                         StackTwoCubes and PushCubeLoop; 0 = never cooperatively)
 *   LCR_REDO_KERNEL=0     one-cube Newton kernel: the kernel with both substep copies alone instead of the fast-copy-only kernel followed by it (lcr_get_redo_flags)
 *   LCR_RENDER_OVERLAP=0  image observations: frames on the handle's stream after the step kernel instead of on the second stream (see lcr_step)
 *   LCR_STEP_KERNEL=single|coop1|coop2, LCR_STACK_LDS=small|big   sweep kernels (LCR_PRESET_FAST): pin a kernel family / LDS variant
 *   LCR_RENDER_EPW=1|2|4  frame kernel, frames up to 170 px wide: envs per workgroup instead of the choice by frame size (tools/frame_sizes.py; same bytes under all three)
 *   LCR_RENDER_COUNT=1    frame kernel: count ray-cast passes into the diagnostics arrays (tools/render_work.py; read at the first frame launch) */
int lcr_abi_version(void);
const char *lcr_last_error(void);

/* Fill `cfg` with the reference constructor defaults for `task`. */
int lcr_config_default(lcr_config *cfg, int task);
/* The reference constructor defaults for `task` with the solver / contact-row settings of `preset` (lcr_preset). */
int lcr_config_preset(lcr_config *cfg, int task, int preset);
/* Number of action components k for a config: {joint:5, ee:3} + (0 if block_gripper else 1)  (reach_cube_env.py:95-96) */
int lcr_action_dim(const lcr_config *cfg);
int lcr_nq(int task); /* 13, stack 20 */
int lcr_nv(int task); /* 12, stack 18 */

/* == EnvClass.__init__ (reach_cube_env.py:77-139): allocate device state for n_envs envs.  The envs are
 * left in the post-reset state of seed (base_seed + global env id). */
int lcr_create(const lcr_config *cfg, lcr_sim **out);
void lcr_destroy(lcr_sim *sim); /* == close() reach_cube_env.py:357-363; frees everything the enable calls allocated (planes, look, wrist camera, observation stack) */

/* Which step-kernel family this handle runs (decided at lcr_create from lcr_config.step_kernel and the shard size): 0 = one wave per 64 envs
 * (lcr_step_kernel), 1 / 2 = two cooperating waves per 64 envs (lcr_step2_kernel) compiled for one / two waves per SIMD. */
int lcr_step_kernel_family(lcr_sim *sim);

/* Debug accessor (tests, profiling).  The one-cube tasks under LCR_SOLVER_NEWTON step with a pair of launches: a kernel that holds only the substep copy with
 * 6-dimensional solves, and behind it the kernel with the coupled SIMT copy as well, which repeats -- from the untouched state -- the control step of the 64-env waves
 * that gave up in the first (more than LCR_COOP_MAX coupled envs in a substep) and leaves at once when there is none.  flags_host[w] (capacity >= ceil(N / 64) words;
 * NULL: only the counts) is 1 if wave w went through the second launch in the LAST lcr_step; a host wait on the handle's stream.  *n_waves: ceil(N / 64), or 0 for
 * a handle whose kernel keeps no such flags (every other task / solver; the flags are then not written).  *paired: 1 the pair, 0 the second kernel alone and ungated
 * (LCR_REDO_KERNEL=0: the flags stay zero). */
int lcr_get_redo_flags(lcr_sim *sim, int32_t *flags_host, int32_t capacity, int32_t *n_waves, int32_t *paired);

/* HIP stream (hipStream_t passed as void*) all later work is enqueued on; NULL = default stream.  Synchronises the OLD stream (a host wait, after making it wait for
 * frames still being ray-cast) before it switches: whatever was enqueued on it -- a step, a reset, lcr_fill_random_actions -- has finished when work on the new stream
 * begins, the two streams need no ordering of the caller's.  Meant to be called once, not in a loop. */
int lcr_set_stream(lcr_sim *sim, void *hip_stream);
int lcr_sync(lcr_sim *sim); /* hipStreamSynchronize on the handle's stream (after making it wait for frames still being ray-cast, see lcr_step) */

/* == reset(seed) (reach_cube_env.py:297-311, push:308-328, pick_place:316-336, stack:307-324).
 * mask_host: N bytes, nonzero = reset that env, NULL = all.  seeds_host: N uint64, env i is re-seeded
 * with numpy's Generator(PCG64(SeedSequence(seeds[i]))) before sampling; NULL = continue each env's
 * generator stream (gymnasium reset(seed=None) semantics). */
int lcr_reset(lcr_sim *sim, const uint8_t *mask_host, const uint64_t *seeds_host);

/* == step(action) (reach_cube_env.py:313-333) for all envs: apply_action (joint or ee+IK) -> 20 physics
 * substeps -> reward / terminated / truncated -> fused auto-reset.  action_dev: [k][N] float32.
 * Asynchronous.  With image observations the two frames of every env (at the configured size) are ray-cast on a second, internal stream from a snapshot of the poses, so that the step kernel of
 * the NEXT lcr_step overlaps them (BASELINE config 5: 9.7 -> see DESIGN.md section 3.4).  The planes, the wrist frames and the observation stack are made on the same
 * stream, behind them.  Every other entry point that takes the handle first makes the handle's stream wait for all of these (a "join") -- EXCEPT lcr_step itself,
 * lcr_fill_random_actions, lcr_get_outputs and lcr_step_kernel_family, which touch none of them; the calls that take no handle have no stream to join.  A join is a
 * hipStreamWaitEvent on the handle's stream, not a host wait: the host goes on, and work enqueued on the handle's stream afterwards sees the frames of the last step.  A
 * caller that reads lcr_obs_view.image_* (or the planes, the wrist frames, the stack) with its own kernels on the handle's stream calls a joining entry point after the
 * step first: lcr_get_obs is the cheap one, lcr_sync also blocks the host.  Reads enqueued before the NEXT lcr_step are finished before that step's frames overwrite them.
 * LCR_RENDER_OVERLAP=0 in the environment: frames on the handle's stream, after the step kernel. */
int lcr_step(lcr_sim *sim, const float *action_dev);
/* Convenience for host callers (single-env facade): copies [k][N] host floats then steps. */
int lcr_step_host(lcr_sim *sim, const float *action_host);

/* Views into the state arrays and the two frames.  Joins (see lcr_step): what is enqueued on the handle's stream after this call reads the frames of the last step. */
int lcr_get_obs(lcr_sim *sim, lcr_obs_view *out);
/* == what DummyVecEnv.step_wait hands to SB3 (examples/gym_manipulation_sb3.py:34-39): state observations + rewards + flags of
 * all envs in ONE device-to-host copy into pinned memory (132 B/env), plus the terminal observations (72 B/env) only when some
 * env was reset.  Synchronises the handle's stream. */
int lcr_fetch_host(lcr_sim *sim, lcr_host_view *out);
int lcr_get_outputs(lcr_sim *sim, lcr_out_view *out); /* does not join: the step kernel writes all of it, on the handle's stream */

/* Full simulator state (replaces poking env.data.qpos / env.data.qvel, e.g. examples/dynamixel_gym_leader.py:96-98;
 * also checkpoint/resume and the "(qpos, qvel, action) triple" parity tests).  Host pointers, any may be
 * NULL, SoA [component][N]; synchronous.
 * `warm` (ABI v3) is the solver state the reference keeps in mjData.qacc_warmstart between env.step calls
 * (reach_cube_env.py:276-279 never resets it): the constraint forces of the last substep, [LCR_NWARM][N] float32 --
 *   rows  0..31  floor<->cube      [cube c][vertex slot s][row k]   at 16 c + 4 s + k   (rows: normal, t1, t2, torsion)
 *   rows 32..61  arm-coupled slots [slot s][row k]                  at 32 + 6 s + k     (s: 0,1 finger<->cube, 2,3 finger<->floor,
 *                                                                                           4 arm-link proxies; k < 4, or 6 with rolling rows)
 *   rows 62..67  joint limits      [joint j]                        at 62 + j
 *   rows 68..83  rails (PushCubeLoop) [slot s][row k]               at 68 + 4 s + k
 *   rows 84..99  cube<->cube (Stack)  [slot s][row k]               at 84 + 4 s + k
 *   rows 100..103 cube<->cube slot s was active in the last substep (0.0 / 1.0)
 *   rows 104..119 cube<->cube slots 4..7 of the eight-point manifold (cc_points = 8) [slot s - 4][row k]  at 104 + 4 (s - 4) + k
 *   rows 120..123 their "was active" flags
 * lcr_get_state + lcr_set_state with all arrays including `warm` is an exact checkpoint: the next lcr_step is bit-identical to
 * the one the un-checkpointed sim would have made.  lcr_set_state with qpos or qvel but warm == NULL clears the carried forces
 * (cold solve in the first substep of the next step); with LCR_COMPAT_COLD_SOLVE_EACH_STEP nothing is carried: get returns zeros,
 * set ignores `warm`. */
#define LCR_NWARM 124
int lcr_get_state(lcr_sim *sim, double *qpos /*[nq][N]*/, double *qvel /*[nv][N]*/, double *ee_lag /*[3][N]*/,
                  float *target /*[3][N]*/, int32_t *elapsed /*[N]*/, uint64_t *rng /*[4][N]*/,
                  int32_t *current_goal /*[N]*/, double *sim_time /*[N]*/, float *warm /*[LCR_NWARM][N]*/);
int lcr_set_state(lcr_sim *sim, const double *qpos, const double *qvel, const double *ee_lag, const float *target,
                  const int32_t *elapsed, const uint64_t *rng, const int32_t *current_goal, const double *sim_time,
                  const float *warm);

/* small device-memory helpers so a ctypes/numpy caller needs no other GPU library */
int lcr_malloc(lcr_sim *sim, size_t bytes, void **dev_out);
int lcr_free(lcr_sim *sim, void *dev);
int lcr_memcpy_h2d(lcr_sim *sim, void *dst_dev, const void *src_host, size_t bytes); /* synchronous */
int lcr_memcpy_d2h(lcr_sim *sim, void *dst_host, const void *src_dev, size_t bytes); /* synchronous */

/* HIP-event timing on the handle's stream: begin, enqueue work, end (synchronises) -> milliseconds */
int lcr_timer_begin(lcr_sim *sim);
int lcr_timer_end(lcr_sim *sim, float *ms_out);

/* Fill action_dev [k][N] with U(-1,1) from a counter-based generator keyed (seed, global env id, step):
 * the synthetic policy of the benchmark; shard-invariant by construction. */
int lcr_fill_random_actions(lcr_sim *sim, float *action_dev, uint64_t seed, uint64_t step);

/* == render() with render_mode="rgb_array" (reach_cube_env.py:350-355: 640x640 frame of camera_vizu) and ad-hoc frames of
 * the observation cameras: ray-cast env `env` from camera 0 (camera_front), 1 (camera_top) or 2 (camera_vizu) at
 * width x height into rgb_host[height][width][3].  Synchronous. */
int lcr_render(lcr_sim *sim, int env, int camera, int width, int height, uint8_t *rgb_host);   /* (camera 3: the wrist camera, on a handle that has one -- see lcr_enable_wrist_camera) */
/* The same for an arbitrary pose given by the caller (qpos_host[nq] as env.data.qpos, target_host[3] or NULL): e.g. the last
 * frame of an episode whose env the step kernel has already reset (terminal_obs + terminal_quat).  Does not touch the sim state. */
int lcr_render_state(lcr_sim *sim, int camera, int width, int height, const double *qpos_host, const float *target_host, uint8_t *rgb_host);

/* Batched last frames of finished episodes (what DummyVecEnv puts into infos[i]["terminal_observation"]["image_front" / "image_top"],
 * examples/gym_manipulation_sb3.py:34-39 with observation_mode image / both; reach_cube_env.py:288-292): the step kernel has already reset
 * those envs, so their frame buffers show the reset state; this draws camera_front / camera_top of the TERMINAL poses (terminal_obs +
 * terminal_quat of the last step) of the `count` listed envs with the observation ray-caster, as one batch, into
 * front_host / top_host [count][H][W][3] (the configured size).  Needs observation_mode image / both.  Synchronous.
 * PRECONDITION: every listed env was reset by the LAST lcr_step (out.did_reset[id] != 0) -- the terminal pose arrays are written only by lanes that auto-reset, an
 * env that did not finish shows the last frame of an OLDER episode (or zeros before its first reset).  The library does not re-read did_reset here; the Python
 * binding (VecSim.render_terminal) checks it and raises ValueError. */
int lcr_render_terminal(lcr_sim *sim, const int32_t *env_ids_host, int count, uint8_t *front_host, uint8_t *top_host);

/* == Depth and segmentation planes of the image observations (MuJoCo's Renderer.enable_depth_rendering / enable_segmentation_rendering, the renderer of
 * reach_cube_env.py:112; the reference's envs never switch them on).  The frame kernel knows the nearest surface of every pixel it draws and the distance to it;
 * with planes enabled it writes them beside the colours, in the same launch, at the configured frame size.
 *   ray    of pixel (row, px): d = sx X + sy Y - Z for the camera axes X, Y, Z (un-normalised; sx, sy as the colours have them).  d . (-Z) = 1, so the ray parameter t
 *          IS the distance along the optical axis in metres -- the z-depth a depth camera reports, not the radial distance.
 *   depth  float32 metres: min(t of the nearest opaque surface, depth_far).  Floor: t = -ro.z / d.z where the normalised d.z < -1e-6 (the horizon rule of the
 *          colours); sky: depth_far.  No near plane beyond t > 0.  depth_far is the caller's: finite, in (0, 1000] m.
 *   seg    uint8: the low 7 bits are the id of the nearest opaque surface -- 0 sky, 1 floor, 2 .. 8 base_link, link_1 .. link_6 (the seven arm boxes), 9 the cube
 *          (StackTwoCubes: the red one), 10 the second cube (StackTwoCubes only).  Bit 7 (0x80) is set where the translucent target marker (PushCube / PickPlaceCube)
 *          covers the pixel in front of that surface; the marker never writes depth and never becomes the id, as it only blends into the colours.
 *   layout [N][H][W] per camera, (H, W) = the size of the colour frames.  Memory: 2 x 4 B (depth) + 2 x 1 B (segmentation) per pixel and env beside 2 x 3 B of
 *          colour -- 768 000 B per env at 320 x 240 beside 460 800 B. */
enum { LCR_PLANE_DEPTH = 1, LCR_PLANE_SEGMENTATION = 2 };
typedef struct lcr_planes_view {
    uint32_t planes;                           /* LCR_PLANE_* bits in use; 0: no planes, everything below is 0 / NULL */
    int32_t image_width, image_height;
    float depth_far;
    const float *depth_front, *depth_top;      /* device, [N][H][W], or NULL */
    const uint8_t *seg_front, *seg_top;        /* device, [N][H][W], or NULL */
} lcr_planes_view;

/* Switch the planes on (`planes`: LCR_PLANE_* bits, at least one; depth_far in metres).  `planes` and `depth_far` are checked before the handle is looked at; then a NULL
 * handle and a handle without image observations are refused -- all with LCR_ERR_INVALID and the argument's name in the message.  Allocates the plane buffers and the
 * cached background planes (floor, sky, the arm's base) and ray-casts them from the current state.  From then on whatever draws the colour frames -- the step, reset and
 * its masked no-op form -- draws the planes in the same launch, so they share the frames' stream ordering.  A second call with the same arguments does nothing, one
 * with other arguments is refused: the planes are fixed for the life of the handle. */
int lcr_enable_image_planes(lcr_sim *sim, uint32_t planes, float depth_far);
/* The plane buffers; waits (on the handle's stream) for frames still being ray-cast on the second stream, as every entry point but the step does. */
int lcr_get_image_planes(lcr_sim *sim, lcr_planes_view *out);
/* One env / an arbitrary pose, any camera (0 front, 1 top, 2 vizu), any size, one ray per pixel: the siblings of the two single-frame calls above.  Either of
 * depth_host[height][width] / seg_host[height][width] may be NULL.  They work without planes enabled; the far clip is the handle's depth_far when they are, else 10. */
int lcr_render_planes(lcr_sim *sim, int env, int camera, int width, int height, float *depth_host, uint8_t *seg_host);
int lcr_render_state_planes(lcr_sim *sim, int camera, int width, int height, const double *qpos_host, const float *target_host, float *depth_host, uint8_t *seg_host);
/* The batched sibling of the terminal-frames call above (same precondition): the enabled planes of the TERMINAL poses of the listed envs, [count][H][W] each.  Needs planes
 * enabled; a pointer of a plane that is not enabled may be NULL (and is not written). */
int lcr_render_terminal_planes(lcr_sim *sim, const int32_t *env_ids_host, int count, float *depth_front, float *depth_top, uint8_t *seg_front, uint8_t *seg_top);

/* == The look of the image observations: visual domain randomisation (the reference trains policies for a real arm watched by real cameras; its envs draw one fixed world).
 * A look has two parts: a VARIANT, one of n_variants per handle, which holds everything the cached background of the frame kernel depends on -- the two observation
 * cameras, floor, sky, light, the arm's colours -- and nine per-env colour channels (cube, second cube, target marker).  Every env points at one variant; the frame kernel
 * copies untouched bands from that variant's background and ray-casts the rest with that variant's cameras and light and the env's colours.  Without lcr_enable_look every
 * frame is what it was: the default variant with the task's colours (cube 0.5 0 0, second cube 0 0 0.5, marker 0 0 1) draws the very bytes of a handle without a look.
 *   sampler  counter-based, no state of its own and none of the envs' PCG64 streams (state trajectories with and without a look are bit-identical): Philox-4x32-10, the
 *            generator of lcr_fill_random_actions, with key (seed low word, seed high word) and counter (global env id low, high, episode count of the env, block b); the
 *            blocks b = 0, 1, 2 give the words w[0 .. 11].  variant = (w[0] * n_variants) >> 32; channel j = 0 .. 8 (cube r g b, second cube r g b, marker r g b):
 *            u = (w[1 + j] >> 8) / 2^24, value = min(fma(u, hi - lo, lo), hi) in float32.  Keyed by the GLOBAL env id: every sharding of a job draws the same looks.
 *   episode  count of an env: 0 after lcr_create, + 1 on every reset of the env -- lcr_reset (masked or not) and the auto-reset of lcr_step.  With a sampler a reset
 *            redraws the look from the new count (a small kernel behind the step / reset kernel, before the frames are drawn); the look the env had is kept as its
 *            TERMINAL look, with which lcr_render_terminal / lcr_render_terminal_planes draw the episode that ended.
 *   who draws with which look: the batched frames (and planes) the env's current look; lcr_render / lcr_render_planes of env e that env's look -- cameras 0 and 1 are the
 *            variant's, camera 2 is camera_vizu unmoved with the variant's colours and light; lcr_render_state / lcr_render_state_planes keep the default look. */
#define LCR_LOOK_MAX_VARIANTS 64
typedef struct lcr_look_variant {      /* index 0 = camera_front, 1 = camera_top */
    float cam_dpos[2][3];    /* metres, world frame, added to the scene camera's position; |.| <= 0.2 per component, the camera stays >= 0.05 m above the floor */
    float cam_drot[2][3];    /* rotation vector, world frame: the camera axes X, Y, Z are rotated by |r| rad about r / |r|; 0 = none; |r| <= 0.5 */
    float fovy_deg[2];       /* 45; in [20, 90] */
    float floor_rgb[2][3];   /* checker cells: odd (0.2, 0.3, 0.4), even (0.1, 0.2, 0.3) */
    float sky_rgb[3], sky_slope[3];   /* colour = sky_rgb + a * sky_slope, a = clamp(2 * normalised d.z, 0, 1); both (0.15, 0.25, 0.35) */
    float ambient, diffuse;  /* 0.3, 0.6: floor, base, arm, cubes, marker; each in [0, 1.5] */
    float arm_rgb[3], finger_rgb[3];  /* base_link .. link_4: 0.8 grey; link_5, link_6: 0.75 grey */
} lcr_look_variant;
typedef struct lcr_look_sampler {      /* redraw an env's look whenever it is reset */
    uint64_t seed;
    float cube_lo[3], cube_hi[3], cube2_lo[3], cube2_hi[3], marker_lo[3], marker_hi[3];   /* per channel uniform in [lo, hi] within [0, 1]; lo == hi pins it */
} lcr_look_sampler;
/* Every colour lies in [0, 1] and every number is finite. */
int lcr_look_variant_default(lcr_look_variant *v);   /* the values in the comments above */
/* Switch the look on.  The arguments are checked before the handle is looked at (LCR_ERR_INVALID with the field's name in the message); then a NULL handle, a handle without
 * image observations, a moved camera less than 5 cm above the floor, a handle whose planes are already enabled (enable the look first, the planes second) and one whose observation stack is on
 * (lcr_enable_obs_stack comes last) are refused.
 * Builds the 2 n_variants cameras in fp64 (an all-zero offset gives the very floats of the scene cameras), ray-casts the n_variants cached background pairs, gives every env
 * variant 0 and its task's colours -- with a sampler the draw of episode 0 -- and redraws the frames.  Fixed for the life of the handle: a second call with the same
 * arguments does nothing, one with other arguments is refused. */
int lcr_enable_look(lcr_sim *sim, int n_variants, const lcr_look_variant *variants_host, const lcr_look_sampler *sampler_or_null);
/* The checkpoint of the look, beside lcr_get_state / lcr_set_state.  lcr_set_look: mask_host N bytes (NULL = all), variant_host / rgb_host may each be NULL (left as it is);
 * the values of the masked envs are checked (variant in [0, n_variants), colours in [0, 1]); redraws the frames as a masked lcr_reset does.  Synchronous. */
int lcr_set_look(lcr_sim *sim, const uint8_t *mask_host, const int32_t *variant_host /*[N]*/, const float *rgb_host /*[9][N]: cube, cube2, marker*/);
int lcr_get_look(lcr_sim *sim, int32_t *variant /*[N]*/, float *rgb /*[9][N]*/, uint32_t *episode /*[N]*/);   /* any may be NULL */

/* == The wrist camera: an optional third observation camera per handle, rigidly mounted on a body of the arm (or fixed in the world), drawn for every env beside
 * camera_front / camera_top at the handle's frame size -- the eye-in-hand view a visuomotor policy for this arm is normally fed; the reference's scenes have the two fixed
 * cameras only.  Off by default: without lcr_enable_wrist_camera no frame, plane, state or output of the handle changes.
 *   axes    built in fp64 on the host: X normalised; Y minus its projection on X, normalised (Gram-Schmidt, as MuJoCo does for xyaxes); Z = X x Y; then rounded to float32.
 *   pose    per env and step, from the chain of link frames that places the arm's boxes: ro = p_link + R_link pos, X_w = R_link X (likewise Y, Z); link 0: the numbers themselves.
 *   rays    s = 2 tan(fovy / 2) / H in fp64, rounded; d = sx X_w + sy Y_w - Z_w with sx, sy as the other cameras have them.
 *   scene, shading, marker blending, depth (t along the un-normalised ray) and segmentation ids (0 .. 10, bit 7 the marker): exactly those of the other cameras; the
 *           headlight is at the camera.  A box that contains the camera is not seen (t > 0).
 *   floor   seen only where the normalised d.z < -1e-6 AND ro.z > 0.  A camera at or below the floor plane -- random arm poses do put a camera on link_5 there -- sees no
 *           floor: those rays take the sky formula (a = clamp(2 normalised d.z, 0, 1): sky_rgb where they point down), segmentation 0, depth depth_far, and the floor
 *           limits no box.
 *   look    the wrist frames take the env's variant's floor, sky, light and arm colours and the env's own nine channels; the variant's camera offsets do not apply to it.
 *   order   look and wrist camera in either order, the planes last: planes enabled afterwards cover the wrist camera (depth_wrist / seg_wrist, [N][H][W]). */
typedef struct lcr_wrist_camera {
    int32_t link;      /* 0 = world frame (a fixed third camera); 1..6 = body frame of link_1..link_6 (follower.xml:56-93) */
    float pos[3];      /* metres in that frame; each |.| <= 0.5 (link 0: <= 2, and pos[2] >= 0.05) */
    float xyaxes[6];   /* MuJoCo's camera xyaxes in that frame: X then Y; the camera looks along -Z, Z = X x Y */
    float fovy_deg;    /* [20, 120] */
} lcr_wrist_camera;
typedef struct lcr_wrist_view {
    int32_t enabled;                   /* 0: no wrist camera, everything below is 0 / NULL */
    lcr_wrist_camera camera;           /* the arguments of lcr_enable_wrist_camera */
    int32_t image_width, image_height;
    float depth_far;                   /* the planes' far clip, 0 without planes */
    const uint8_t *image_wrist;        /* device, [N][H][W][3] */
    const float *depth_wrist;          /* device, [N][H][W], or NULL (plane not enabled) */
    const uint8_t *seg_wrist;          /* device, [N][H][W], or NULL */
} lcr_wrist_view;
/* Guard regions.  The wrist frames lie between two regions of LCR_WRIST_GUARD bytes, [image_wrist - LCR_WRIST_GUARD, image_wrist) and LCR_WRIST_GUARD bytes from the first 256-byte
 * boundary at or behind the frames' end; depth_wrist and seg_wrist each have LCR_WRIST_GUARD bytes before them and behind their end rounded up likewise.  The regions are filled
 * with LCR_WRIST_GUARD_BYTE when the buffers are allocated and nothing writes them afterwards: a caller (the tests do) can read them back to see that the kernels keep to their frames. */
#define LCR_WRIST_GUARD 4096
#define LCR_WRIST_GUARD_BYTE 0xA5
/* link 5, pos (0.03, 0.0033, 0.045), xyaxes (0, 1, 0, -0.4226, 0, 0.9063), fovy 60: above the gripper body, looking 25 degrees down along its -x towards the end-effector site */
int lcr_wrist_camera_default(lcr_wrist_camera *cam);
/* The checks lcr_enable_wrist_camera makes of `cam` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field's name in the message */
int lcr_wrist_camera_check(const lcr_wrist_camera *cam);
/* Switch the wrist camera on.  `cam` is checked before the handle is looked at (LCR_ERR_INVALID with the field's name in the message: link outside 0 .. 6, pos out of
 * range, a zero X or a Y parallel to X -- norm after the projection < 1e-6 --, fovy_deg outside [20, 120], a number that is not finite); then a NULL handle, a handle without
 * image observations, a handle whose planes are already enabled and one whose observation stack is on (lcr_enable_obs_stack comes last) are refused.  Allocates [N][H][W][3] and draws it from the current state; from then on whatever draws the
 * two colour frames -- step, reset and its masked no-op form, lcr_set_look -- draws the wrist frames behind them, on the same stream, from the same pose snapshot.  Fixed for
 * the life of the handle: the same arguments again do nothing, other arguments are refused. */
int lcr_enable_wrist_camera(lcr_sim *sim, const lcr_wrist_camera *cam);
/* The wrist camera's buffers; waits (on the handle's stream) for frames still being ray-cast on the second stream, as every entry point but the step does. */
int lcr_get_wrist_camera(lcr_sim *sim, lcr_wrist_view *out);
/* On a handle with a wrist camera lcr_render, lcr_render_state, lcr_render_planes and lcr_render_state_planes accept camera 3: the wrist camera of env `env`'s pose, or of
 * the given pose, at any size.  On any other handle 3 is refused.
 * The batched last wrist frames of finished episodes: the sibling of lcr_render_terminal (same precondition, same terminal look), rgb_host [count][H][W][3]; depth_host /
 * seg_host [count][H][W] may be NULL, and must be where that plane is not enabled. */
int lcr_render_terminal_wrist(lcr_sim *sim, const int32_t *env_ids_host, int count, uint8_t *rgb_host, float *depth_or_null, uint8_t *seg_or_null);

/* == The observation stack: an optional device buffer per handle, [N][K][C][H][W] contiguous, that the library keeps current -- the cameras' frames channels-first, in the
 * policy's element type, the last K of them per env.  Policy-ready as (N, K C, H, W) by a plain reshape: what SB3's VecTransposeImage + VecFrameStack or gymnasium's
 * FrameStackObservation build on the host, here on the device, behind the frame kernels, with the one rule only the library can apply without a host round trip -- which envs
 * the step has just auto-reset.  Off by default: without lcr_enable_obs_stack no byte, state, output or kernel of the handle changes.
 *   channels  C = 3 x (number of selected cameras), in the order front, top, wrist, each as r, g, b.  `cameras` is a mask of LCR_STACK_CAM_* bits; 0 = every camera the handle
 *             has.  The wrist bit on a handle without a wrist camera is refused.
 *   slots     K = frames, 1 .. LCR_STACK_MAX_FRAMES.  Slot K - 1 is the newest, slot 0 the oldest.  K = 1 is the pure transpose and cast.
 *   elements  of source byte x -- LCR_STACK_UINT8: x.  LCR_STACK_FLOAT32: (float)x * (1.0f / 255.0f), ONE correctly rounded float32 multiply by the float32 constant 1 / 255
 *             (0x3b808081), not a division: bit for bit numpy's np.float32(x) * np.float32(1 / 255).  LCR_STACK_FLOAT16: that float32 value rounded to nearest even.
 *   invariant after every entry point that draws frames, slot K - 1 of every env equals that env's current frames of the selected cameras.
 *   lcr_step  (push) slots 1 .. K - 1 move to 0 .. K - 2 and the new frames go to slot K - 1.  An env with did_reset set in that step is instead REFILLED from its new
 *             (reset-state) frames: LCR_STACK_FILL_REPEAT (default) writes them to all K slots (gymnasium's padding_type="reset"), LCR_STACK_FILL_ZERO writes zeros to
 *             slots 0 .. K - 2 and the new frames to slot K - 1 (SB3's VecFrameStack).
 *   lcr_reset masked envs are refilled (a NULL mask: all); unmasked envs have slot K - 1 rewritten and their older slots kept -- no time has passed for them.  This covers
 *             the masked no-op form (an all-zero mask redraws after lcr_set_state).
 *   lcr_set_look  slot K - 1 of every env is rewritten.      enabling: every env is refilled from its current frames.
 *   ordering  the stack kernel runs behind the frame kernels, on whatever stream they ran on.  After an lcr_step with the second stream in use it reads a SNAPSHOT of did_reset
 *             (N bytes beside the pose snapshots, two in turn): without it the step kernel of step k + 1 would overwrite the flags the stack of step k still has to read.
 *             The event every other entry point waits for is recorded after the stack kernel: every entry point but the step sees a finished stack.
 *   life      enabled last -- after look, wrist camera and planes -- and fixed for the life of the handle: the same arguments again do nothing, other arguments are refused,
 *             and lcr_enable_look / lcr_enable_wrist_camera on a handle whose stack is on are refused.  The planes are not stacked unless asked for ("The depth channel" below:
 *             lcr_enable_obs_stack_planes); without the depth channel they may be enabled before or after.
 *   guards    the stack lies between two regions of LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE, [data - LCR_WRIST_GUARD, data) and LCR_WRIST_GUARD bytes from the first
 *             256-byte boundary at or behind its end; filled once, never written afterwards.
 *   not kept  unless asked for, the stack of an episode that ended: the refill overwrites the K - 1 older frames of a reset env.  "Terminal observation stacks" below keeps
 *             them (lcr_enable_obs_stack_terminal with keep_terminal = 1) and hands out the stacked terminal observation (lcr_obs_stack_terminal). */
enum { LCR_STACK_CAM_FRONT = 1, LCR_STACK_CAM_TOP = 2, LCR_STACK_CAM_WRIST = 4 };
typedef enum lcr_obs_stack_dtype { LCR_STACK_UINT8 = 0, LCR_STACK_FLOAT16 = 1, LCR_STACK_FLOAT32 = 2 } lcr_obs_stack_dtype;
typedef enum lcr_obs_stack_fill { LCR_STACK_FILL_REPEAT = 0, LCR_STACK_FILL_ZERO = 1 } lcr_obs_stack_fill;
#define LCR_STACK_MAX_FRAMES 8
typedef struct lcr_obs_stack_spec {
    int32_t frames;       /* K, 1 .. LCR_STACK_MAX_FRAMES */
    uint32_t cameras;     /* LCR_STACK_CAM_* bits; 0 = every camera the handle has */
    int32_t dtype;        /* lcr_obs_stack_dtype */
    int32_t reset_fill;   /* lcr_obs_stack_fill */
} lcr_obs_stack_spec;
typedef struct lcr_obs_stack_view {
    int32_t enabled;                   /* 0: no stack, everything below is 0 / NULL */
    lcr_obs_stack_spec spec;           /* as enabled, `cameras` resolved to the bits in use */
    int32_t channels;                  /* C */
    int32_t image_width, image_height;
    const void *data;                  /* device, [N][K][C][H][W] of the element type */
    uint64_t bytes_per_env;            /* K C H W sizeof(element) */
} lcr_obs_stack_view;
/* The checks lcr_enable_obs_stack makes of `spec` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field's name in the message */
int lcr_obs_stack_check(const lcr_obs_stack_spec *spec);
/* Switch the stack on.  `spec` is checked first; then a NULL handle, a handle without image observations and a wrist bit without a wrist camera are refused (LCR_ERR_INVALID);
 * an allocation that fails is LCR_ERR_OOM.  Refills every env from its current frames. */
int lcr_enable_obs_stack(lcr_sim *sim, const lcr_obs_stack_spec *spec);
/* The stack; waits (on the handle's stream) for frames and stack still being made on the second stream, as every entry point but the step does. */
int lcr_get_obs_stack(lcr_sim *sim, lcr_obs_stack_view *out);

/* == Terminal observation stacks: the stack of an episode that has ended, for the consumers that owe SB3 / gymnasium a complete terminal_observation / final_obs, and for an
 * on-device loop that bootstraps the value of a truncated episode.  The sibling of lcr_render_terminal for the stack.  Off unless asked for: a handle enabled with
 * lcr_enable_obs_stack, or with keep_terminal = 0, launches the stack kernel it always launched and produces its bytes.
 *   definition  env e was reset by the last lcr_step; before that step its slots 0 .. K - 1 held o(t-K+1) .. o(t).  Its terminal stack is [slots 1 .. K - 1 as they were before
 *               that step's stack kernel ran, the terminal frame], newest last.  The terminal frame is what lcr_render_terminal (and lcr_render_terminal_wrist) draw for e,
 *               of the stack's selected cameras, through the stack's element rule.  An episode shorter than K - 1 steps still shows its reset fill (repeat or zeros) in the
 *               older slots -- what gymnasium's FrameStackObservation and SB3's VecFrameStack hold at that point.
 *   history     with keep_terminal = 1 and K > 1 a device buffer [N][K - 1][C][H][W] of the element type, zero-filled when it is allocated.  The stack kernel of lcr_step, in
 *               the build this mode launches, copies slots 1 .. K - 1 of every env whose did_reset is set to history[e] before it refills them (on the second stream it
 *               reads the did_reset snapshot it already reads).  ONLY step refills save: the refills of lcr_reset, the rewrites of lcr_set_look and enabling leave the
 *               history alone, and the history of an env stands until that env's next step reset.  K = 1 keeps nothing: the terminal stack is the terminal frame.
 *   guards      the history lies behind the stack's second guard region, and LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE follow the first 256-byte boundary at or behind its
 *               end; filled once, never written afterwards.
 *   life        as the spec: the same spec and the same keep_terminal again do nothing, anything else is refused.
 *   not kept    terminal history of the depth and segmentation planes (but for the depth channel of a stack enabled with it, below); device-side outputs of the terminal
 *               calls. */
/* lcr_enable_obs_stack with the choice to keep terminal stacks; lcr_enable_obs_stack(sim, spec) is this call with keep_terminal = 0.  `spec` is checked first, then
 * keep_terminal (0 or 1: LCR_ERR_INVALID naming it), then the handle. */
int lcr_enable_obs_stack_terminal(lcr_sim *sim, const lcr_obs_stack_spec *spec, int32_t keep_terminal);
/* Whether terminal stacks are kept (*keep_terminal 1 / 0), the history (device, [N][K - 1][C][H][W]; NULL with K = 1 or without keep_terminal) and its bytes per env; joins
 * as lcr_get_obs_stack does. */
int lcr_get_obs_stack_terminal(lcr_sim *sim, int32_t *keep_terminal, const void **history, uint64_t *history_bytes_per_env);
/* The terminal stacks of the listed envs, out_host [count][K][C][H][W] of the element type.  Synchronous; joins first.  Env ids are checked against the handle's range, and
 * the precondition is that of lcr_render_terminal: every listed env was reset by the LAST lcr_step (the terminal poses, the terminal looks and the history belong to that
 * step).  Refused (LCR_ERR_INVALID, naming which) on a handle without a stack and on one whose stack was enabled without keep_terminal.  count = 0 is LCR_OK.  The terminal
 * frames are drawn and the stacks assembled in device staging, in as many passes as keep the staging -- per env the terminal frames of front, top and (if stacked) wrist and the
 * terminal stack -- within the 450 MiB a pass of the terminal-frame calls takes. */
int lcr_obs_stack_terminal(lcr_sim *sim, const int32_t *env_ids_host, int count, void *out_host);

/* == The depth channel of the observation stack: RGB-D for a convolutional policy.  Off unless asked for: a handle enabled with lcr_enable_obs_stack or
 * lcr_enable_obs_stack_terminal, or with planes = 0, launches the stack kernel it always launched and produces its bytes.
 *   channels    a stack enabled with the depth plane has C = 4 x (number of selected cameras) channels.  The cameras keep the order front, top, wrist; each contributes
 *               r, g, b, d.
 *   the same    slots, push, refill (repeat / zero), lcr_reset, lcr_set_look, enabling, ordering on the second stream, guards and life are word for word those of the colour
 *               stack: the depth channel is one more channel that moves with the others.  A zero refill writes zero bits to the depth channel too.  The colour channels of a
 *               depth stack follow the existing rule unchanged.
 *   elements    d is the float32 of the depth plane: metres along the optical axis, already clipped to [0, depth_far] by the frame kernel.  Two float32 constants are fixed
 *               when the stack is enabled, inv_far = (float)(1.0 / (double)depth_far) and s255 = (float)(255.0 / (double)depth_far).
 *               LCR_STACK_FLOAT32: fminf(d * inv_far, 1.0f) -- ONE rounded float32 multiply, then the clamp.  LCR_STACK_FLOAT16: that float32 value rounded to nearest even.
 *               LCR_STACK_UINT8: min((int)fmaf(d, s255, 0.5f), 255) -- ONE fused multiply-add, truncation toward zero, then the clamp.  Nothing in these chains is
 *               re-associated or contracted differently by the build's fast-math flags: they are pinned as the crop box's point chain is.
 *   enabling    the depth channel is made of the depth plane, which is not switched on silently: with the depth bit the planes must be enabled BEFORE the stack, and a handle
 *               whose depth plane is not enabled is refused by name.  depth_far is then fixed: a later lcr_enable_image_planes with another depth_far is refused.
 *   terminal    with keep_terminal = 1 the history is [N][K - 1][4 ncam][H][W] and carries the depth channel; lcr_obs_stack_terminal returns [count][K][4 ncam][H][W], its
 *               staging additionally holds the terminal depth planes of the selected cameras, drawn the way lcr_render_terminal_planes / lcr_render_terminal_wrist draw
 *               them: same poses, same terminal looks.
 *   not in it   a segmentation channel (ids are categorical: a cast of them is not policy-ready); normalisation by mean and std; a depth-only stack without colours;
 *               per-camera depth_far; the recorder. */
/* lcr_enable_obs_stack_terminal with the choice of planes: `planes` is a mask of the LCR_PLANE_* bits lcr_enable_image_planes uses.  planes = 0 is exactly
 * lcr_enable_obs_stack_terminal; LCR_PLANE_DEPTH asks for the RGB-D stack; LCR_PLANE_SEGMENTATION is LCR_ERR_UNSUPPORTED, named in the message; unknown bits are
 * LCR_ERR_INVALID.  `spec` is checked first, then keep_terminal, then planes, then the handle: a handle whose depth plane is not enabled is refused by name (LCR_ERR_INVALID),
 * and so is a stack enabled already with another mask. */
int lcr_enable_obs_stack_planes(lcr_sim *sim, const lcr_obs_stack_spec *spec, int32_t keep_terminal, uint32_t planes);
/* The mask in use and the two constants of the depth element as the float32 values in use; 0, 0, 0 without a depth channel.  Joins as lcr_get_obs_stack does. */
int lcr_get_obs_stack_planes(lcr_sim *sim, uint32_t *planes, float *inv_far, float *s255);

/* == The point cloud: an optional device buffer per handle, `points` [N][P][C] float32, that the library keeps current behind the frame kernels -- a fixed number of
 * world-frame points per env, fused over the cameras, floor and sky dropped: the input of a PointNet-style encoder or a 3-D diffusion policy.  Everything it is made of
 * lies in device memory after the frame kernels (depth along a known ray, surface ids, colours, the cameras); the kernel compacts a variable number of surface pixels per
 * env to a fixed count and unprojects them with the cameras that drew them, in stream order, without a host round trip.  Off by default: without
 * lcr_enable_point_cloud no byte, state, output or kernel of the handle changes.
 *   cameras     a mask of LCR_STACK_CAM_* bits; 0 = every camera the handle has.  Camera SLOTS are the selected cameras in the order front, top, wrist.  The wrist bit on
 *               a handle without a wrist camera is refused.
 *   candidates  a pixel of a selected camera whose segmentation byte has id = byte & 0x7f with bit `id` set in `ids` (the marker bit 7 is ignored).  `ids` is a mask over
 *               the ids 1 .. 10; 0 means 0x7FC: the arm's seven boxes and the cubes, without the floor.  Bit 0 (sky: no surface) and bits above 10 are refused.
 *               Candidates are numbered 0 .. M - 1 by camera slot, then row-major pixel.
 *   selection   deterministic, one rule for every M: output point j (0 <= j < P) is candidate ((2 j + 1) M) / (2 P), an integer division in 64 bits (the product exceeds
 *               2^32).  M >= P: an even stride through the candidates; 0 < M < P: candidates repeat monotonically, each at least floor(P / M) times; M = 0: zeros in
 *               all of the env's points and -1 in its sources.
 *   point       of a candidate at (row, px) of a camera with position ro, world axes X, Y, Z and ray scale s: the ray of the planes section, d = sx X + sy Y - Z with
 *               sx, sy exactly as the colour and plane kernels form them; p = ro + t d with t the float32 depth plane value, in the WORLD frame.  A surface beyond
 *               depth_far sits at depth_far along its ray: documented, not filtered (the default 10 m is beyond every scene).
 *   channels    C = 3: x y z.  C = 6 (colors = 1): x y z r g b, the colours from the colour frame as (float)x * (1.0f / 255.0f), the stack's float32 rule, bit for bit.
 *   count       [N] int32: M.
 *   source      [N][P] int32: slot H W + row W + px of the chosen candidate, or -1.  A policy can gather per-pixel features with it.
 *   camera_pose [slots][13][N] float32: ro, X, Y, Z, s of every slot per env as the kernel used them -- the cloud's extrinsics, which a caller who fuses views needs as
 *               well.  Front and top are the handle's cameras or the env's look variant's; the wrist pose comes from the link chain of the same pose snapshot the wrist
 *               frames were drawn from, computed by the device code the wrist kernel uses.
 *   P           `points`: a multiple of 64 in 64 .. 8192.
 *   invariant   after every entry point that draws the batched frames -- lcr_step, lcr_reset with its masked and no-op forms, lcr_set_look, enabling -- cloud, count,
 *               source and pose are the function above of that env's current frames, planes and cameras.  No history and no reset rule: an auto-reset env shows its reset
 *               state, as its frames do.
 *   ordering    the cloud kernel runs behind the frame kernels (and the stack kernel, if there is one) on whatever stream they ran on; the event the joining entry points
 *               wait for is recorded after it.  After a step on the second stream it reads the look snapshot and the pose snapshot the frames used.
 *   life        needs image observations and BOTH planes; since look and wrist camera refuse to come after the planes, the cloud is enabled after all three, before or
 *               after the observation stack.  Fixed for the life of the handle: the same spec again does nothing, another spec is refused.
 *   memory      one allocation: LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE, points, the same guard from the first 256-byte boundary at or behind their end (as the
 *               stack has them), then count, source and camera_pose.  Freed by lcr_destroy.
 *   not in it   random sampling, normals, a base-frame transform.  Not KEPT either, and it need not be, is the cloud of an episode that has ended: lcr_point_cloud_terminal
 *               ("The point cloud of the terminal observation" below) makes it from the terminal frames.  (Farthest-point sampling from a strided pool and a crop box
 *               are optional modes of their own: "The point cloud by farthest-point sampling" and "The point cloud inside a crop box" below.) */
typedef struct lcr_point_cloud_spec {
    int32_t points;       /* P: a multiple of 64 in 64 .. 8192 */
    uint32_t cameras;     /* LCR_STACK_CAM_* bits; 0 = every camera the handle has */
    uint32_t ids;         /* bit i: surface id i is a candidate, i = 1 .. 10; 0 = 0x7FC (arm and cubes) */
    int32_t colors;       /* 0: C = 3 (x y z); 1: C = 6 (x y z r g b) */
} lcr_point_cloud_spec;
typedef struct lcr_point_cloud_view {
    int32_t enabled;                   /* 0: no cloud, everything below is 0 / NULL */
    lcr_point_cloud_spec spec;         /* as enabled, `cameras` and `ids` resolved to the bits in use */
    int32_t channels, slots, image_width, image_height;
    const float *points;               /* device, [N][P][C] */
    const int32_t *count;              /* device, [N] */
    const int32_t *source;             /* device, [N][P] */
    const float *camera_pose;          /* device, [slots][13][N] */
    uint64_t bytes_per_env;            /* P C sizeof(float) */
} lcr_point_cloud_view;
#define LCR_CLOUD_DEFAULT_IDS 0x7FCu
/* The checks lcr_enable_point_cloud makes of `spec` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field's name in the message */
int lcr_point_cloud_check(const lcr_point_cloud_spec *spec);
/* Switch the cloud on.  `spec` is checked first; then a NULL handle, a handle without image observations, one without both planes and a wrist bit without a wrist camera
 * are refused (LCR_ERR_INVALID, naming what is missing); an allocation that fails is LCR_ERR_OOM.  Makes the cloud of the current frames. */
int lcr_enable_point_cloud(lcr_sim *sim, const lcr_point_cloud_spec *spec);
/* The cloud; waits (on the handle's stream) for frames and cloud still being made on the second stream, as every entry point but the step does. */
int lcr_get_point_cloud(lcr_sim *sim, lcr_point_cloud_view *out);

/* == The point cloud by farthest-point sampling (FPS): an optional sampling mode of the point cloud.  The strided selection above is even in image space, not in 3-D: a
 * surface near a camera takes most of the points.  PointNet-style encoders and 3-D diffusion policies down-sample with FPS instead; this mode does it on the device, in
 * the cloud's kernel: FPS of P points out of a POOL of Q candidates, the pool chosen by the strided rule.  Off unless asked for: a handle enabled with
 * lcr_enable_point_cloud, or with LCR_CLOUD_SAMPLE_STRIDE, launches the strided kernel and produces its bytes.
 *   pool        Q = `pool`: a multiple of 64 with P <= Q <= LCR_CLOUD_MAX_POOL (4096), which caps P at 4096 under FPS as well.  No default: the caller chooses the cost,
 *               N P Q distance updates per cloud.  Pool entry i (0 <= i < Q) is candidate ((2 i + 1) M) / (2 Q), the selection rule above with Q in place of P, in
 *               64 bits.  Its point is the point formula above, evaluated as the strided kernel evaluates it: p = ro + t d by the same fmaf chain, r g b by the stack's
 *               rule with colors = 1.  If 0 < M < Q, candidates repeat in the pool, as they do in a strided cloud.
 *   order       greedy.  Every pool entry has a float32 `mind`, initially + inf.  For k = 0 .. P - 1: output point k is the pool entry with the largest mind, ties to the
 *               LOWEST pool index -- the first point is pool entry 0; the pool is monotone in the candidate number, so among distinct tied candidates the one with the
 *               lowest source wins.  The chosen entry's mind is set to - 1: it is never chosen again.  Every other entry i with mind[i] >= 0 takes
 *               mind[i] = min(mind[i], dist(i, chosen)).
 *   distance    pinned to the bit: dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, one float32 subtraction each; dist = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) -- one
 *               rounded multiply, then two fused steps, in that order.  Nothing is re-associated or contracted beyond the two fmaf, denormals are kept.  Only x y z enter
 *               the distance, colours never do.
 *   output      points[env][k] and source[env][k], in greedy order: the first k points of the buffer are themselves an FPS of k points from the same pool, so a consumer
 *               may truncate.  count is M, camera_pose is as above.
 *   M = 0       the env's points are zeros and its sources - 1, as above.      0 < M < P: after the M distinct candidates the remaining outputs are duplicates at
 *               distance 0, taken in pool order.
 *   the rest    invariant, ordering (behind the frame and stack kernels, the look and pose snapshots on the second stream, the join event), guards, memory and life are
 *               those of the point cloud above, word for word.
 *   not in it   random sampling, normals, pools beyond 4096, FPS over colours.  (A crop box was left out of this mode at first: a float32 comparison at the box faces
 *               decides what a candidate is, so count and source are exact decisions only if the point itself is pinned to the bit, as the distance above is.  "The
 *               point cloud inside a crop box" below does that; it combines with this mode.) */
enum { LCR_CLOUD_SAMPLE_STRIDE = 0, LCR_CLOUD_SAMPLE_FPS = 1 };
#define LCR_CLOUD_MAX_POOL 4096
typedef struct lcr_point_cloud_sampling {
    int32_t mode;         /* LCR_CLOUD_SAMPLE_* */
    int32_t pool;         /* Q under LCR_CLOUD_SAMPLE_FPS: a multiple of 64, points <= pool <= LCR_CLOUD_MAX_POOL; under LCR_CLOUD_SAMPLE_STRIDE it must be 0 */
} lcr_point_cloud_sampling;
/* The checks lcr_enable_point_cloud_sampled makes of `sampling` (against an already checked `spec`) before it looks at the handle, on their own: LCR_OK, or
 * LCR_ERR_INVALID with the field's name first in the message */
int lcr_point_cloud_sampling_check(const lcr_point_cloud_spec *spec, const lcr_point_cloud_sampling *sampling);
/* lcr_enable_point_cloud with a sampling mode; a NULL sampling is LCR_CLOUD_SAMPLE_STRIDE, and lcr_enable_point_cloud(sim, spec) is this call with NULL.  `spec` is checked
 * first, then `sampling`, then the handle.  Fixed for the life of the handle: the same spec and the same sampling again do nothing; if either differs the call is refused. */
int lcr_enable_point_cloud_sampled(lcr_sim *sim, const lcr_point_cloud_spec *spec, const lcr_point_cloud_sampling *sampling_or_null);
/* The sampling of the handle's cloud (mode LCR_CLOUD_SAMPLE_STRIDE and pool 0 for a strided cloud and for a handle without a cloud); joins as lcr_get_point_cloud does. */
int lcr_get_point_cloud_sampling(lcr_sim *sim, lcr_point_cloud_sampling *out);

/* == The point cloud inside a crop box: an optional axis-aligned box in the WORLD frame, lo[3] and hi[3], float32.  The selection to a fixed P (the strided rule) or to a
 * pool of Q (FPS) happens inside the cloud's kernel: a point outside the workspace has taken a slot that a workspace point should have had, and no consumer can give it
 * back.  PointNet-style encoders and 3-D diffusion policies crop to the workspace first and down-sample second; this mode does the same, on the device, in the cloud's
 * kernel.  Off unless asked for: a handle enabled without a crop launches the kernels it launched before, and produces their bytes.
 *   candidates  a pixel is a candidate if it is one by the id rule of the point cloud above AND its point, below, lies inside the box.  Candidates are numbered as there
 *               (camera slot, then row-major pixel).  M, count, the strided selection ((2 j + 1) M) / (2 P), the FPS pool ((2 i + 1) M) / (2 Q), source, the M = 0 and
 *               0 < M < P rules, camera_pose, colours, guards, memory, ordering (the second stream and its snapshots, the join event), invariant and life are those of the
 *               two sections above, word for word, with "candidate" meaning this.
 *   point       pinned to the bit in this mode.  Of the pixel (row, px) of a W x H frame, t its float32 depth plane value, ro, X, Y, Z, s the float32 values written to
 *               camera_pose:  hx = (float)px + 0.5f - 0.5f * (float)W, an exact half-integer;  sx = hx * s, one rounded float32 multiply;
 *               hy = (float)row + 0.5f - 0.5f * (float)H;  sy = - (hy * s);  and per axis k = x, y, z:  d_k = fmaf(sx, X_k, fmaf(sy, Y_k, - Z_k)),
 *               p_k = fmaf(t, d_k, ro_k).  This is the expression of the point cloud above; here nothing is re-associated or contracted beyond the fmaf named, and
 *               denormals are kept.
 *   inside      lo_k <= p_k && p_k <= hi_k for all three k: float32 comparisons on those bits.  Both faces belong to the box.
 *   output      the x y z of a cropped cloud ARE these p_k: every point of an env with M > 0 satisfies the inside test exactly.  Under FPS the pool points, and so the
 *               points that go out, are these bits too; the distance rule is unchanged.  count, source and, in this mode, x y z are reproducible decisions: a model that
 *               evaluates the chain above with an exact fused multiply-add gets the same bits.
 *   the box     each of the six numbers is finite or an infinity: lo_k = - inf or hi_k = + inf is an open side.  NaN is refused; lo_k > hi_k is refused, naming the axis;
 *               lo_k == hi_k is allowed (it usually gives M = 0).  One box per handle, fixed for its life, like spec and sampling.
 *   depth_far   a surface beyond depth_far sits at depth_far along its ray, as above, and the box then drops it.
 *   not in it   oriented or per-env boxes, several boxes, a base-frame transform, normals, random sampling. */
typedef struct lcr_point_cloud_crop {
    float lo[3];          /* x, y, z of the lower corner, world frame; - inf: open */
    float hi[3];          /* x, y, z of the upper corner; + inf: open */
} lcr_point_cloud_crop;
/* The checks lcr_enable_point_cloud_cropped makes of `crop` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field and the axis in the
 * message */
int lcr_point_cloud_crop_check(const lcr_point_cloud_crop *crop);
/* lcr_enable_point_cloud_sampled with a crop box; a NULL crop is no box, and lcr_enable_point_cloud_sampled(sim, spec, sampling) is this call with a NULL crop.  `spec` is
 * checked first, then `sampling`, then `crop`, then the handle.  Fixed for the life of the handle: the same spec, sampling and crop again do nothing; if any differs -- a box
 * on a handle enabled without one and the reverse included -- the call is refused, and the message names what is enabled and what was asked for, boxes included. */
int lcr_enable_point_cloud_cropped(lcr_sim *sim, const lcr_point_cloud_spec *spec, const lcr_point_cloud_sampling *sampling_or_null,
                                   const lcr_point_cloud_crop *crop_or_null);
/* The crop box of the handle's cloud: *enabled = 1 and the box in use, or *enabled = 0 and zeros for a cloud without a box and for a handle without a cloud; joins as
 * lcr_get_point_cloud does. */
int lcr_get_point_cloud_crop(lcr_sim *sim, int32_t *enabled, lcr_point_cloud_crop *out);

/* == The point cloud of the terminal observation: the sibling of lcr_render_terminal for the cloud.  It needs no state and no enabling step: per pass of the listed envs the
 * library gathers their terminal poses and terminal looks, draws their terminal colour frames, both planes and -- if the cloud selects it -- the wrist camera's into device
 * staging, and launches the handle's OWN cloud kernel (strided, farthest-point or cropped, with the handle's pool and box) over that view, with the wrist pose from the
 * terminal joint angles.  The result is therefore, by construction, the function the three sections above define for the cloud, applied to the terminal frames, planes and
 * cameras: what lcr_render_terminal, lcr_render_terminal_planes and lcr_render_terminal_wrist return for the same envs, and the cameras in `pose_host`.
 *   outputs     points_host [count][P][C], count_host [count], source_host [count][P], pose_host [slots][13][count]; any of them may be NULL.
 *   the rest    synchronous, joins first; env ids are checked against the handle's range; the precondition is that of lcr_render_terminal (every listed env was reset by the
 *               LAST lcr_step).  A handle without a point cloud is refused (LCR_ERR_INVALID).  count = 0 is LCR_OK.  Nothing of the live cloud is touched. */
int lcr_point_cloud_terminal(lcr_sim *sim, const int32_t *env_ids_host, int count, float *points_host, int32_t *count_host, int32_t *source_host, float *pose_host);

/* == The voxel grid: an optional device buffer per handle, `voxels` [N][C][Dz][Dy][Dx], that the library keeps current behind the frame kernels -- occupancy (and colour) over a
 * fixed axis-aligned box of the WORLD frame, fused over the cameras: the dense input of a voxel policy (PerAct, C2F-ARM, 3-D conv encoders), fed straight to a Conv3d as
 * (N, C, D, H, W).  It is made of ALL candidate pixels, not of the P a point cloud keeps, by one streaming kernel, in stream order, without a host round trip.  Off by
 * default: without lcr_enable_voxel_grid no byte, state, output or kernel of the handle changes.
 *   inputs      those of the point cloud: the image observations at the configured size, both planes, the selected camera slots (`cameras`: LCR_STACK_CAM_* bits, 0 = every
 *               camera the handle has; slots in the order front, top, wrist; the wrist bit on a handle without a wrist camera is refused), `ids` (a mask over the ids 1 .. 10,
 *               0 = 0x7FC, bit 0 and bits above 10 refused), the cameras of the handle or of the env's look variant, the wrist pose from the pose snapshot.
 *   candidate   a pixel that is a candidate by the id rule of the point cloud (id = byte & 0x7f, bit `id` set in `ids`; the marker bit 7 is ignored).
 *   pixel index g = slot H W + row W + px: the global pixel index, the `source` numbering of the cloud.
 *   point       the pinned chain of "The point cloud inside a crop box", word for word: hx = (float)px + 0.5f - 0.5f * (float)W;  sx = hx * s, one rounded float32 multiply;
 *               hy = (float)row + 0.5f - 0.5f * (float)H;  sy = - (hy * s);  per axis k:  d_k = fmaf(sx, X_k, fmaf(sy, Y_k, - Z_k)),  p_k = fmaf(t, d_k, ro_k) -- with t the
 *               float32 depth plane value and ro, X, Y, Z, s the float32 values the kernel writes to a camera_pose buffer of the grid's own, [slots][13][N].  Nothing is
 *               re-associated or contracted beyond the fmaf named, denormals are kept.
 *   box, cells  lo[3], hi[3]: float32, FINITE, lo_k < hi_k -- unlike the crop box there are no open sides.  dims = (Dx, Dy, Dz), each in 1 .. 64, Dx a multiple of 4,
 *               V = Dx Dy Dz <= LCR_VOXEL_MAX_CELLS (32 768).  The library forms inv_k = (float)((double)D_k / ((double)hi_k - (double)lo_k)) once, on the host, and REPORTS
 *               the three float32 values in the view (inv_cell): the reported values are the authority for everything below.
 *   voxel       of a candidate, per axis k:  u_k = p_k - lo_k, one float32 subtraction;  v_k = u_k * inv_k, one rounded float32 multiply.  The candidate is inside iff
 *               u_k >= 0.0f && v_k < (float)D_k on all three axes (u = - 0.0 is inside, in cell 0); then i_k = (int)v_k.  Both operations are opaque to the optimiser.  The
 *               box is half-open UP TO THIS ROUNDING: a point a rounding below hi_k whose v_k rounds to D_k is outside, and no face of hi is promised either way.
 *   grid        voxel (ix, iy, iz) is OCCUPIED iff some candidate falls in it; its SOURCE is the smallest g among them -- front wins over top over wrist, then row-major.  An
 *               order-independent minimum: the grid is deterministic whatever the order lanes arrive in.
 *   voxels      [N][C][Dz][Dy][Dx]: z is the depth axis, y the height, x the width of a Conv3d input.  Channel 0: occupancy, source byte 255 or 0.  With LCR_VOXEL_RGB in
 *               `features`: channels 1 .. 3, the colour-frame bytes of the source pixel, 0 where empty.  Elements: LCR_STACK_UINT8 the source byte x, LCR_STACK_FLOAT32
 *               (float)x * (1.0f / 255.0f), the stack's element rule, bit for bit (LCR_STACK_FLOAT16 is refused).
 *   source      optional (`source` = 1), [N][Dz][Dy][Dx] int32: the voxel's source g, - 1 where empty.  Off by default: it is 4 V bytes per env.
 *   count       [N] int32, always: candidates inside the grid.        occupied  [N] int32, always: occupied voxels.
 *   camera_pose [slots][13][N] float32, always: ro, X, Y, Z, s of every slot per env as the kernel used them, as the cloud reports them.
 *   invariant   after every entry point that draws the batched frames -- lcr_step, lcr_reset with its masked and no-op forms, lcr_set_look, enabling -- the grid is the
 *               function above of that env's current frames, planes and cameras.  No history and no reset rule: an auto-reset env shows its reset state, as its frames do.
 *   ordering    the grid kernel runs behind the frame kernels, the stack kernel and the cloud kernel, on whatever stream they ran on; the event the joining entry points wait
 *               for is recorded after it.  After a step on the second stream it reads the look snapshot and the pose snapshot the frames used.
 *   life        needs image observations and BOTH planes; independent of the point cloud: either, both or neither.  Fixed for the life of the handle: the same spec again
 *               does nothing, another spec is refused, naming both.
 *   memory      one allocation: LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE, voxels, the same guard from the first 256-byte boundary at or behind their end (as the
 *               cloud and the stack have them), then source, count, occupied and camera_pose.  Freed by lcr_destroy; LCR_ERR_OOM if it fails.  N V C sizeof(element) grows
 *               fast: 32 768 envs of 32 x 32 x 32 with colours are 4 GiB as uint8 and 16 GiB as float32, and `source` adds 4 GiB.
 *   not in it   mean colours and per-voxel counts, oriented or per-env boxes, float16, the recorder, and the grid of an episode that has ended: there is no _terminal call, so
 *               the vector adapters refuse the grid.
 * LCR_VOXEL_LDS=slab|big in the environment (read by lcr_enable_voxel_grid): how the kernel holds a grid of more than 16 384 voxels, a word a voxel in LDS -- in passes over
 * the planes of one z-slab each (the default), or whole, in a build with 128 KiB of LDS; the same bytes under both (an A/B switch: profiles/voxel_grid.txt). */
enum { LCR_VOXEL_OCCUPANCY = 1, LCR_VOXEL_RGB = 2 };
#define LCR_VOXEL_MAX_DIM 64
#define LCR_VOXEL_MAX_CELLS 32768
typedef struct lcr_voxel_grid_spec {
    float lo[3];          /* x, y, z of the box's lower corner, world frame; finite */
    float hi[3];          /* x, y, z of the upper corner; finite, lo[k] < hi[k] */
    int32_t dims[3];      /* Dx, Dy, Dz: each 1 .. LCR_VOXEL_MAX_DIM, Dx a multiple of 4, Dx Dy Dz <= LCR_VOXEL_MAX_CELLS */
    uint32_t cameras;     /* LCR_STACK_CAM_* bits; 0 = every camera the handle has */
    uint32_t ids;         /* bit i: surface id i is a candidate, i = 1 .. 10; 0 = 0x7FC (arm and cubes) */
    uint32_t features;    /* LCR_VOXEL_* bits; occupancy is implied, 0 = occupancy only */
    int32_t dtype;        /* LCR_STACK_UINT8 or LCR_STACK_FLOAT32 */
    int32_t source;       /* 0 | 1: keep the source index of every voxel */
} lcr_voxel_grid_spec;
typedef struct lcr_voxel_grid_view {
    int32_t enabled;                   /* 0: no grid, everything below is 0 / NULL */
    lcr_voxel_grid_spec spec;          /* as enabled: `cameras` and `ids` resolved to the bits in use, the occupancy bit set in `features` */
    float inv_cell[3];                 /* inv_k: cells per metre along x, y, z, the float32 values the kernel multiplies with */
    int32_t channels, slots, image_width, image_height;
    const void *voxels;                /* device, [N][C][Dz][Dy][Dx] of the element type */
    const int32_t *source;             /* device, [N][Dz][Dy][Dx], or NULL */
    const int32_t *count;              /* device, [N] */
    const int32_t *occupied;           /* device, [N] */
    const float *camera_pose;          /* device, [slots][13][N] */
    uint64_t bytes_per_env;            /* C Dz Dy Dx sizeof(element) */
} lcr_voxel_grid_view;
/* The checks lcr_enable_voxel_grid makes of `spec` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field and the axis in the message -- a
 * corner that is NaN or an infinity, lo_k >= hi_k, a dim outside 1 .. 64, Dx not a multiple of 4, more than LCR_VOXEL_MAX_CELLS voxels, unknown feature bits, a dtype
 * other than uint8 / float32, source other than 0 / 1, and the cloud's refusals of `cameras` and `ids` */
int lcr_voxel_grid_check(const lcr_voxel_grid_spec *spec);
/* Switch the grid on.  `spec` is checked first; then a NULL handle, a handle without image observations, one without both planes and a wrist bit without a wrist camera are
 * refused (LCR_ERR_INVALID, naming what is missing); an allocation that fails is LCR_ERR_OOM.  Makes the grid of the current frames. */
int lcr_enable_voxel_grid(lcr_sim *sim, const lcr_voxel_grid_spec *spec);
/* The grid; waits (on the handle's stream) for frames and grid still being made on the second stream, as every entry point but the step does. */
int lcr_get_voxel_grid(lcr_sim *sim, lcr_voxel_grid_view *out);

/* == The heightmap: an optional device buffer per handle, `heightmap` [N][C][Hy][Hx] float32, that the library keeps current behind the frame kernels -- an orthographic
 * top-down map over a fixed axis-aligned box of the WORLD frame, fused over the cameras: channel 0 is the height of the highest surface above every cell of the table and,
 * with LCR_HEIGHTMAP_RGB, channels 1 .. 3 its colour -- the input of Transporter-Nets / CLIPort-style "where to push, where to grasp" policies, fed straight to a Conv2d as
 * (N, C, H, W).  It is made of ALL candidate pixels by one streaming kernel, in stream order, without a host round trip; unlike the voxel grid its height is not quantised
 * to layers and it costs N Hx Hy elements, not N V.  Off by default: without lcr_enable_heightmap no byte, state, output or kernel of the handle changes.
 *   inputs      those of the voxel grid: the image observations at the configured size, both planes, the selected camera slots (`cameras`: LCR_STACK_CAM_* bits, 0 = every
 *               camera the handle has; slots in the order front, top, wrist; the wrist bit on a handle without a wrist camera is refused), `ids` (a mask over the ids 1 .. 10,
 *               0 = 0x7FC, bit 0 and bits above 10 refused), the cameras of the handle or of the env's look variant, the wrist pose from the pose snapshot.
 *   candidate   a pixel that is a candidate by the id rule of the point cloud (id = byte & 0x7f, bit `id` set in `ids`; the marker bit 7 is ignored).
 *   pixel index g = slot H W + row W + px: the global pixel index, the `source` numbering of the cloud.
 *   point       the pinned chain of "The voxel grid", word for word: hx = (float)px + 0.5f - 0.5f * (float)W;  sx = hx * s, one rounded float32 multiply;
 *               hy = (float)row + 0.5f - 0.5f * (float)H;  sy = - (hy * s);  per axis k:  d_k = fmaf(sx, X_k, fmaf(sy, Y_k, - Z_k)),  p_k = fmaf(t, d_k, ro_k) -- with t the
 *               float32 depth plane value and ro, X, Y, Z, s the float32 values the kernel writes to a camera_pose buffer of the map's own, [slots][13][N].  Nothing is
 *               re-associated or contracted beyond the fmaf named, denormals are kept.
 *   box, dims   lo[3], hi[3]: float32, FINITE, lo_k < hi_k.  dims = (Hx, Hy), each in 1 .. 256, Hx a multiple of 4, Hx Hy <= LCR_HEIGHTMAP_MAX_CELLS (16 384).  The
 *               library forms inv_k = (float)((double)H_k / ((double)hi_k - (double)lo_k)) for k = x, y once, on the host, and REPORTS the two float32 values in the view
 *               (inv_cell): the reported values are the authority for everything below.
 *   cell        of a candidate, per axis k = x, y, the grid's axis rule:  u_k = p_k - lo_k, one float32 subtraction;  v_k = u_k * inv_k, one rounded float32 multiply.  The
 *               candidate is inside along k iff u_k >= 0.0f && v_k < (float)H_k (u = - 0.0 is inside, in cell 0); then i_k = (int)v_k.  Both operations are opaque to the
 *               optimiser.  Along x and y the box is half-open UP TO THIS ROUNDING, as the grid's is: a point a rounding below hi_k whose v_k rounds to H_k is outside.
 *   height      u_z = p_z - lo_z, one float32 subtraction, opaque to the optimiser.  The candidate is inside along z iff u_z >= 0.0f && p_z <= hi_z: BOTH faces belong to the
 *               box, as they belong to the crop box.  The height word hb is the bit pattern of u_z with the sign bit cleared: - 0.0 - (+ 0.0) is - 0.0, which passes the
 *               test, and its height is + 0.0.  For u_z >= 0 the words order as the heights do.
 *   key, map    every inside candidate has the 64-bit key ((uint64)hb << 32) | (0xFFFFFFFF - g).  A cell's value is the MAXIMUM key among its candidates: the highest
 *               point, and among points of bit-equal height the smallest g -- front wins over top over wrist, then row-major.  An order-independent maximum: the map is
 *               deterministic whatever the order lanes arrive in.  A cell without candidates is EMPTY, key 0; no candidate has key 0, since g < 2^32 - 1.
 *   heightmap   [N][C][Hy][Hx] float32: x is the fastest axis; row iy is the cell row at lo_y + iy cell_y along + y of the world frame.  Channel 0: the float32 with the
 *               bits hb, metres above lo_z; + 0.0 where empty.  With LCR_HEIGHTMAP_RGB in `features`: channels 1 .. 3, the colour-frame bytes x of the key's pixel as
 *               (float)x * (1.0f / 255.0f), the stack's element rule, bit for bit; 0.0 where empty.
 *   source      optional (`source` = 1), [N][Hy][Hx] int32: the g of the cell's key, - 1 where empty.
 *   count       [N] int32, always: candidates inside the box.         filled  [N] int32, always: non-empty cells.
 *               A cell filled at height 0.0 and an EMPTY cell hold the same bits in every channel but the colours: they differ only in `source` and `filled`.
 *   camera_pose [slots][13][N] float32, always: ro, X, Y, Z, s of every slot per env as the kernel used them, as the cloud and the grid report them.
 *   invariant   after every entry point that draws the batched frames -- lcr_step, lcr_reset with its masked and no-op forms, lcr_set_look, enabling -- the map is the
 *               function above of that env's current frames, planes and cameras.  No history and no reset rule: an auto-reset env shows its reset state, as its frames do.
 *   ordering    the heightmap kernel runs behind the frame kernels, the stack kernel, the cloud kernel and the voxel kernel, on whatever stream they ran on; the event the
 *               joining entry points wait for is recorded after it.  After a step on the second stream it reads the look snapshot and the pose snapshot the frames used.
 *   life        needs image observations and BOTH planes; independent of the point cloud and the voxel grid.  Fixed for the life of the handle: the same spec again does
 *               nothing, another spec is refused, naming both.
 *   memory      one allocation: LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE, the map, the same guard from the first 256-byte boundary at or behind its end (as the
 *               grid has them), then source, count, filled and camera_pose.  Freed by lcr_destroy; LCR_ERR_OOM if it fails.
 *   not in it   mean height and per-cell counts, oriented or per-env boxes, float16 / uint8 output, a per-cell surface id, the recorder, and the map of an episode that has
 *               ended: there is no _terminal call, so the vector adapters refuse the map.
 * LCR_HEIGHTMAP_ROUNDS=1|4 in the environment (read by lcr_enable_heightmap): the rounds of the scan the kernel keeps in flight, in place of the launcher's choice; the same
 * bytes under both (an A/B switch: profiles/heightmap.txt). */
enum { LCR_HEIGHTMAP_HEIGHT = 1, LCR_HEIGHTMAP_RGB = 2 };
#define LCR_HEIGHTMAP_MAX_DIM 256
#define LCR_HEIGHTMAP_MAX_CELLS 16384
typedef struct lcr_heightmap_spec {
    float lo[3];          /* x, y, z of the box's lower corner, world frame; finite */
    float hi[3];          /* x, y, z of the upper corner; finite, lo[k] < hi[k] */
    int32_t dims[2];      /* Hx, Hy: each 1 .. LCR_HEIGHTMAP_MAX_DIM, Hx a multiple of 4, Hx Hy <= LCR_HEIGHTMAP_MAX_CELLS */
    uint32_t cameras;     /* LCR_STACK_CAM_* bits; 0 = every camera the handle has */
    uint32_t ids;         /* bit i: surface id i is a candidate, i = 1 .. 10; 0 = 0x7FC (arm and cubes) */
    uint32_t features;    /* LCR_HEIGHTMAP_* bits; the height is implied, 0 = height only */
    int32_t source;       /* 0 | 1: keep the source index of every cell */
} lcr_heightmap_spec;
typedef struct lcr_heightmap_view {
    int32_t enabled;                   /* 0: no map, everything below is 0 / NULL */
    lcr_heightmap_spec spec;           /* as enabled: `cameras` and `ids` resolved to the bits in use, the height bit set in `features` */
    float inv_cell[2];                 /* inv_k: cells per metre along x, y, the float32 values the kernel multiplies with */
    int32_t channels, slots, image_width, image_height;
    const float *heightmap;            /* device, [N][C][Hy][Hx] */
    const int32_t *source;             /* device, [N][Hy][Hx], or NULL */
    const int32_t *count;              /* device, [N] */
    const int32_t *filled;             /* device, [N] */
    const float *camera_pose;          /* device, [slots][13][N] */
    uint64_t bytes_per_env;            /* C Hy Hx sizeof(float) */
} lcr_heightmap_view;
/* The checks lcr_enable_heightmap makes of `spec` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field and the axis in the message -- a
 * corner that is NaN or an infinity, lo_k >= hi_k, a dim outside 1 .. 256, Hx not a multiple of 4, more than LCR_HEIGHTMAP_MAX_CELLS cells, unknown feature bits, source
 * other than 0 / 1, and the cloud's refusals of `cameras` and `ids` */
int lcr_heightmap_check(const lcr_heightmap_spec *spec);
/* Switch the map on.  `spec` is checked first; then a NULL handle, a handle without image observations, one without both planes and a wrist bit without a wrist camera are
 * refused (LCR_ERR_INVALID, naming what is missing); an allocation that fails is LCR_ERR_OOM.  Makes the map of the current frames. */
int lcr_enable_heightmap(lcr_sim *sim, const lcr_heightmap_spec *spec);
/* The map; waits (on the handle's stream) for frames and map still being made on the second stream, as every entry point but the step does. */
int lcr_get_heightmap(lcr_sim *sim, lcr_heightmap_view *out);

/* == Object boxes: an optional device buffer per handle, `boxes` [N][slots][O][8] int32, that the library keeps current behind the frame kernels -- per env, camera and
 * object the tight 2-D box of the object's VISIBLE pixels, their count, their coordinate sums and the nearest depth among them: where an object is in a frame, how much of
 * it shows, whether it shows at all.  The labels of object-centric and keypoint policies, of visibility and occlusion terms ("is the cube in the wrist camera"), of attention
 * crops and of auto-labelled detection sets under visual domain randomisation.  One streaming kernel reads every segmentation byte once and makes every object's record, in
 * stream order, without a host round trip.  Off by default: without lcr_enable_object_boxes no byte, state, output or kernel of the handle changes.
 *   inputs      the segmentation planes of the selected camera slots at the configured size [H][W] (`cameras`: LCR_STACK_CAM_* bits, at least one; slots in the order front,
 *               top, wrist, as the cloud has them; the wrist bit on a handle without a wrist camera is refused) and, with `depth` = 1, their depth planes.
 *   object      a 32-bit mask m.  Bits 1 .. 10 select surface ids of the segmentation plane (1 the floor, 2 .. 8 base_link and link_1 .. link_6, 9 the cube, 10 the second
 *               cube); LCR_BOXES_MARKER (0x80000000u) selects the target marker, bit 7 of the byte.  Bit 0 (the sky, which is no object), bits 11 .. 30 and an empty mask are
 *               refused.  Objects may overlap: "arm" (0x1FC) beside "link_6" (0x100), "cube" beside the union of both cubes (0x600).  1 .. LCR_BOXES_MAX_OBJECTS objects.
 *   match       a segmentation byte b matches object m iff ((m >> (b & 0x7f)) & 1) != 0, or (m & LCR_BOXES_MARKER) && (b & 0x80).  (The planes hold the ids 0 .. 10; an id
 *               of 31 or more, which no plane holds, selects no bit.)  A cube pixel under the marker matches the cube AND the marker.
 *   record      eight int32 over the matching pixels (r, c) of the plane, r the row and c the column:
 *                 0 x0 = min c     1 y0 = min r     2 x1 = max c + 1     3 y1 = max r + 1     4 count = the number of matching pixels
 *                 5 sum_x = the sum of c (at most 512 * 512 * 511 / 2 = 66 977 792: it fits)     6 sum_y = the sum of r
 *                 7 nearest: with `depth` = 1 the minimum over the matching pixels of the depth plane's 32-bit word, compared as uint32 -- the planes hold positive floats,
 *                   whose words order as they do, so these are the bits of the smallest depth; with `depth` = 0: 0.
 *               x0 .. y1 are a half-open box, [x0, x1) x [y0, y1); the centroid is (sum_x / count, sum_y / count).
 *   empty       no matching pixel: all eight are zero.  count == 0 is the only "absent" test a consumer needs.
 *   boxes       [N][slots][O][8] int32, env-major.
 *   reproducible  every field is a minimum, a maximum or a sum of INTEGERS, taken with integer atomics in LDS: none depends on the order lanes arrive in, nor on the
 *               floating-point flags of the build.  The same planes give the same bytes on every run.
 *   invariant   after every entry point that draws the batched frames -- lcr_step, lcr_reset with its masked and no-op forms, lcr_set_look, enabling -- the record is the
 *               function above of that env's current planes.  No history and no reset rule: an auto-reset env shows its reset state, as its planes do.
 *   ordering    the boxes kernel is the last launch behind the frame kernels -- frames, stack, cloud, grid, map, boxes -- on whatever stream they ran on; the event the
 *               joining entry points wait for is recorded after it.
 *   life        needs image observations and the segmentation plane, with `depth` = 1 the depth plane too; no plane is switched on silently.  Fixed for the life of the
 *               handle: the same spec again does nothing, another spec is refused, naming both.
 *   memory      one allocation: LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE, the records, the same guard from the first 256-byte boundary at or behind their end (as the
 *               heightmap has them).  Freed by lcr_destroy; LCR_ERR_OOM if it fails.
 *   not in it   amodal boxes (the extent of occluded parts), oriented boxes, instances beyond the surface ids, a normalised float form (one torch expression over the
 *               record), the recorder, and the boxes of an episode that has ended: there is no _terminal call, so the vector adapters refuse them. */
#define LCR_BOXES_MAX_OBJECTS 16
#define LCR_BOXES_MARKER 0x80000000u
enum { LCR_BOXES_X0 = 0, LCR_BOXES_Y0 = 1, LCR_BOXES_X1 = 2, LCR_BOXES_Y1 = 3, LCR_BOXES_COUNT = 4, LCR_BOXES_SUM_X = 5, LCR_BOXES_SUM_Y = 6, LCR_BOXES_NEAREST = 7 };
typedef struct lcr_object_boxes_spec {
    uint32_t cameras;                           /* LCR_STACK_CAM_* bits, at least one */
    int32_t n_objects;                          /* 1 .. LCR_BOXES_MAX_OBJECTS */
    uint32_t objects[LCR_BOXES_MAX_OBJECTS];    /* [i < n_objects]: bits 1 .. 10 and LCR_BOXES_MARKER, not empty; [i >= n_objects] ignored (reported as 0) */
    int32_t depth;                              /* 0 | 1: keep the nearest depth word of every record */
} lcr_object_boxes_spec;
typedef struct lcr_object_boxes_view {
    int32_t enabled;                   /* 0: no boxes, everything below is 0 / NULL */
    lcr_object_boxes_spec spec;        /* as enabled; the masks beyond n_objects are 0 */
    int32_t slots, image_width, image_height;
    const int32_t *boxes;              /* device, [N][slots][O][8] */
    uint64_t bytes_per_env;            /* slots O 8 sizeof(int32_t) */
} lcr_object_boxes_view;
/* The checks lcr_enable_object_boxes makes of `spec` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field in the message -- cameras 0 or
 * with unknown bits, n_objects outside 1 .. 16, an object that is empty or selects bit 0 or one of bits 11 .. 30 (named with its index), depth other than 0 / 1 */
int lcr_object_boxes_check(const lcr_object_boxes_spec *spec);
/* Switch the boxes on.  `spec` is checked first; then a NULL handle, a handle without image observations, one without the segmentation plane, `depth` without the depth plane
 * and a wrist bit without a wrist camera are refused (LCR_ERR_INVALID, naming what is missing); an allocation that fails is LCR_ERR_OOM.  Makes the records of the current
 * planes. */
int lcr_enable_object_boxes(lcr_sim *sim, const lcr_object_boxes_spec *spec);
/* The records; waits (on the handle's stream) for frames and records still being made on the second stream, as every entry point but the step does. */
int lcr_get_object_boxes(lcr_sim *sim, lcr_object_boxes_view *out);

/* == Surface normals: optional device buffers per handle, one plane `normals` [N][H][W][4] int8 per selected camera, that the library keeps current behind the frame kernels
 * -- per pixel the unit normal of the surface the pixel shows and the face of the box it belongs to.  For point clouds with normals (grasp-pose networks gather them through
 * the cloud's `source`), RGB-D-N inputs, and contact-direction or "which face of the cube" labels.  The normal is EXACT, not estimated from depth gradients: every opaque
 * surface is the floor or one of nine oriented boxes, the segmentation byte says which, the depth plane gives the point, and the pose snapshot the frames were drawn from
 * gives the box frames.  One streaming kernel, in stream order, without a host round trip.  Off by default: without lcr_enable_normals no byte, state, output or kernel of
 * the handle changes.
 *   inputs      the segmentation and depth planes of the selected camera slots at the configured size [H][W] (`cameras`: LCR_STACK_CAM_* bits, 0 = every camera the handle
 *               has; slots in the order front, top, wrist, as the cloud has them; the wrist bit on a handle without a wrist camera is refused), the camera that drew each
 *               slot (the env's look variant's; the wrist pose of the step) and the pose snapshot `qpos` the frames were drawn from.
 *   element     [..., 0:3] the normal n as rint(127 n), [..., 3] the face code w:
 *                 w = 0                    no surface (sky): four zeros
 *                 w = 1 + 2 axis + side    face `axis` (0 X, 1 Y, 2 Z) of the box's own frame, `side` 1 on the negative side: 1 .. 6
 *                 the floor is w = 5, the + Z face of the world: (0, 0, 127, 5) in the world frame
 *   boxes       the nine opaque boxes in the order of the surface ids 2 .. 10 (base_link, link_1 .. link_6, the cube, the second cube), placed as the frame kernels place
 *               them: centre c, axes X, Y, Z (A_0, A_1, A_2) and half-extents h in float32, reported as `boxes` [9][15][N] (c, X, Y, Z, h) exactly as the kernel used them;
 *               all 15 are zero for a second cube the task does not have.
 *   the rule    for pixel (row, px) of a slot with id i = seg & 0x7F.  The marker bit is ignored: the normal is that of the opaque surface the id names.
 *                 i = 0 or i > 10   four zeros
 *                 i = 1             world + z, w = 5
 *                 i = 2 .. 10       box i - 2:
 *                   p     the pinned point of the crop box, the voxel grid and the heightmap: per axis fmaf(t, fmaf(sx, X, fmaf(sy, Y, -Z)), ro) with sx = (px + 0.5 -
 *                         W / 2) s and sy = -((row + 0.5 - H / 2) s) one rounded float32 multiply each, t the depth word as stored, and ro, X, Y, Z, s the reported
 *                         `camera_pose` of the slot
 *                   u     = p - c: one float32 subtraction per axis
 *                   l_k   = fmaf(u.x, A_k.x, fmaf(u.y, A_k.y, u.z * A_k.z)) for k = 0, 1, 2
 *                   e_k   = |l_k| - h_k: one float32 subtraction
 *                   axis  the largest e_k, ties to the lowest k: e_0 >= e_1 && e_0 >= e_2 ? 0 : e_1 >= e_2 ? 1 : 2
 *                   side  negative (1) iff l_axis < 0.0f
 *                   n     = +- A_axis
 *   quantised   each of the at most 55 vectors per (env, slot) -- the floor and six faces of nine boxes -- once: clamp((int)rintf(127.0f * component), -127, 127), rintf
 *               to nearest even.  `frame` LCR_NORMALS_WORLD: the component of n itself.  LCR_NORMALS_CAMERA: first dot(n, C) = fmaf(n.x, C.x, fmaf(n.y, C.y, n.z * C.z))
 *               for C the slot's camera axis X, Y, Z in turn -- the axes the cloud, the grid and the map use, those of the camera that drew the pixel.  The axes of a
 *               cube are those of its quaternion as stored; the clamp keeps a component that a quaternion off the unit sphere by rounding would carry past 127.
 *   reproducible  every word is a function of its own pixel, the boxes and the pose: nothing depends on the order lanes arrive in, there are no atomics, and every rounded
 *               intermediate above is one float32 operation whatever the floating-point flags of the build.
 *   depth_far   a depth clipped at depth_far gives the face of the CLIPPED point, which need not be the face the ray entered by: depth_far belongs beyond the scene, as
 *               its default (10 m) is.  There is no special case.
 *   invariant   after every entry point that draws the batched frames -- lcr_step, lcr_reset with its masked and no-op forms, lcr_set_look, enabling -- each plane is the
 *               function above of that env's current planes, boxes and pose.  No history and no reset rule: an auto-reset env shows its reset state, as its planes do.
 *   ordering    the normals kernel is the last launch behind the frame kernels -- frames, stack, cloud, grid, map, boxes, normals -- on whatever stream they ran on; the
 *               event the joining entry points wait for is recorded after it.
 *   life        needs image observations and BOTH planes, neither switched on silently (lcr_enable_image_planes stays what it is: normals are no third plane bit).  Fixed
 *               for the life of the handle: the same spec again does nothing, another spec is refused, naming both.
 *   memory      4 bytes per pixel and camera (307 200 bytes per env and camera at 240 x 320); the caller chooses it.  One allocation: LCR_WRIST_GUARD bytes of
 *               LCR_WRIST_GUARD_BYTE, then per slot the plane and the same guard from the first 256-byte boundary at or behind its end (every plane lies between two guard
 *               regions, as the wrist buffers do), then boxes and camera_pose.  Freed by lcr_destroy; LCR_ERR_OOM if it fails.
 *   not in it   float output (one torch expression, x[..., :3].float() * (1 / 127)), terminal planes (there is no _terminal call, so the vector adapters refuse them), the
 *               recorder, a normals channel of the stack or the cloud, and the marker's own faces. */
enum { LCR_NORMALS_WORLD = 0, LCR_NORMALS_CAMERA = 1 };
typedef struct lcr_normals_spec {
    uint32_t cameras;                  /* LCR_STACK_CAM_* bits; 0 = every camera the handle has */
    int32_t frame;                     /* LCR_NORMALS_WORLD | LCR_NORMALS_CAMERA */
} lcr_normals_spec;
typedef struct lcr_normals_view {
    int32_t enabled;                   /* 0: no normals, everything below is 0 / NULL */
    lcr_normals_spec spec;             /* as enabled, cameras resolved */
    int32_t slots, image_width, image_height;
    const int8_t *normals_front, *normals_top, *normals_wrist;   /* device, [N][H][W][4]; NULL for a camera that is not selected */
    const float *boxes;                /* device, [9][15][N]: c, X, Y, Z, h of the nine boxes */
    const float *camera_pose;          /* device, [slots][13][N]: ro, X, Y, Z, s */
    uint64_t bytes_per_env;            /* slots H W 4 */
} lcr_normals_view;
/* The checks lcr_enable_normals makes of `spec` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID with the field in the message -- cameras with unknown
 * bits, frame other than 0 / 1 */
int lcr_normals_check(const lcr_normals_spec *spec);
/* Switch the normals on.  `spec` is checked first; then a NULL handle, a handle without image observations, one without both planes (naming the missing one) and a wrist bit
 * without a wrist camera are refused (LCR_ERR_INVALID); an allocation that fails is LCR_ERR_OOM.  Makes the planes of the current frames. */
int lcr_enable_normals(lcr_sim *sim, const lcr_normals_spec *spec);
/* The planes; waits (on the handle's stream) for frames and normals still being made on the second stream, as every entry point but the step does. */
int lcr_get_normals(lcr_sim *sim, lcr_normals_view *out);

/* == Motion vectors: optional device buffers per handle, one plane `flow` [N][H][W][2] float16 per selected camera, that the library keeps current behind the frame kernels --
 * per pixel the BACKWARD optical flow of the surface point the pixel shows: current pixel position minus the position of the same point one control step (one lcr_step) ago,
 * in pixels, x to the right and y down.  The point pixel (row, px) shows was at (px - fx, row - fy) in the frame of the previous step.  For flow-conditioned policies,
 * point-track prediction and video-prediction pre-training.  The flow is EXACT, not estimated from two frames: every opaque surface is the floor or one of nine rigid boxes,
 * the segmentation byte says which, the depth plane gives the point, and the pose snapshots of this step and the previous one give the rigid motion of that box and of the
 * camera.  One streaming kernel, in stream order, without a host round trip.  Off by default: without lcr_enable_motion_vectors no byte, state, output or kernel of the handle
 * changes.  It is the one observation with a step of history in its geometry: the stack keeps frames, this keeps poses.
 *   inputs      as the surface normals: the segmentation and depth planes of the selected camera slots at the configured size [H][W] (`cameras`: LCR_STACK_CAM_* bits, 0 =
 *               every camera the handle has; slots in the order front, top, wrist; the wrist bit on a handle without a wrist camera is refused), the camera that drew each
 *               slot and the pose snapshot `qpos` the frames were drawn from -- and the same of the previous step, kept as numbers, never recomputed.
 *   element     [..., 0] fx and [..., 1] fy as IEEE binary16.
 *   history     `boxes` [2][9][15][N] and `camera_pose` [2][slots][13][N], [0] NOW and [1] BEFORE, in the layout of the normals' boxes (c, X, Y, Z, h of the nine opaque
 *               boxes, surface ids 2 .. 10) and camera_pose (ro, X, Y, Z, s): exactly what the kernel used and what a model of the rule reads.  This unit is built without
 *               -ffast-math (see "the division"), so the sine and cosine behind the wrist pose and the arm boxes may differ in the last bit from what the normals' unit
 *               computes from the same joints: a model reads THESE arrays, not the normals'.
 *   valid       [N] uint8: 1 iff the env's planes describe the motion across the last lcr_step and that step did not auto-reset the env.
 *   bit-equal   a slot is CAMERA-STATIC iff its 13 pose words are bit-equal now and before; box b is STATIC iff its 12 words c, A_0, A_1, A_2 are.  Both compare the uint32
 *               words, not the floats.
 *   the rule    for pixel (row, px) of a slot with pose now (ro, X, Y, Z, s) and before (ro', X', Y', Z', s'), id i = seg & 0x7F (the marker bit is ignored), box b = i - 2
 *               now (c, A_0, A_1, A_2) and before (c', A'_0, A'_1, A'_2).  Every step is ONE float32 operation; dot(a, b) = fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)).
 *                 env not valid, or i = 0, or i > 10              (+0.0, +0.0): the sky carries no flow, also under a turning wrist camera
 *                 i = 1 (the floor), slot camera-static           (+0.0, +0.0), no depth is loaded
 *                 i = 1, otherwise                                the chain with q = p
 *                 i = 2 .. 10, box b static, slot camera-static   (+0.0, +0.0), no depth is loaded
 *                 i = 2 .. 10, otherwise                          the chain
 *   the chain     hx    = px + 0.5 - W / 2, hy = row + 0.5 - H / 2: exact
 *                 p     the pinned point of the crop box, the grid, the map and the normals, through the pose NOW and the depth word as stored: per axis
 *                       fmaf(t, fmaf(sx, X, fmaf(sy, Y, -Z)), ro) with sx = hx s and sy = -(hy s) one rounded multiply each
 *                 u     = p - c per axis
 *                 l_k   = dot(u, A_k) for k = 0, 1, 2: the point in the box's own frame
 *                 q     per axis: fmaf(l_0, A'_0.axis, fmaf(l_1, A'_1.axis, fmaf(l_2, A'_2.axis, c'.axis))): the same point of the box where the box was
 *                 w     = q - ro' per axis
 *                 a     = dot(w, X'), b = dot(w, Y'), d = dot(w, Z')
 *                 den   = (-d) * s'
 *                 !(den > 0.0f): (+0.0, +0.0) -- a point behind the previous camera; it cannot happen on the fixed cameras
 *                 gx    = a / den, gy = b / den: ONE correctly rounded float32 division each
 *                 fx    = hx - gx, fy = hy + gy
 *                 out   ((half)fx, (half)fy), each rounded to nearest even; an overflow gives what the conversion gives (an infinity)
 *   the division  under -ffast-math every spelling of a float32 division compiles to a reciprocal and a multiply on gfx950, so the unit of this kernel alone is built with
 *               -fno-fast-math -ffp-contract=off (gym_lowcostrobot_amd/build.py) and the division is the IEEE one.
 *   reproducible  every word is a function of its own pixel and the history: nothing depends on the order lanes arrive in.
 *   invariant   lcr_step is the only entry point that MEASURES: before its kernel "now" becomes "before" (two device-to-device copies, about 700 bytes an env together, on
 *               the stream the frames run on), the kernel reads only "before" and writes only "now", and valid[env] = !did_reset[env], read from the snapshot of the flags
 *               the step takes for the stack (taken for the motion vectors too on a handle without a stack).  An env the step has auto-reset has zero planes.
 *               Every other entry point that draws the batched frames -- lcr_reset with its masked and no-op forms, lcr_set_look, enabling -- and lcr_set_state (which
 *               draws none, but makes the state jump) RESTARTS every env: the planes are zero, valid is 0, "now" is the current state and "before" a copy of it, so the
 *               next step is valid.
 *   ordering    the motion-vector kernel is the last launch behind the frame kernels -- frames, stack, cloud, grid, map, boxes, normals, motion vectors -- on whatever stream
 *               they ran on; the event the joining entry points wait for is recorded after it.
 *   life        needs image observations and BOTH planes, neither switched on silently.  Fixed for the life of the handle: the same spec again does nothing, another spec is
 *               refused, naming both.
 *   memory      4 bytes per pixel and camera (307 200 bytes per env and camera at 240 x 320); the caller chooses it.  One allocation, laid out as the normals' is:
 *               LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE, then per slot the plane and the same guard from the first 256-byte boundary at or behind its end, then
 *               boxes, camera_pose, valid and two snapshots of did_reset.  Freed by lcr_destroy; LCR_ERR_OOM if it fails.
 *   not in it   an occlusion or disocclusion mask, forward flow on the previous frame's grid, scene flow in metres, flow of the sky or of the marker, float32 output,
 *               terminal planes (there is no _terminal call, so the vector adapters refuse them), the recorder, a flow channel of the stack. */
typedef struct lcr_motion_spec {
    uint32_t cameras;                  /* LCR_STACK_CAM_* bits; 0 = every camera the handle has */
} lcr_motion_spec;
typedef struct lcr_motion_view {
    int32_t enabled;                   /* 0: no motion vectors, everything below is 0 / NULL */
    lcr_motion_spec spec;              /* as enabled, cameras resolved */
    int32_t slots, image_width, image_height;
    const uint16_t *flow_front, *flow_top, *flow_wrist;   /* device, [N][H][W][2] binary16; NULL for a camera that is not selected */
    const uint8_t *valid;              /* device, [N] */
    const float *boxes;                /* device, [2][9][15][N]: now, before -- c, X, Y, Z, h of the nine boxes */
    const float *camera_pose;          /* device, [2][slots][13][N]: now, before -- ro, X, Y, Z, s */
    uint64_t bytes_per_env;            /* slots H W 4 */
} lcr_motion_view;
/* The checks lcr_enable_motion_vectors makes of `spec` before it looks at the handle, on their own: LCR_OK, or LCR_ERR_INVALID -- cameras with unknown bits */
int lcr_motion_check(const lcr_motion_spec *spec);
/* Switch the motion vectors on.  `spec` is checked first; then a NULL handle, a handle without image observations, one without both planes (naming the missing one) and a
 * wrist bit without a wrist camera are refused (LCR_ERR_INVALID); an allocation that fails is LCR_ERR_OOM.  Restarts: zero planes, valid 0. */
int lcr_enable_motion_vectors(lcr_sim *sim, const lcr_motion_spec *spec);
/* The planes; waits (on the handle's stream) for frames and motion vectors still being made on the second stream, as every entry point but the step does. */
int lcr_get_motion_vectors(lcr_sim *sim, lcr_motion_view *out);

/* Measurement support: copy n_floats floats from the start of the state arena to dst_dev with one dword load and
 * one dword store per lane (the step kernel's access pattern): a launch with a KNOWN byte count (4*n read, 4*n
 * written) against which rocprofv3 FETCH_SIZE / WRITE_SIZE are calibrated (MI355X_MICROARCH.md, HBM section). */
int lcr_calibrate_copy(lcr_sim *sim, float *dst_dev, size_t n_floats);

#ifdef __cplusplus
}
#endif
#endif /* LCR_H */
