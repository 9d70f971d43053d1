// lcr_capi.hip -- the C ABI of include/lcr.h: device-memory ownership, launches, host<->device state I/O.
// No simulation arithmetic lives here (that is lcr_kernels.hip) and there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lcr.h"
#include "lcr_device.h"
#include "lcr_model_gen.h"
#include "lcr_stack.h"
#include "lcr_cloud.h"
#include "lcr_voxel.h"
#include "lcr_heightmap.h"
#include "lcr_boxes.h"
#include "lcr_normals.h"
#include "lcr_flow.h"

static_assert(LCR_NWARM == LCR_DEV_NWARM, "include/lcr.h and lcr_device.h disagree on the carried-force block");

namespace {
thread_local char g_err[768] = "";   // (the longest message, the refusal of another point cloud, names two specs, samplings and crop boxes)

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(LCR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
// the status of a kernel launcher: 0, a hipError_t, or -- lcr_launch_obs_stack alone -- a negative number for arguments it refuses
#define LAUNCHCHK(what, expr)                                                                  \
    do {                                                                                       \
        int _rc = (expr);                                                                      \
        if (_rc) return fail(LCR_ERR_HIP, what " launch failed: %s", _rc < 0 ? "bad arguments" : hipGetErrorString((hipError_t)_rc)); \
    } while (0)

// grows the device scratch buffer `*buf` of `*have` bytes to `need` bytes (what it held is dropped)
int reserve(void **buf, size_t *have, size_t need) {
    if (need <= *have) return LCR_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    hipError_t e = hipMalloc(buf, need);
    if (e != hipSuccess) return fail(LCR_ERR_OOM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
    *have = need;
    return LCR_OK;
}

// the layout of one allocation: slices handed out front to back, each rounded up to a multiple of 256 bytes
struct Carver {
    size_t off = 0;   // bytes handed out so far: the offset of the next slice, at the end the size of the allocation
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }   // (0 bytes: the offset of whatever follows, nothing taken)
    size_t skip(size_t bytes) { const size_t o = off; off += bytes; return o; }                          // as it is, not rounded: the guard regions
};
}  // namespace

namespace {
// `rot` (or null): a rotation vector, world frame, the finished axes are turned by (lcr_look_variant.cam_drot); `fovy_deg` 45: MuJoCo's default camera fovy
void cam_finish(LcrCam &c, const double p[3], double X[3], double Y[3], int height, const double *rot = nullptr, double fovy_deg = 45.0) {
    auto nrm = [](double *v) { double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= n; v[1] /= n; v[2] /= n; };
    nrm(X);
    double d = X[0] * Y[0] + X[1] * Y[1] + X[2] * Y[2];
    for (int i = 0; i < 3; i++) Y[i] -= d * X[i];
    nrm(Y);
    double Z[3] = {X[1] * Y[2] - X[2] * Y[1], X[2] * Y[0] - X[0] * Y[2], X[0] * Y[1] - X[1] * Y[0]};
    const double th = rot ? std::sqrt(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2]) : 0.0;
    if (th > 0.0) {   // Rodrigues: v cos + (k x v) sin + k (k . v)(1 - cos); no rotation leaves the axes bit for bit
        const double k[3] = {rot[0] / th, rot[1] / th, rot[2] / th}, cs = std::cos(th), sn = std::sin(th);
        for (double *v : {X, Y, Z}) {
            const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
            const double cr[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
            for (int i = 0; i < 3; i++) v[i] = v[i] * cs + cr[i] * sn + k[i] * kv * (1.0 - cs);
        }
    }
    c.px = (float)p[0]; c.py = (float)p[1]; c.pz = (float)p[2];
    c.xx = (float)X[0]; c.xy = (float)X[1]; c.xz = (float)X[2];
    c.yx = (float)Y[0]; c.yy = (float)Y[1]; c.yz = (float)Y[2];
    c.zx = (float)Z[0]; c.zy = (float)Z[1]; c.zz = (float)Z[2];
    // (45 degrees keeps its own expression: the scene cameras' `s` stays the constant it has always been, whatever the compiler makes of the general one)
    if (fovy_deg == 45.0) c.s = (float)(2.0 * std::tan(0.5 * 45.0 * M_PI / 180.0) / height);  // MuJoCo default camera fovy = 45 deg
    else c.s = (float)(2.0 * std::tan(0.5 * fovy_deg * M_PI / 180.0) / height);
}
// scene pose of observation camera `which` (0 camera_front, 1 camera_top; reach_cube.xml:29-30 and siblings)
void scene_cam_pose(int which, double p[3], double X[3], double Y[3]) {
    static const double P[2][3] = {{0.049, 0.5, 0.225}, {0, 0.1, 0.6}}, XX[2][3] = {{-0.998, 0.056, -0.000}, {1, 0, 0}}, YY[2][3] = {{-0.019, -0.335, 0.942}, {0, 1, 0}};
    for (int i = 0; i < 3; i++) { p[i] = P[which][i]; X[i] = XX[which][i]; Y[i] = YY[which][i]; }
}
// observation camera `which` of a look variant for frames `height` rows high: the scene camera moved by cam_dpos, turned by cam_drot, with the variant's fovy
void make_look_camera(const lcr_look_variant &v, int which, int height, LcrCam &out) {
    double p[3], X[3], Y[3];
    scene_cam_pose(which, p, X, Y);
    double rot[3];
    for (int i = 0; i < 3; i++) { p[i] += (double)v.cam_dpos[which][i]; rot[i] = (double)v.cam_drot[which][i]; }
    cam_finish(out, p, X, Y, height, rot, (double)v.fovy_deg[which]);
}
// cameras of the scene files (reach_cube.xml:29-31 and siblings)
void make_cameras(int task, int img_h, LcrCam &front, LcrCam &top, LcrCam &vizu) {
    {   // camera_front pos="0.049 0.5 0.225" xyaxes="-0.998 0.056 -0.000 -0.019 -0.335 0.942"
        double p[3] = {0.049, 0.5, 0.225}, X[3] = {-0.998, 0.056, -0.000}, Y[3] = {-0.019, -0.335, 0.942};
        cam_finish(front, p, X, Y, img_h);
    }
    {   // camera_top pos="0 0.1 0.6" euler="0 0 0"
        double p[3] = {0, 0.1, 0.6}, X[3] = {1, 0, 0}, Y[3] = {0, 1, 0};
        cam_finish(top, p, X, Y, img_h);
    }
    {   // camera_vizu pos="-0.2 0.6 0.3" (reach) / "-0.1 0.6 0.3" (others) quat="-0.15 -0.1 0.6 1"
        double p[3] = {task == LCR_TASK_REACH ? -0.2 : -0.1, 0.6, 0.3};
        double q[4] = {-0.15, -0.1, 0.6, 1.0}, n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
        double X[3] = {1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)};
        double Y[3] = {2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)};
        cam_finish(vizu, p, X, Y, 640);
    }
}
}  // namespace

struct lcr_sim {
    lcr_config cfg;
    LcrDev dev;
    int nq, nv, k;
    int ee_mode;
    hipStream_t stream;
    void *arena;        // one allocation holding every SoA array
    size_t arena_bytes;
    LcrRedo redo;            // one-cube Newton kernels: the per-wave flags of the pair of launches and whether the pair runs (lcr_device.h)
    size_t redo_words;       // ints of redo.flags (0: this handle's step kernel keeps no such flags)
    float *action_stage;     // [k][N] staging for lcr_step_host
    unsigned char *mask_dev; // [N]
    unsigned long long *seeds_dev; // [N]
    hipEvent_t ev0, ev1;
    bool has_images;
    LcrCam cam_front, cam_top, cam_vizu;
    unsigned char *render_dev;  // scratch frame for lcr_render
    size_t render_bytes;
    void *term_stage;           // staging of lcr_render_terminal: env ids, gathered poses, two frame blocks
    size_t term_stage_bytes;
    // lcr_fetch_host: pinned host mirror of the arena range [qpos .. did_reset] (+ terminal observations)
    size_t fetch_bytes, tobs_off, tobs_bytes;
    char *host_mirror;
    // image observations: the frames of step k are ray-cast on a second stream from a snapshot of the poses while the step kernel of step k + 1 runs (lcr_step).  The
    // step kernel is VALU-bound and ends with a tail of few slow waves, the frame kernel is HBM-write-bound: together they take little more than the longer one.
    // Every entry point that takes the handle, except the four that touch no frame (lcr_step, lcr_fill_random_actions, lcr_get_outputs, lcr_step_kernel_family), first makes
    // the caller's stream wait for the pending frames (join_render: a hipStreamWaitEvent, no host wait), so nothing but lcr_step sees the second stream.
    hipStream_t rstream;         // null: frames on the caller's stream, after the step kernel (LCR_RENDER_OVERLAP=0)
    hipEvent_t ev_snap[2], ev_rdone[2];
    float *snap_qpos[2], *snap_target[2];
    bool snap_used[2];
    int rpar, rlast;
    bool rpending;
    // depth / segmentation planes of the frames (lcr_enable_image_planes): one allocation, fixed for the life of the handle
    uint32_t planes;             // LCR_PLANE_* bits in use, 0: none
    LcrPlanes pl;
    void *planes_mem;
    // the look (lcr_enable_look): one allocation, fixed for the life of the handle.  A look is ten words per env, [10][N]: row 0 the variant, rows 1 .. 9 the colours
    int look_K;                  // variants, 0: no look
    void *look_mem;
    LcrLook look;                // the arguments of the kernels that draw with the envs' current looks
    int *look_cur, *look_term;   // current / terminal looks
    unsigned *look_episode;      // [N]
    int *snap_look[2];           // beside snap_qpos / snap_target
    LcrLookSampler look_sm;
    lcr_look_variant *look_variants;   // host copies of the arguments of lcr_enable_look
    lcr_look_sampler look_sampler;
    bool look_has_sampler;
    // the wrist camera (lcr_enable_wrist_camera): its frames are one allocation, its planes live in planes_mem; fixed for the life of the handle
    bool wrist_on;
    lcr_wrist_camera wrist_cam;  // the arguments of lcr_enable_wrist_camera
    LcrWrist wrist;              // the arguments of the kernels that draw it
    void *wrist_mem;
    // the observation stack (lcr_enable_obs_stack): one allocation -- guard, stack, guard, the two snapshots of did_reset --, fixed for the life of the handle
    bool stack_on;
    lcr_obs_stack_spec stack_spec;     // as enabled, cameras resolved
    LcrStack stack;                    // the arguments of its kernel (flags and op are set per launch)
    void *stack_mem;
    size_t stack_bytes_per_env;
    unsigned char *snap_reset[2];      // beside snap_qpos / snap_target / snap_look
    // terminal stacks (lcr_enable_obs_stack_terminal with keep_terminal = 1): the history [N][K - 1][C][H][W] lies in stack_mem behind the stack's second guard, with a guard
    // of its own behind it; stack.history is null without it (K = 1 keeps nothing: the terminal stack is the terminal frame)
    bool stack_keep;
    size_t stack_hist_bytes_per_env;
    // the depth channel (lcr_enable_obs_stack_planes): LCR_PLANE_DEPTH or 0; with it stack.cpc is 4, stack.depth the handle's depth planes, and depth_far is fixed
    uint32_t stack_planes;
    // the point cloud (lcr_enable_point_cloud): one allocation -- guard, points, guard, count, source, camera poses --, fixed for the life of the handle
    bool cloud_on;
    lcr_point_cloud_spec cloud_spec;   // as enabled, cameras and ids resolved
    LcrCloud cloud;                    // the arguments of its kernel (the cameras and the pose snapshot are set per launch)
    lcr_point_cloud_sampling cloud_sampling;   // stride, or farthest-point sampling from a pool (lcr_enable_point_cloud_sampled): which kernel makes the cloud
    bool cloud_crop_on;                // a crop box (lcr_enable_point_cloud_cropped): the kernels of lcr_cloud_crop.hip make the cloud
    lcr_point_cloud_crop cloud_crop;
    void *cloud_mem;
    // the voxel grid (lcr_enable_voxel_grid): one allocation -- guard, voxels, guard, source, count, occupied, camera poses --, fixed for the life of the handle
    bool voxel_on;
    lcr_voxel_grid_spec voxel_spec;    // as enabled, cameras, ids and features resolved
    LcrVoxel voxel;                    // the arguments of its kernel (the cameras and the pose snapshot are set per launch)
    void *voxel_mem;
    size_t voxel_bytes_per_env;
    // the heightmap (lcr_enable_heightmap): one allocation -- guard, map, guard, source, count, filled, camera poses --, fixed for the life of the handle
    bool height_on;
    lcr_heightmap_spec height_spec;    // as enabled, cameras, ids and features resolved
    LcrHeightmap height;               // the arguments of its kernel (the cameras and the pose snapshot are set per launch)
    void *height_mem;
    size_t height_bytes_per_env;
    // the object boxes (lcr_enable_object_boxes): one allocation -- guard, records, guard --, fixed for the life of the handle
    bool boxes_on;
    lcr_object_boxes_spec boxes_spec;  // as enabled, the masks beyond n_objects zero
    LcrBoxes boxes;                    // the arguments of their kernel: a view of the handle's own planes
    void *boxes_mem;
    // the surface normals (lcr_enable_normals): one allocation -- guard, then per slot plane and guard, boxes, camera poses --, fixed for the life of the handle
    bool normals_on;
    lcr_normals_spec normals_spec;     // as enabled, cameras resolved
    LcrNormals normals;                // the arguments of their kernel (the cameras and the pose snapshot are set per launch)
    void *normals_mem;
    // the motion vectors (lcr_enable_motion_vectors): one allocation -- guard, then per slot plane and guard, boxes, camera poses (now and before each), valid, the two
    // snapshots of did_reset a handle without a stack has nowhere else --, fixed for the life of the handle
    bool flow_on;
    lcr_motion_spec flow_spec;         // as enabled, cameras resolved
    LcrFlow flow;                      // the arguments of their kernel (the cameras, the pose snapshot, the flags and the mode are set per launch)
    void *flow_mem;
    unsigned char *flow_reset[2];      // beside snap_qpos / snap_target / snap_look; used when there is no stack (whose snap_reset serves both)
};

// the looks P's envs are drawn with: the current ones, or `look` ([10][P.n]: a snapshot, the gathered terminal looks)
static LcrLook look_args(const lcr_sim *s, const LcrDev &P, const int *look) {
    LcrLook LK = s->look;
    if (look) { LK.variant = look; LK.rgb = (const float *)(look + P.n); }
    return LK;
}

// the wrist frames (and planes) of P's envs, behind the two colour frames on the same stream
static int launch_wrist_frames(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look = nullptr) {
    if (!s->look_K) return lcr_launch_render_wrist(P, s->wrist, nullptr, stream);
    const LcrLook LK = look_args(s, P, look);
    return lcr_launch_render_wrist(P, s->wrist, &LK, stream);
}

static int launch_frames(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look = nullptr) {
    int rc;
    if (s->look_K) rc = lcr_launch_render_obs_look(P, look_args(s, P, look), s->planes ? &s->pl : nullptr, stream);
    else if (s->planes) rc = lcr_launch_render_obs_planes(P, s->cam_front, s->cam_top, s->pl, stream);
    else rc = lcr_launch_render_obs(P, s->cam_front, s->cam_top, stream);
    if (!rc && s->wrist_on) rc = launch_wrist_frames(s, P, stream, look);
    return rc;
}

// the stack kernel, behind the frame kernels on their stream: envs with flags[e] != 0 are refilled, `op` (LCR_STACK_*) is what happens to the others (flags null: to all).
// `step`: the launch of lcr_step, whose flags are did_reset -- on a handle that keeps terminal stacks the refilled envs first save their history (a handle that does
// not launches the kernel it always has)
static int launch_stack(lcr_sim *s, hipStream_t stream, const unsigned char *flags, int op, bool step) {
    LcrStack A = s->stack;
    A.flags = flags; A.op = op;
    A.mode = step && A.history ? LCR_STACK_MODE_SAVE : LCR_STACK_MODE_PLAIN;
    return lcr_launch_obs_stack(A, stream);
}

// What every kernel of a depth-plane observation (LcrCloud, LcrVoxel, LcrHeightmap, LcrNormals) is told per launch: the cameras that drew the frames of P's envs -- the
// handle's or, with a look, those of the envs' variants (`look` as in look_args) -- and P's qpos, the pose snapshot the wrist frames were drawn from
template <class Args>
static Args with_cameras(const lcr_sim *s, const LcrDev &P, const int *look, Args A) {
    A.front = s->cam_front; A.top = s->cam_top;
    if (s->look_K) { const LcrLook LK = look_args(s, P, look); A.var = LK.var; A.variant = LK.variant; }
    A.qpos = P.qpos;
    return A;
}

// the cloud kernel, behind the frame kernels (and the stack kernel) on their stream: the cloud of P's envs from the frames just drawn (with_cameras).
// `view` (or null: the handle's own buffers): the cloud's arguments with planes, frames, outputs and n of a view of some envs (lcr_point_cloud_terminal)
static int launch_cloud(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look, const LcrCloud *view = nullptr) {
    const LcrCloud A = with_cameras(s, P, look, view ? *view : s->cloud);
    if (s->cloud_crop_on) {   // (a handle without a crop launches what it launched before there was one)
        LcrCloudCrop B{};
        B.c = A;
        for (int k = 0; k < 3; k++) { B.lo[k] = s->cloud_crop.lo[k]; B.hi[k] = s->cloud_crop.hi[k]; }
        B.pool = s->cloud_sampling.mode == LCR_CLOUD_SAMPLE_FPS ? s->cloud_sampling.pool : 0;
        return lcr_launch_point_cloud_crop(B, stream);
    }
    if (s->cloud_sampling.mode == LCR_CLOUD_SAMPLE_FPS) return lcr_launch_point_cloud_fps(LcrCloudFps{A, s->cloud_sampling.pool}, stream);
    return lcr_launch_point_cloud(A, stream);
}

// the grid, the heightmap and the normals kernel, in this order behind the frame kernels (the stack kernel and the cloud kernel) on their stream: the grid, the map and the
// normal planes of P's envs from the frames just drawn (with_cameras; the normals' boxes come from P's qpos too)
static int launch_voxel(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look) { return lcr_launch_voxel_grid(with_cameras(s, P, look, s->voxel), stream); }
static int launch_heightmap(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look) { return lcr_launch_heightmap(with_cameras(s, P, look, s->height), stream); }
static int launch_normals(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look) { return lcr_launch_normals(with_cameras(s, P, look, s->normals), stream); }

// the motion-vector kernel, the last behind the frame kernels on their stream.  `step`: the launch of lcr_step, the only one that measures -- "now" (the boxes and the
// poses of the previous launch) first becomes "before", on the same stream, so the kernel reads only "before" and writes only "now"; `flags` is did_reset of that step.
// Every other launch restarts every env: zero planes, valid 0, "before" a copy of "now"
static int launch_flow(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look, const unsigned char *flags, bool step) {
    LcrFlow A = with_cameras(s, P, look, s->flow);
    A.restart = step ? 0 : 1;
    A.flags = step ? flags : nullptr;
    if (step) {
        const size_t N = (size_t)A.n, boxes = (size_t)LCR_FLOW_BOXES * LCR_FLOW_BOX_FLOATS * N, poses = (size_t)A.slots * 13 * N;
        hipError_t e = hipMemcpyAsync(A.boxes + boxes, A.boxes, boxes * sizeof(float), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(A.pose + poses, A.pose, poses * sizeof(float), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return (int)e;
    }
    return lcr_launch_flow(A, stream);
}

// frames, then stack, then cloud: what every entry point that has changed the poses or the looks enqueues on `stream` -- the frames of P's envs (`look` as in look_args) and, on a
// handle with a stack, the stack kernel behind them (`reset_flags`, `op` as in launch_stack), on a handle with a point cloud its kernel, on one with a voxel grid its kernel, on
// one with a heightmap its kernel, on one with object boxes their kernel (it reads the planes alone: no camera, no look, no pose), and on one with surface normals their
// kernel, and on one with motion vectors their kernel last (a step measures, every other caller restarts: launch_flow)
static int frames_after(lcr_sim *s, const LcrDev &P, hipStream_t stream, const int *look, const unsigned char *reset_flags, int op, bool step = false) {
    LAUNCHCHK("render", launch_frames(s, P, stream, look));
    if (s->stack_on) LAUNCHCHK("stack kernel", launch_stack(s, stream, reset_flags, op, step));
    if (s->cloud_on) LAUNCHCHK("point-cloud kernel", launch_cloud(s, P, stream, look));
    if (s->voxel_on) LAUNCHCHK("voxel-grid kernel", launch_voxel(s, P, stream, look));
    if (s->height_on) LAUNCHCHK("heightmap kernel", launch_heightmap(s, P, stream, look));
    if (s->boxes_on) LAUNCHCHK("object-boxes kernel", lcr_launch_object_boxes(s->boxes, stream));
    if (s->normals_on) LAUNCHCHK("normals kernel", launch_normals(s, P, stream, look));
    if (s->flow_on) LAUNCHCHK("motion-vector kernel", launch_flow(s, P, stream, look, reset_flags, step));
    return LCR_OK;
}

// ---- the set-up path the observations made of the depth and segmentation planes share (the point cloud, the voxel grid, the heightmap, the object boxes, the normals) ----

// What every observation that needs BOTH planes asks of the handle, behind its argument checks: frames, both planes, and a wrist camera where `*cameras` selects one;
// *cameras == 0 becomes every camera the handle has.  The words name the observation in the refusals: there are no frames `of` ("to make a voxel grid of"), `needs` ("the
// voxel grid needs") both planes, enabled before `it` ("the grid").  (The object boxes need the segmentation plane alone and keep their own checks.)
static int planes_ready(const lcr_sim *s, uint32_t *cameras, const char *of, const char *needs, const char *it) {
    if (!s->has_images) return fail(LCR_ERR_INVALID, "sim has no image observations (observation_mode state): there are no frames %s", of);
    const uint32_t both = LCR_PLANE_DEPTH | LCR_PLANE_SEGMENTATION;
    if ((s->planes & both) != both)
        return fail(LCR_ERR_INVALID, "%s both image planes, depth and segmentation (lcr_enable_image_planes with planes = 3, before %s): %s", needs, it,
                    s->planes == 0 ? "none is enabled" : (s->planes & LCR_PLANE_DEPTH) ? "the segmentation plane is missing" : "the depth plane is missing");
    if (*cameras == 0) *cameras = LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | (s->wrist_on ? LCR_STACK_CAM_WRIST : 0);
    if ((*cameras & LCR_STACK_CAM_WRIST) && !s->wrist_on)
        return fail(LCR_ERR_INVALID, "cameras selects the wrist camera (4), but the sim has none (lcr_enable_wrist_camera, before the planes and %s)", it);
    return LCR_OK;
}

// a selected camera: where its pose comes from (LCR_CLOUD_CAM_*) and the planes and frames it draws.  The argument structs differ (the normals take no frames, the object
// boxes no camera and the depth as words), so every enable copies the fields its kernel has out of these
struct ObsSource {
    int cam;
    const unsigned char *seg;
    const float *depth;
    const unsigned char *rgb;
};
// the cameras `cameras` selects, in slot order front, top, wrist; returns how many
static int sources(const lcr_sim *s, uint32_t cameras, ObsSource (&src)[3]) {
    int n = 0;
    if (cameras & LCR_STACK_CAM_FRONT) src[n++] = ObsSource{LCR_CLOUD_CAM_FRONT, s->pl.seg_front, s->pl.depth_front, s->dev.img_front};
    if (cameras & LCR_STACK_CAM_TOP) src[n++] = ObsSource{LCR_CLOUD_CAM_TOP, s->pl.seg_top, s->pl.depth_top, s->dev.img_top};
    if (cameras & LCR_STACK_CAM_WRIST) src[n++] = ObsSource{LCR_CLOUD_CAM_WRIST, s->wrist.seg, s->wrist.depth, s->wrist.img};
    return n;
}

// The tail of every enable: the allocation C lays out (*mem), its first `guarded` bytes filled with the guard byte and the rest zeroed, then `first(base)` -- which points the
// kernel's arguments into the allocation, puts on the handle what the launch reads there and returns the first launch's status -- and a wait for it.  On a failure the
// allocation is freed and `undo()` takes back what first() put on the handle: LCR_ERR_OOM, LCR_ERR_HIP, or LCR_ERR_UNSUPPORTED for arguments the launcher refuses (a
// negative status), whose message is the caller's to word.  `what` ("the voxel grid") names the observation in the other two
template <class First, class Undo>
static int bring_up(lcr_sim *s, const Carver &C, size_t guarded, const char *what, void **mem, First first, Undo undo) {
    hipError_t e = hipMalloc(mem, C.off);
    if (e != hipSuccess) return fail(LCR_ERR_OOM, "hipMalloc(%zu bytes) for %s failed: %s", C.off, what, hipGetErrorString(e));
    char *base = (char *)*mem;
    int rc = (int)hipMemsetAsync(base, LCR_WRIST_GUARD_BYTE, guarded, s->stream);
    if (!rc && C.off > guarded) rc = (int)hipMemsetAsync(base + guarded, 0, C.off - guarded, s->stream);
    if (!rc) rc = first(base);
    if (rc < 0) (void)hipStreamSynchronize(s->stream);   // (the memsets are on their way: the allocation is not freed under them)
    else if (!rc) rc = (int)hipStreamSynchronize(s->stream);
    if (!rc) return LCR_OK;
    (void)hipFree(*mem);
    *mem = nullptr;
    undo();
    if (rc < 0) return LCR_ERR_UNSUPPORTED;   // (the caller says what the kernel is not built for)
    return fail(LCR_ERR_HIP, "making %s failed: %s", what, hipGetErrorString((hipError_t)rc));
}

// the wrist camera's mount with the ray scale of a frame `height` rows high (s = 2 tan(fovy / 2) / height in fp64, then rounded)
static LcrWristMount wrist_mount_at(const lcr_sim *s, int height) {
    LcrWristMount M = s->wrist.mount;
    M.s = (float)(2.0 * std::tan(0.5 * (double)s->wrist_cam.fovy_deg * M_PI / 180.0) / height);
    return M;
}
// the cameras a single-frame call accepts: 3 (the wrist camera) on a handle that has one
#define CAMCHK(s, camera)                                                                                                   \
    if ((camera) < 0 || (camera) > ((s)->wrist_on ? 3 : 2))                                                                 \
        return fail(LCR_ERR_INVALID, (s)->wrist_on ? "camera must be 0 (front), 1 (top), 2 (vizu) or 3 (wrist)" : "camera must be 0 (front), 1 (top) or 2 (vizu)")

static int join_render(lcr_sim *s) {
    if (s->rpending) {
        hipError_t e = hipStreamWaitEvent(s->stream, s->ev_rdone[s->rlast], 0);
        if (e != hipSuccess) return (int)e;
        s->rpending = false;
    }
    return 0;
}

// ---- the staging and the pass loop of the three terminal-frame calls (lcr_render_terminal, lcr_render_terminal_planes, lcr_render_terminal_wrist) ----
// one pass: `c` env ids to the device, their terminal poses gathered behind them and -- with a look -- their terminal looks.  P1: the c-env view of the handle over the
// gathered poses (the caller points its frame buffers into the staging), LK: the looks to draw it with
static int term_stage_gather(lcr_sim *s, const int32_t *ids_host, int c, char *base, size_t o_ids, size_t o_q, size_t o_t, size_t o_lk, LcrDev &P1, LcrLook &LK) {
    HIPCHK(hipMemcpyAsync(base + o_ids, ids_host, sizeof(int) * c, hipMemcpyHostToDevice, s->stream));
    LAUNCHCHK("gather", lcr_launch_gather_terminal(s->dev, (const int *)(base + o_ids), c, (float *)(base + o_q), (float *)(base + o_t), s->stream));
    P1 = s->dev;
    P1.n = c;
    P1.qpos = (float *)(base + o_q);
    P1.target = (float *)(base + o_t);
    LK = LcrLook{};
    if (s->look_K) {
        LAUNCHCHK("gather", lcr_launch_look_gather((const int *)(base + o_ids), c, s->dev.n, s->look_term, (int *)(base + o_lk), s->stream));
        LK = look_args(s, P1, (const int *)(base + o_lk));
    }
    return LCR_OK;
}

// The driver of the three calls, behind their own argument checks.  `per_env`: the bytes per env of each buffer the caller's frame kernel writes (0: a buffer it does not
// use).  The listed envs are drawn in passes of at most `cap` envs, as many as keep those buffers within the budget.  The staging -- the ids, the gathered poses, the
// caller's buffers at `cap` envs each, the gathered looks -- is laid out once and used again by every pass, a shorter last pass filling the front of each slice.  In each
// pass `pass(P1, LK, c, done, buf)` draws the `c` envs behind the first `done` ones: P1 and LK as term_stage_gather leaves them, buf[i] the device buffer of per_env[i]
// (null where that is 0); it launches its frame kernel and enqueues the copies into its host arrays at env `done`; the driver waits for them.
template <size_t NB, class Pass>
static int render_terminal_passes(lcr_sim *s, const int32_t *env_ids_host, int count, const size_t (&per_env)[NB], Pass pass) {
    for (int i = 0; i < count; i++)
        if (env_ids_host[i] < 0 || env_ids_host[i] >= s->dev.n) return fail(LCR_ERR_INVALID, "env id %d out of range", env_ids_host[i]);
    size_t env_bytes = 0;
    for (size_t b : per_env) env_bytes += b;
    const size_t BUDGET = (size_t)450 << 20;   // bytes of frame staging per pass: 1 024 envs of two colour frames at 320 x 240 (2 x 225 KiB each), 19 200 at 64 x 64
    const size_t chunk = BUDGET / env_bytes;
    const int cap = (size_t)count < chunk ? count : (int)chunk;
    if (cap == 0) return LCR_OK;
    Carver C;
    const size_t o_ids = C.take(sizeof(int) * cap);
    const size_t o_q = C.take(sizeof(float) * s->nq * cap);
    const size_t o_t = C.take(sizeof(float) * 3 * cap);
    size_t o_buf[NB];
    for (size_t i = 0; i < NB; i++) o_buf[i] = C.take(per_env[i] * cap);
    const size_t o_lk = C.take(s->look_K ? sizeof(int) * 10 * cap : 0);   // the terminal looks of the listed envs
    if (int rc = reserve(&s->term_stage, &s->term_stage_bytes, C.off)) return rc;
    char *base = (char *)s->term_stage, *buf[NB];
    for (size_t i = 0; i < NB; i++) buf[i] = per_env[i] ? base + o_buf[i] : nullptr;
    for (int done = 0; done < count; done += cap) {
        const int c = count - done < cap ? count - done : cap;
        LcrDev P1;   // a `c`-env view of the handle whose state arrays are the gathered terminal poses
        LcrLook LK;  // ... drawn, with a look, as the episodes that ended looked
        if (int rc = term_stage_gather(s, env_ids_host + done, c, base, o_ids, o_q, o_t, o_lk, P1, LK)) return rc;
        if (int rc = pass(P1, LK, c, (size_t)done, buf)) return rc;
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    return LCR_OK;
}

extern "C" {

int lcr_abi_version(void) { return LCR_ABI_VERSION; }
const char *lcr_last_error(void) { return g_err; }

int lcr_nq(int task) { return task == LCR_TASK_STACK ? 20 : 13; }
int lcr_nv(int task) { return task == LCR_TASK_STACK ? 18 : 12; }

// the reference constructor defaults + the rounds 1-4 solver settings (LCR_PRESET_FAST); lcr_config_preset builds on it
static int config_base(lcr_config *cfg, int task) {
    if (!cfg) return fail(LCR_ERR_INVALID, "cfg is NULL");
    if (task < LCR_TASK_REACH || task > LCR_TASK_PUSH_LOOP) return fail(LCR_ERR_INVALID, "unknown task %d", task);
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof(lcr_config);
    cfg->task = task;
    cfg->n_envs = 1;
    cfg->device = 0;
    cfg->env_id_offset = 0;
    cfg->action_mode = LCR_ACTION_JOINT;   // reach_cube_env.py:80
    cfg->obs_mode = LCR_OBS_IMAGE;         // reach_cube_env.py:79 (the reference default is "image")
    cfg->reward_type = LCR_REWARD_SPARSE;  // reach_cube_env.py:81
    cfg->block_gripper = -1;
    cfg->distance_threshold = 0.05;
    cfg->cube_xy_range = 0.3;
    cfg->target_xy_range = 0.3;
    cfg->goal_z_range = 0.1;
    cfg->height_threshold = 0.1;
    cfg->impratio = 100.0;
    cfg->n_substeps = 20;
    cfg->max_episode_steps = 50;
    cfg->pgs_iters = 4;
    cfg->compat = 0;
    cfg->auto_reset = 1;
    cfg->arm_collision = 1;
    cfg->base_seed = 0;
    cfg->pgs_tol = 1e-6;
    // rolling rows of the finger<->cube contacts: on where their effect on a touched cube within one control step exceeds the fp32
    // parity tolerance in the median (tools/condim6_effect.py: PushCubeLoop 1.4e-2 -- rolling coefficient 1.5 m, push_cube_loop.xml:31;
    // StackTwoCubes 4e-4 -- default coefficient 1e-4 m but cube inertia 1.1e-5), off where it does not (<= 4e-5: deviation D4)
    cfg->finger_cube_condim = (task == LCR_TASK_PUSH_LOOP || task == LCR_TASK_STACK) ? 6 : 4;
    cfg->diagnostics = 0;
    cfg->step_kernel = 0;
    cfg->cc_points = 0;
    cfg->global_envs = 0;   // this handle is the whole job
    cfg->solver = LCR_SOLVER_PGS;
    cfg->newton_iters = 30;
    cfg->ls_iters = 8;
    cfg->finger_floor_condim = 0;
    cfg->newton_tol = 1e-6;
    cfg->ls_tol = 1e-2;   // (MuJoCo's own default: ls_tolerance 0.01; measured on the oracle: a sixth fewer evaluations of phi', same distance to the exact optimum)
    return LCR_OK;
}

int lcr_config_default(lcr_config *cfg, int task) { return lcr_config_preset(cfg, task, LCR_PRESET_FAITHFUL); }

int lcr_config_preset(lcr_config *cfg, int task, int preset) {
    if (preset != LCR_PRESET_FAITHFUL && preset != LCR_PRESET_FAST) return fail(LCR_ERR_INVALID, "unknown preset %d", preset);
    const int rc = config_base(cfg, task);
    if (rc != LCR_OK) return rc;
    if (preset == LCR_PRESET_FAITHFUL) {
        cfg->solver = LCR_SOLVER_NEWTON;
        cfg->finger_cube_condim = 6;
        cfg->finger_floor_condim = 6;
        cfg->cc_points = task == LCR_TASK_STACK ? 8 : 0;
    } else {
        cfg->solver = LCR_SOLVER_PGS;
        cfg->finger_floor_condim = 4;
    }
    return LCR_OK;
}

// the two-wave kernels implement neither the converged solver mode nor the per-wave cycle read-back of diagnostics = 2
static bool two_wave_possible(const lcr_config *cfg) { return cfg->pgs_iters >= 0 && cfg->diagnostics != 2; }

static int resolved_block_gripper(const lcr_config *cfg) {
    if (cfg->block_gripper >= 0) return cfg->block_gripper ? 1 : 0;
    return (cfg->task == LCR_TASK_REACH || cfg->task == LCR_TASK_PUSH || cfg->task == LCR_TASK_PUSH_LOOP) ? 1 : 0;  // reach:82 push:84 loop:80 / lift:82
}

int lcr_action_dim(const lcr_config *cfg) {
    if (!cfg) return fail(LCR_ERR_INVALID, "cfg is NULL");
    if (cfg->action_mode != LCR_ACTION_JOINT && cfg->action_mode != LCR_ACTION_EE)
        return fail(LCR_ERR_INVALID, "Invalid action mode, must be 'ee' or 'joint'");
    return (cfg->action_mode == LCR_ACTION_EE ? 3 : 5) + (resolved_block_gripper(cfg) ? 0 : 1);
}

int lcr_create(const lcr_config *cfg, lcr_sim **out) {
    if (!cfg || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(lcr_config))
        return fail(LCR_ERR_INVALID, "lcr_config size mismatch (got %u, want %zu): ABI version skew", cfg->struct_size, sizeof(lcr_config));
    if (cfg->task < LCR_TASK_REACH || cfg->task > LCR_TASK_PUSH_LOOP) return fail(LCR_ERR_INVALID, "unknown task %d", cfg->task);
    if (cfg->n_envs <= 0) return fail(LCR_ERR_INVALID, "n_envs must be positive");
    // the kernels index [component][env] arrays with 32-bit products (20 components at most): keep 20 * n_envs < 2^31
    if (cfg->n_envs > (1 << 26)) return fail(LCR_ERR_INVALID, "n_envs %d exceeds 67108864 per handle; shard the batch over several handles", cfg->n_envs);
    if (cfg->n_substeps <= 0) return fail(LCR_ERR_INVALID, "n_substeps must be positive");
    if (cfg->pgs_iters < 0 && !(cfg->pgs_tol > 0)) return fail(LCR_ERR_INVALID, "pgs_tol must be positive in converged mode (pgs_iters < 0)");
    if (cfg->finger_cube_condim != 0 && cfg->finger_cube_condim != 4 && cfg->finger_cube_condim != 6) return fail(LCR_ERR_INVALID, "finger_cube_condim must be 4 or 6");
    if (cfg->cc_points != 0 && cfg->cc_points != 4 && cfg->cc_points != 8) return fail(LCR_ERR_INVALID, "cc_points must be 4 or 8");
    if (cfg->coop_share < 0 || cfg->coop_share > 5) return fail(LCR_ERR_INVALID, "coop_share must be 0 (default), 1 (owner only), 2 (shared), 3 (always hand off), 4 (ahead) or 5 (early)");
    // frame size: both zero (320 x 240) or each a multiple of 4 in [16, 512] (lcr.h: 16-byte aligned bands, one 32-bit mask of tile columns); checked whatever obs_mode is
    if ((cfg->image_width == 0) != (cfg->image_height == 0)) return fail(LCR_ERR_INVALID, "image_width and image_height must both be 0 (320 x 240) or both be set (got %d x %d)", cfg->image_width, cfg->image_height);
    if (cfg->image_width != 0 && (cfg->image_width < 16 || cfg->image_width > 512 || cfg->image_width % 4 != 0)) return fail(LCR_ERR_INVALID, "image_width must be a multiple of 4 in [16, 512] (got %d)", cfg->image_width);
    if (cfg->image_height != 0 && (cfg->image_height < 16 || cfg->image_height > 512 || cfg->image_height % 4 != 0)) return fail(LCR_ERR_INVALID, "image_height must be a multiple of 4 in [16, 512] (got %d)", cfg->image_height);
    if (cfg->cc_points == 8 && cfg->task != LCR_TASK_STACK) return fail(LCR_ERR_INVALID, "cc_points = 8 is the cube<->cube manifold of StackTwoCubes; this task has one cube");
    if (cfg->cc_points == 8 && cfg->pgs_iters < 0) return fail(LCR_ERR_UNSUPPORTED, "cc_points = 8 is implemented by the two-wave kernels, the converged solver mode (pgs_iters < 0) by the one-wave kernels");
    if (cfg->step_kernel < 0 || cfg->step_kernel > 2) return fail(LCR_ERR_INVALID, "step_kernel must be 0 (by task and job size), 1 (one wave per 64 envs) or 2 (two cooperating waves)");
    if (cfg->diagnostics < 0 || cfg->diagnostics > 3) return fail(LCR_ERR_INVALID, "diagnostics must be 0, 1 (decision signature), 2 or 3 (per-wave cycle read-back, profiling)");
    // combinations no kernel implements are refused, not silently degraded
    if (cfg->cc_points == 8 && cfg->solver == LCR_SOLVER_PGS && cfg->diagnostics == 2) return fail(LCR_ERR_UNSUPPORTED, "cc_points = 8 runs on the two-wave kernels, diagnostics = 2 (per-wave cycles) on the one-wave kernels");
    if (cfg->cc_points == 8 && cfg->solver == LCR_SOLVER_PGS && cfg->step_kernel == 1) return fail(LCR_ERR_UNSUPPORTED, "cc_points = 8 is implemented by the two-wave kernels only (step_kernel = 1 pins the one-wave family)");
    if (cfg->step_kernel == 2 && cfg->pgs_iters < 0) return fail(LCR_ERR_UNSUPPORTED, "the converged solver mode (pgs_iters < 0) is implemented by the one-wave kernels only (step_kernel = 2 pins the two-wave family)");
    if (cfg->step_kernel == 2 && cfg->task == LCR_TASK_PUSH_LOOP) return fail(LCR_ERR_UNSUPPORTED, "PushCubeLoop has the one-wave step kernel only (lcr_kernels.hip); step_kernel = 2 pins the two-wave family");
    if (cfg->step_kernel == 2 && cfg->diagnostics == 2) return fail(LCR_ERR_UNSUPPORTED, "diagnostics = 2 (per-wave cycles) reads back the one-wave kernels only (step_kernel = 2 pins the two-wave family)");
    if (cfg->solver != LCR_SOLVER_PGS && cfg->solver != LCR_SOLVER_NEWTON) return fail(LCR_ERR_INVALID, "solver must be LCR_SOLVER_PGS (0) or LCR_SOLVER_NEWTON (1)");
    if (cfg->finger_floor_condim != 0 && cfg->finger_floor_condim != 4 && cfg->finger_floor_condim != 6) return fail(LCR_ERR_INVALID, "finger_floor_condim must be 4 or 6");
    if (cfg->solver == LCR_SOLVER_NEWTON) {
        if (cfg->newton_iters <= 0 || cfg->ls_iters <= 0 || !(cfg->newton_tol > 0) || !(cfg->ls_tol > 0)) return fail(LCR_ERR_INVALID, "newton_iters, ls_iters, newton_tol and ls_tol must be positive");
        if (cfg->finger_cube_condim == 4 || cfg->finger_floor_condim == 4) return fail(LCR_ERR_UNSUPPORTED, "the Newton kernels carry six-row finger contacts (finger_cube_condim = finger_floor_condim = 6)");
        if (cfg->step_kernel == 2) return fail(LCR_ERR_UNSUPPORTED, "the Newton kernels are one-wave kernels (step_kernel = 2 pins the two-wave family)");
        if (cfg->pgs_iters < 0) return fail(LCR_ERR_INVALID, "pgs_iters < 0 (converged sweeps) belongs to LCR_SOLVER_PGS");
        if (cfg->diagnostics == 3) return fail(LCR_ERR_UNSUPPORTED, "the per-phase cycle read-back (diagnostics = 3) belongs to the two-wave sweep kernels");
    } else if (cfg->finger_floor_condim == 6) return fail(LCR_ERR_UNSUPPORTED, "six-row finger<->floor contacts are implemented by the Newton kernels (solver = LCR_SOLVER_NEWTON)");
    if (cfg->global_envs < 0) return fail(LCR_ERR_INVALID, "global_envs must be >= 0 (0 = n_envs)");
    if (cfg->global_envs > 0 && (cfg->env_id_offset < 0 || cfg->env_id_offset + (int64_t)cfg->n_envs > cfg->global_envs))
        return fail(LCR_ERR_INVALID, "shard [env_id_offset, env_id_offset + n_envs) = [%lld, %lld) does not lie inside the job of global_envs = %lld",
                    (long long)cfg->env_id_offset, (long long)(cfg->env_id_offset + cfg->n_envs), (long long)cfg->global_envs);
    // A wave (64 consecutive env ids) takes its shortcuts -- slots no lane touches, the coupled lanes it solves cooperatively, the exits of the solver loops -- for all of
    // its lanes at once, so the low-order bits of an env's result depend on which envs share its wave.  "Identical bits for every sharding of a job" (lcr.h) therefore
    // requires that shards are cut at wave boundaries: a shard of a larger job starts at a multiple of 64 and, unless it is the job's last, holds a multiple of 64 envs.
    {
        const bool last = cfg->global_envs <= 0 || cfg->env_id_offset + (int64_t)cfg->n_envs == cfg->global_envs;   // (no job declared: the handle is the job's only or last shard)
        if (cfg->env_id_offset % 64 != 0 || (!last && cfg->n_envs % 64 != 0))
            return fail(LCR_ERR_INVALID, "shard [%lld, %lld) of a job of %lld envs is not cut at wave boundaries: env_id_offset and (except for the last shard) n_envs must be multiples of 64 (lcr.h: global_envs)",
                        (long long)cfg->env_id_offset, (long long)(cfg->env_id_offset + cfg->n_envs), (long long)cfg->global_envs);
    }
    if (cfg->obs_mode < LCR_OBS_IMAGE || cfg->obs_mode > LCR_OBS_BOTH) return fail(LCR_ERR_INVALID, "invalid observation_mode");
    if (cfg->reward_type != LCR_REWARD_SPARSE && cfg->reward_type != LCR_REWARD_DENSE) return fail(LCR_ERR_INVALID, "invalid reward_type");
    int k = lcr_action_dim(cfg);
    if (k < 0) return k;
    const bool gripper_task = !(cfg->task == LCR_TASK_REACH || cfg->task == LCR_TASK_PUSH || cfg->task == LCR_TASK_PUSH_LOOP);
    if (cfg->action_mode == LCR_ACTION_EE && gripper_task && resolved_block_gripper(cfg))
        return fail(LCR_ERR_INVALID, "ee mode with block_gripper on a gripper task indexes action[3] out of range in the reference (lift_cube_env.py:242)");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(LCR_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(LCR_ERR_INVALID, "device %d out of range (have %d)", cfg->device, ndev);
    HIPCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(LCR_ERR_NO_DEVICE, "device %d is %s; the kernels are built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);

    lcr_sim *s = new (std::nothrow) lcr_sim();
    if (!s) return fail(LCR_ERR_OOM, "host allocation failed");
    memset(s, 0, sizeof *s);
    s->cfg = *cfg;
    s->cfg.block_gripper = resolved_block_gripper(cfg);
    s->nq = lcr_nq(cfg->task);
    s->nv = lcr_nv(cfg->task);
    s->k = k;
    s->ee_mode = cfg->action_mode == LCR_ACTION_EE;
    s->stream = nullptr;
    s->has_images = cfg->obs_mode != LCR_OBS_STATE;
    const size_t N = (size_t)cfg->n_envs;

    // ---- one arena for all SoA arrays (256-B aligned slices) ----
    Carver C;
    const size_t o_qpos = C.take(sizeof(float) * s->nq * N);
    const size_t o_qvel = C.take(sizeof(float) * s->nv * N);
    const size_t o_ee = C.take(sizeof(float) * 3 * N);
    const size_t o_tgt = C.take(sizeof(float) * 3 * N);
    // step outputs follow the observable state directly: [qpos .. did_reset] is ONE contiguous range, fetched by lcr_fetch_host
    // with a single device-to-host copy (the terminal observations behind it only when some env was reset)
    const size_t o_rew = C.take(sizeof(float) * N);
    const size_t o_term = C.take(N);
    const size_t o_trunc = C.take(N);
    const size_t o_succ = C.take(N);
    const size_t o_dres = C.take(N);
    const size_t o_fetch_end = C.off;
    const size_t o_tobs = C.take(sizeof(float) * LCR_OBS_DIM * N);
    const size_t o_tquat = C.take(sizeof(float) * 8 * N);
    const size_t o_tobs_end = C.off;
    const size_t o_el = C.take(sizeof(int) * N);
    const size_t o_rng = C.take(sizeof(unsigned long long) * 4 * N);
    const size_t o_goal = C.take(sizeof(int) * N);
    const size_t o_time = C.take(sizeof(double) * N);
    const size_t diag_on = cfg->diagnostics ? 1 : 0;   // the diagnostics arrays take room only when they are asked for
    const size_t o_dmask = C.take(diag_on * sizeof(unsigned) * N);
    const size_t o_dcount = C.take(diag_on * sizeof(unsigned) * N);
    const size_t o_dsweeps = C.take(diag_on * sizeof(unsigned) * N);
    const size_t o_dchoice = C.take(diag_on * sizeof(unsigned) * N);
    const size_t o_dctrl = C.take(diag_on * sizeof(float) * 6 * N);
    // scratch: Stack on the one-wave kernels keeps the g rows of the arm-link proxy slot (+ the rolling rows of the finger slots) here, 24 / 48 floats per env;
    // the two-wave kernels compiled for two waves per SIMD hand Wm = (M + hD)^-1 L from the cube wave to the arm wave through it in substeps with a finger on
    // a cube, 36 floats per lane of every (64-lane) workgroup
    const size_t o_scr = C.take(sizeof(float) * 48 * (((N + 63) / 64) * 64));
    const bool carry_warm = !(cfg->compat & LCR_COMPAT_COLD_SOLVE_EACH_STEP);
    const size_t o_warm = C.take(carry_warm ? sizeof(float) * LCR_NWARM * N : 0);   // constraint forces carried between control steps
    const size_t o_act = C.take(sizeof(float) * 6 * N);
    const size_t o_mask = C.take(N);
    const size_t o_seeds = C.take(sizeof(unsigned long long) * N);
    const int img_w = cfg->image_width ? cfg->image_width : LCR_IMG_W, img_h = cfg->image_height ? cfg->image_height : LCR_IMG_H;
    const size_t img_bytes = (size_t)img_h * img_w * 3;
    const size_t o_img0 = C.take(s->has_images ? img_bytes * N : 0);
    const size_t o_img1 = C.take(s->has_images ? img_bytes * N : 0);
    const size_t o_bg = C.take(s->has_images ? 2 * img_bytes : 0);
    // one-cube Newton kernel: a flag per wave, for the launch that repeats the control step of waves the fast-copy-only kernel gave up on (lcr_kernels.hip: STEP_FAST_ONLY).
    // The workgroup's four waves read their four words: rounded up; the words of waves past the last env stay zero
    const bool redo_wg = cfg->solver == LCR_SOLVER_NEWTON && cfg->task != LCR_TASK_STACK && cfg->task != LCR_TASK_PUSH_LOOP;
    const size_t redo_words = redo_wg ? ((N + 255) / 256) * 4 : 0;
    const size_t o_redo = C.take(sizeof(int) * redo_words);
    const size_t off = C.off;
    s->arena_bytes = off;
    s->fetch_bytes = o_fetch_end;
    s->tobs_off = o_tobs;
    s->tobs_bytes = o_tobs_end - o_tobs;
    s->host_mirror = nullptr;
    e = hipMalloc(&s->arena, off);
    if (e != hipSuccess) { lcr_destroy(s); return fail(LCR_ERR_OOM, "hipMalloc(%zu bytes) failed: %s", off, hipGetErrorString(e)); }
    e = hipMemset(s->arena, 0, off);
    if (e != hipSuccess) { lcr_destroy(s); return fail(LCR_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e)); }
    char *base = (char *)s->arena;

    LcrDev &D = s->dev;
    D.n = cfg->n_envs;
    D.k = k;
    D.task = cfg->task;
    D.n_substeps = cfg->n_substeps;
    D.max_steps = cfg->max_episode_steps;
    D.pgs_iters = cfg->pgs_iters;
    D.auto_reset = cfg->auto_reset ? 1 : 0;
    D.gripper_active = gripper_task ? 1 : 0;
    D.reward_type = cfg->reward_type;
    D.has_target = (cfg->task == LCR_TASK_PUSH || cfg->task == LCR_TASK_PICK_PLACE) ? 1 : 0;
    D.compat = cfg->compat;
    D.env_off = cfg->env_id_offset;
    D.dist_thr = (float)cfg->distance_threshold;
    D.height_thr = (float)cfg->height_threshold;
    D.inv_impratio = (float)(1.0 / (cfg->impratio > 1e-15 ? cfg->impratio : 1e-15));
    // scene constants: reach/lift/push cube 0.1 kg, I=1.6667e-4 (reach_cube.xml:25); pick_place 10 kg (pick_place_cube.xml:27);
    // stack 0.1 kg, I=1.125e-5 (stack_two_cubes.xml:27,33)
    // push_cube_loop.xml:29-31: 0.05 kg, I=1.125e-5, friction 1.5 / 1.5 (torsional)
    const bool loop = cfg->task == LCR_TASK_PUSH_LOOP;
    // (numbers from the scene files via tests/golden/model_golden.json -> lcr_model_gen.h)
    double cm = lcrm::SCENE_CUBE_MASS[cfg->task];
    double ci = lcrm::SCENE_CUBE_INERTIA[cfg->task];
    {
        const double mu = lcrm::SCENE_CUBE_MU[cfg->task], mut = lcrm::SCENE_CUBE_MU_TORS[cfg->task];   // cube geom friction (tangential, torsional)
        const double muf = mu > 1.5 ? mu : 1.5, muft = mut > 0.005 ? mut : 0.005;   // finger<->cube pair (both priority 1): max of both geoms (finger: follower.xml:15)
        D.rt_cube = (float)(mu * mu / (mut * mut));
        D.inv_mu_c2 = (float)(1.0 / (mu * mu));
        D.inv_mu_ct2 = (float)(1.0 / (mut * mut));
        D.rt_fc = (float)(muf * muf / (muft * muft));
        D.inv_mu_fct2 = (float)(1.0 / (muft * muft));
        const double mur = lcrm::SCENE_CUBE_MU_ROLL[cfg->task], mufr = mur > 0.0001 ? mur : 0.0001;   // rolling: max(cube, finger default 1e-4)
        D.rr_fc = (float)(muf * muf / (mufr * mufr));
        D.inv_mu_fcr2 = (float)(1.0 / (mufr * mufr));
        D.mu_c2 = (float)(mu * mu); D.mu_ct2 = (float)(mut * mut);
        D.mu_fc2 = (float)(muf * muf); D.mu_fct2 = (float)(muft * muft); D.mu_fcr2 = (float)(mufr * mufr);
        const bool roll_default = loop || cfg->task == LCR_TASK_STACK;
        D.roll = (cfg->finger_cube_condim == 6 || (cfg->finger_cube_condim == 0 && roll_default)) ? 1 : 0;   // 0 = the task's default
        // Stack shards of at most three waves per CU (MI355X: up to 49 152 envs; BASELINE config 5's per-GPU size is 32 768) run the kernel
        // variant that keeps every g row in LDS (46 / 52 KiB per wave, 3 x 52 <= 160 KiB); LCR_STACK_LDS=small|big overrides the choice
        // (tests exercise both variants at small sizes)
        D.big_lds = (cfg->task == LCR_TASK_STACK && (N + 63) / 64 <= 3 * (size_t)prop.multiProcessorCount) ? 1 : 0;
        if (const char *ov = getenv("LCR_STACK_LDS")) { if (cfg->task == LCR_TASK_STACK) D.big_lds = strcmp(ov, "big") == 0 ? 1 : (strcmp(ov, "small") == 0 ? 0 : D.big_lds); }
        D.walls = loop ? 1 : 0;
        // step-kernel family: a function of the task, the config and the size of the JOB (lcr_config.global_envs; 0 = this handle is the job) -- never of
        // the shard size, so that every sharding of a job runs the same arithmetic (bit-identical results for G = 1/2/4/8).  Measured on an
        // MI355X with the job as ONE shard (random policy, round 4): the two-cooperating-waves kernels win at every size for the
        // four one-cube tasks without rails (65 536 envs: ReachCube 0.257 against 0.285 ms, Push / Lift / PickPlace 0.308-0.312 against 0.333-0.336;
        // 32 768: 0.205-0.229 against 0.33) -- those tasks ALWAYS run them.  StackTwoCubes needs more than 256 registers per lane in its waves: up to
        // 32 768 envs (2 x 512 waves: one per SIMD) the two-wave kernels win (0.43 against 0.70 ms), above that one round of one-wave workgroups beats two
        // rounds of two-wave ones (65 536: 0.78 against 0.82).  PushCubeLoop has one kernel (lcr_kernels.hip, WALLS: one wave per 64 envs).
        // lcr_config.step_kernel pins a family (a Stack job cut into shards of <= 32 768 envs pins 2); LCR_STEP_KERNEL=single|coop1|coop2 overrides
        // (tests and profiling exercise every build).
        // WHICH BUILD of the two-wave family a shard runs does follow its size (one wave per SIMD while 2 x ceil(N / 64) waves fit the chip's SIMDs, else the
        // build compiled for two waves per SIMD): same source, same bits.
        {
            const size_t waves2 = 2 * ((N + 63) / 64), simds = 4 * (size_t)prop.multiProcessorCount;
            const int64_t job = cfg->global_envs > 0 ? cfg->global_envs : (int64_t)N;
            D.cc8 = (cfg->task == LCR_TASK_STACK && cfg->cc_points == 8) ? 1 : 0;
            // StackTwoCubes: two-wave workgroups while the JOB's 2 x job / 64 waves fit one per SIMD -- 32 envs per SIMD of the part the job runs on (MI355X: 1 024 SIMDs
            // -> 32 768 envs).  Every shard of a job runs on the same part and declares the same global_envs: the same family on all of them
            const int64_t stack_two_wave_max = 32 * (int64_t)simds;
            bool two_wave = job <= stack_two_wave_max || cfg->task != LCR_TASK_STACK;
            if (cfg->step_kernel == 1) two_wave = false;
            else if (cfg->step_kernel == 2) two_wave = true;
            if (D.cc8) two_wave = true;                               // the eight-point manifold lives in the two-wave kernels only
            if (cfg->pgs_iters < 0 || cfg->diagnostics == 2) two_wave = false;   // converged solver mode, per-wave cycle read-back: one-wave kernels only
            D.coop = two_wave ? (waves2 <= simds ? 1 : 2) : 0;
            if (const char *ov = getenv("LCR_STEP_KERNEL")) {
                if (strcmp(ov, "single") == 0 && !D.cc8) D.coop = 0;
                else if (strcmp(ov, "coop1") == 0 && two_wave_possible(cfg)) D.coop = 1;
                else if (strcmp(ov, "coop2") == 0 && two_wave_possible(cfg)) D.coop = 2;
            }
            if (D.cc8) D.coop = 1;   // (74-80 KiB of LDS per workgroup: its only build is the one-wave-per-SIMD one)
            if (loop) D.coop = 0;    // PushCubeLoop: one kernel
            D.newton = cfg->solver == LCR_SOLVER_NEWTON ? 1 : 0;
            D.newton_iters = cfg->newton_iters; D.ls_iters = cfg->ls_iters;
            D.newton_tol = (float)cfg->newton_tol; D.ls_tol = (float)cfg->ls_tol;
            D.coop_share = cfg->coop_share == 0 ? 4 : cfg->coop_share - 1;   // (one-cube Newton kernel: who solves a wave's coupled envs; the bits do not depend on it.  Default: early)
            // coupled envs a wave of the Newton kernels solves cooperatively (lcr_newton_coop.h: four per pass, one per 16-lane row; StackTwoCubes' three-body patients one at a time)
            // before it falls back to the coupled SIMT solves: 8 with one cube (two passes; flat beyond), 16 with rails and for Stack (PushCubeLoop 5.52 / 4.91 / 4.90 ms at 4 / 8 / 16: the
            // fall-back's 12-dim SIMT iteration spills; Stack's 18-dim one 3 KB per lane: profiles/r06_coop_sweep.txt, r06_coop_sweep2.txt); measurement override: LCR_COOP_MAX (0: never)
            D.coop_max = (cfg->task == LCR_TASK_STACK || loop) ? 16 : 8;
            if (const char *cm_ov = getenv("LCR_COOP_MAX")) D.coop_max = atoi(cm_ov) < 0 ? 0 : (atoi(cm_ov) > 64 ? 64 : atoi(cm_ov));
            if (D.newton) { D.coop = 0; D.roll = 1; D.big_lds = 1; }   // the Newton kernels: one wave per 64 envs, six-row finger slots, every g row in LDS (cc8: slots 4-7 of their eight cube<->cube records)
        }
    }
    D.arm_collision = cfg->arm_collision ? 1 : 0;
    D.diag = cfg->diagnostics;   // 2: max_sweeps carries the wave's cycle count instead (profiling aid, one-wave kernels); 3: per-wave phase cycles of the two-wave kernels
    D.pgs_tol = (float)cfg->pgs_tol;
    D.cube_mass = (float)cm;
    D.cube_minv = (float)(1.0 / cm);
    D.cube_iinv = (float)(1.0 / ci);
    {   // reach_cube_env.py:132-139, push_cube_env.py:141-148, pick_place_cube_env.py:143-150 -- same fp64 expressions
        double lo[3] = {-cfg->cube_xy_range / 2, -cfg->cube_xy_range / 2, 0}, hi[3] = {cfg->cube_xy_range / 2, cfg->cube_xy_range / 2, 0};
        lo[1] += 0.165; hi[1] += 0.10;
        double tl[3] = {-cfg->target_xy_range / 2, -cfg->target_xy_range / 2, 0};
        double th[3] = {cfg->target_xy_range / 2, cfg->target_xy_range / 2, cfg->task == LCR_TASK_PICK_PLACE ? cfg->goal_z_range : 0.0};
        tl[1] += 0.165; th[1] += 0.10;
        if (loop) {  // push_cube_loop_env.py:130-135 with push_cube_loop.xml:38: goal_region_high = size/2, [:2] -= 0.008, low = high*(-1,-1,1)
            double gh[3] = {0.035 / 2, 0.045 / 2, 0.007 / 2};
            gh[0] -= 0.008; gh[1] -= 0.008;
            for (int i = 0; i < 3; i++) { hi[i] = gh[i]; lo[i] = gh[i] * (i < 2 ? -1.0 : 1.0); }
        }
        for (int i = 0; i < 3; i++) { D.cube_lo[i] = lo[i]; D.cube_rng[i] = hi[i] - lo[i]; D.tgt_lo[i] = tl[i]; D.tgt_rng[i] = th[i] - tl[i]; }
    }
    D.qpos = (float *)(base + o_qpos);
    D.qvel = (float *)(base + o_qvel);
    D.ee_lag = (float *)(base + o_ee);
    D.target = (float *)(base + o_tgt);
    D.elapsed = (int *)(base + o_el);
    D.rng = (unsigned long long *)(base + o_rng);
    D.goal = (int *)(base + o_goal);
    D.sim_time = (double *)(base + o_time);
    D.reward = (float *)(base + o_rew);
    D.terminated = (unsigned char *)(base + o_term);
    D.truncated = (unsigned char *)(base + o_trunc);
    D.is_success = (unsigned char *)(base + o_succ);
    D.did_reset = (unsigned char *)(base + o_dres);
    D.term_obs = (float *)(base + o_tobs);
    D.term_quat = (float *)(base + o_tquat);
    D.active_mask = cfg->diagnostics ? (unsigned *)(base + o_dmask) : nullptr;
    D.active_count = cfg->diagnostics ? (unsigned *)(base + o_dcount) : nullptr;
    D.max_sweeps = cfg->diagnostics ? (unsigned *)(base + o_dsweeps) : nullptr;
    D.choice = cfg->diagnostics ? (unsigned *)(base + o_dchoice) : nullptr;
    D.ctrl_out = cfg->diagnostics ? (float *)(base + o_dctrl) : nullptr;
    D.scratch = (float *)(base + o_scr);
    D.warm = carry_warm ? (float *)(base + o_warm) : nullptr;
    s->redo.flags = redo_words ? (int *)(base + o_redo) : nullptr;
    s->redo.gate = redo_words ? 1 : 0;
    if (const char *ov = getenv("LCR_REDO_KERNEL")) { if (atoi(ov) == 0) s->redo.gate = 0; }   // (A/B runs and tests: the kernel with both substep copies alone, as before the pair)
    s->redo_words = redo_words;
    D.img_front = s->has_images ? (unsigned char *)(base + o_img0) : nullptr;
    D.img_top = s->has_images ? (unsigned char *)(base + o_img1) : nullptr;
    D.img_bg = s->has_images ? (unsigned char *)(base + o_bg) : nullptr;
    D.img_w = img_w; D.img_h = img_h;
    D.img_epw = lcr_render_envs_per_workgroup(img_w, img_h);
    if (const char *ov = getenv("LCR_RENDER_EPW")) { const int v = atoi(ov); if (v == 1 || v == 2 || v == 4) D.img_epw = v; }   // (measurement: tools/frame_sizes.py; frames wider than 170 px have the one mapping)
    make_cameras(cfg->task, img_h, s->cam_front, s->cam_top, s->cam_vizu);
    s->render_dev = nullptr;
    s->render_bytes = 0;
    s->term_stage = nullptr;
    s->term_stage_bytes = 0;
    s->action_stage = (float *)(base + o_act);
    s->mask_dev = (unsigned char *)(base + o_mask);
    s->seeds_dev = (unsigned long long *)(base + o_seeds);
    e = hipEventCreate(&s->ev0);
    if (e == hipSuccess) e = hipEventCreate(&s->ev1);
    if (e != hipSuccess) { lcr_destroy(s); return fail(LCR_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e)); }

    // initial state: reset of seed (base_seed + global env id) for every env
    int rc = lcr_launch_reset(D, nullptr, nullptr, 1, cfg->base_seed, s->stream);
    if (rc) { lcr_destroy(s); return fail(LCR_ERR_HIP, "reset kernel launch failed: %s", hipGetErrorString((hipError_t)rc)); }
    if (s->has_images) {
        lcr_launch_render_bg(D, s->cam_front, s->cam_top, s->stream);
        lcr_launch_render_obs(D, s->cam_front, s->cam_top, s->stream);
    }
    e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) { lcr_destroy(s); return fail(LCR_ERR_HIP, "initial reset failed: %s", hipGetErrorString(e)); }
    // the second stream of the frames (see lcr_sim); LCR_RENDER_OVERLAP=0: frames on the caller's stream, after the step kernel (A/B, profiling of one kernel at a time)
    const char *ro = getenv("LCR_RENDER_OVERLAP");
    if (s->has_images && !(ro && atoi(ro) == 0)) {
        e = hipStreamCreateWithFlags(&s->rstream, hipStreamNonBlocking);
        for (int p = 0; p < 2 && e == hipSuccess; p++) {
            e = hipEventCreateWithFlags(&s->ev_snap[p], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_rdone[p], hipEventDisableTiming);
            if (e == hipSuccess) e = hipMalloc((void **)&s->snap_qpos[p], sizeof(float) * (size_t)s->nq * N);
            if (e == hipSuccess) e = hipMalloc((void **)&s->snap_target[p], sizeof(float) * 3 * N);
        }
        if (e != hipSuccess) { lcr_destroy(s); return fail(LCR_ERR_HIP, "setting up the frame stream failed: %s", hipGetErrorString(e)); }
    }
    *out = s;
    return LCR_OK;
}

// (also what lcr_create unwinds a half-built handle through: whatever was never created is null and skipped)
void lcr_destroy(lcr_sim *s) {
    if (!s) return;
    (void)hipSetDevice(s->cfg.device);
    (void)hipStreamSynchronize(s->stream);
    if (s->rstream) {
        (void)hipStreamSynchronize(s->rstream);
        for (int p = 0; p < 2; p++) {
            if (s->ev_snap[p]) (void)hipEventDestroy(s->ev_snap[p]);
            if (s->ev_rdone[p]) (void)hipEventDestroy(s->ev_rdone[p]);
            (void)hipFree(s->snap_qpos[p]); (void)hipFree(s->snap_target[p]);
        }
        (void)hipStreamDestroy(s->rstream);
    }
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->render_dev) (void)hipFree(s->render_dev);
    if (s->term_stage) (void)hipFree(s->term_stage);
    if (s->planes_mem) (void)hipFree(s->planes_mem);
    if (s->look_mem) (void)hipFree(s->look_mem);
    if (s->wrist_mem) (void)hipFree(s->wrist_mem);
    if (s->stack_mem) (void)hipFree(s->stack_mem);
    if (s->cloud_mem) (void)hipFree(s->cloud_mem);
    if (s->voxel_mem) (void)hipFree(s->voxel_mem);
    if (s->height_mem) (void)hipFree(s->height_mem);
    if (s->boxes_mem) (void)hipFree(s->boxes_mem);
    if (s->normals_mem) (void)hipFree(s->normals_mem);
    if (s->flow_mem) (void)hipFree(s->flow_mem);
    free(s->look_variants);
    if (s->host_mirror) (void)hipHostFree(s->host_mirror);
    (void)hipFree(s->arena);
    delete s;
}

#define SIMCHK_NOJOIN(s)                                      \
    if (!(s)) return fail(LCR_ERR_INVALID, "sim is NULL"); \
    HIPCHK(hipSetDevice((s)->cfg.device))
#define SIMCHK(s)       \
    SIMCHK_NOJOIN(s);   \
    if (int jr_ = join_render(s)) return fail(LCR_ERR_HIP, "waiting for the frame kernel failed: %s", hipGetErrorString((hipError_t)jr_))

int lcr_step_kernel_family(lcr_sim *s) {
    if (!s) return fail(LCR_ERR_INVALID, "sim is NULL");
    return s->dev.coop;
}

int lcr_get_redo_flags(lcr_sim *s, int32_t *flags_host, int32_t capacity, int32_t *n_waves, int32_t *paired) {
    SIMCHK(s);
    const int waves = (s->dev.n + 63) / 64;
    if (n_waves) *n_waves = s->redo_words ? waves : 0;
    if (paired) *paired = s->redo.gate;
    if (!flags_host || !s->redo_words) return LCR_OK;
    if (capacity < waves) return fail(LCR_ERR_INVALID, "flags_host holds %d words, the handle has %d waves", capacity, waves);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(flags_host, s->redo.flags, sizeof(int32_t) * (size_t)waves, hipMemcpyDeviceToHost));
    return LCR_OK;
}

int lcr_set_stream(lcr_sim *s, void *hip_stream) {
    SIMCHK(s);
    // nothing enqueued on the old stream -- a step kernel, a reset, lcr_fill_random_actions into a buffer the next step reads -- is in flight when the new stream takes over:
    // the two streams are not ordered against each other otherwise.  (A host wait: the call is rare and never in a loop.)
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->rstream) HIPCHK(hipStreamSynchronize(s->rstream));   // (nor anything of the old stream's frames)
    s->stream = (hipStream_t)hip_stream;
    return LCR_OK;
}

int lcr_sync(lcr_sim *s) {
    SIMCHK(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    return LCR_OK;
}

int lcr_reset(lcr_sim *s, const uint8_t *mask_host, const uint64_t *seeds_host) {
    SIMCHK(s);
    const size_t N = (size_t)s->dev.n;
    if (mask_host) HIPCHK(hipMemcpyAsync(s->mask_dev, mask_host, N, hipMemcpyHostToDevice, s->stream));
    if (seeds_host) HIPCHK(hipMemcpyAsync(s->seeds_dev, seeds_host, N * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
    LAUNCHCHK("reset kernel", lcr_launch_reset(s->dev, mask_host ? s->mask_dev : nullptr, seeds_host ? s->seeds_dev : nullptr, 0, 0, s->stream));
    if (s->look_K)   // the reset envs count an episode and -- with a sampler -- draw its look
        LAUNCHCHK("look kernel", lcr_launch_look_redraw(s->dev.n, s->dev.env_off, mask_host ? s->mask_dev : nullptr, 0, s->look_sm, s->look_cur, s->look_episode, nullptr, s->stream));
    if (s->has_images)   // the stack: masked envs (no mask: all) are refilled, the others have their newest slot rewritten
        if (int rc = frames_after(s, s->dev, s->stream, nullptr, mask_host ? s->mask_dev : nullptr, mask_host ? LCR_STACK_NEWEST : LCR_STACK_REFILL)) return rc;
    // the staging copies above read caller memory: do not return before they are consumed
    if (mask_host || seeds_host) HIPCHK(hipStreamSynchronize(s->stream));
    return LCR_OK;
}

int lcr_step(lcr_sim *s, const float *action_dev) {
    SIMCHK_NOJOIN(s);
    if (!action_dev) return fail(LCR_ERR_INVALID, "action is NULL");
    LAUNCHCHK("step kernel", lcr_launch_step(s->dev, action_dev, s->ee_mode, s->stream, s->redo));
    if (s->look_K)   // envs the step has auto-reset: their look becomes the terminal look, they count an episode and draw its look -- before the snapshot below
        LAUNCHCHK("look kernel", lcr_launch_look_redraw(s->dev.n, s->dev.env_off, s->dev.did_reset, 0, s->look_sm, s->look_cur, s->look_episode, s->look_term, s->stream));
    if (s->has_images && s->rstream) {
        // the frame kernel reads qpos and target only: snapshot them (2.7 MB for 32 768 StackTwoCubes envs against 15 GB of frames), then ray-cast on the second stream while
        // this stream goes on with the next step.  Two snapshots in turn; the one about to be overwritten was read by the frames of two steps ago.
        const int p = s->rpar;
        const size_t N = (size_t)s->dev.n;
        if (s->snap_used[p]) HIPCHK(hipStreamWaitEvent(s->stream, s->ev_rdone[p], 0));
        HIPCHK(hipMemcpyAsync(s->snap_qpos[p], s->dev.qpos, sizeof(float) * (size_t)s->nq * N, hipMemcpyDeviceToDevice, s->stream));
        HIPCHK(hipMemcpyAsync(s->snap_target[p], s->dev.target, sizeof(float) * 3 * N, hipMemcpyDeviceToDevice, s->stream));
        // (and the looks, 40 B per env: the redraw of the next step must not reach the frames of this one)
        if (s->look_K) HIPCHK(hipMemcpyAsync(s->snap_look[p], s->look_cur, sizeof(int) * 10 * N, hipMemcpyDeviceToDevice, s->stream));
        // (and did_reset, 1 B per env, for the stack: the step kernel of the next step overwrites the flags while the stack of this one may still have to read them)
        // (the motion vectors read the same flags: on a handle without a stack the snapshot goes into their own allocation)
        const unsigned char *flags = s->snap_reset[p];
        if (s->stack_on) HIPCHK(hipMemcpyAsync(s->snap_reset[p], s->dev.did_reset, N, hipMemcpyDeviceToDevice, s->stream));
        else if (s->flow_on) { HIPCHK(hipMemcpyAsync(s->flow_reset[p], s->dev.did_reset, N, hipMemcpyDeviceToDevice, s->stream)); flags = s->flow_reset[p]; }
        HIPCHK(hipEventRecord(s->ev_snap[p], s->stream));
        HIPCHK(hipStreamWaitEvent(s->rstream, s->ev_snap[p], 0));
        LcrDev R = s->dev;
        R.qpos = s->snap_qpos[p]; R.target = s->snap_target[p];
        // (the stack before ev_rdone: join_render then covers it as it covers the frames)
        if (int rc = frames_after(s, R, s->rstream, s->look_K ? s->snap_look[p] : nullptr, flags, LCR_STACK_PUSH, true)) return rc;
        HIPCHK(hipEventRecord(s->ev_rdone[p], s->rstream));
        s->snap_used[p] = true; s->rpending = true; s->rlast = p; s->rpar = p ^ 1;
    } else if (s->has_images) {   // same stream as the step kernel: did_reset itself is current until the next step
        if (int rc = frames_after(s, s->dev, s->stream, nullptr, s->dev.did_reset, LCR_STACK_PUSH, true)) return rc;
    }
    return LCR_OK;
}

int lcr_step_host(lcr_sim *s, const float *action_host) {
    SIMCHK(s);
    if (!action_host) return fail(LCR_ERR_INVALID, "action is NULL");
    HIPCHK(hipMemcpyAsync(s->action_stage, action_host, sizeof(float) * (size_t)s->k * s->dev.n, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return lcr_step(s, s->action_stage);
}

int lcr_get_obs(lcr_sim *s, lcr_obs_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (image_front / image_top are drawn on the second stream after a step: the handle's stream waits for them here)
    const size_t N = (size_t)s->dev.n;
    out->n_envs = s->dev.n;
    out->arm_qpos = s->dev.qpos;
    out->arm_qvel = s->dev.qvel;
    out->cube_pos = s->dev.qpos + 6 * N;
    if (s->dev.has_target) { out->has_aux = 1; out->aux_pos = s->dev.target; }
    else if (s->cfg.task == LCR_TASK_STACK) { out->has_aux = 1; out->aux_pos = s->dev.qpos + 13 * N; }
    else { out->has_aux = 0; out->aux_pos = nullptr; }
    out->image_front = s->dev.img_front;
    out->image_top = s->dev.img_top;
    out->image_width = s->has_images ? s->dev.img_w : 0;
    out->image_height = s->has_images ? s->dev.img_h : 0;
    return LCR_OK;
}

int lcr_get_outputs(lcr_sim *s, lcr_out_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    out->n_envs = s->dev.n;
    out->_pad = 0;
    out->reward = s->dev.reward;
    out->terminated = s->dev.terminated;
    out->truncated = s->dev.truncated;
    out->is_success = s->dev.is_success;
    out->did_reset = s->dev.did_reset;
    out->terminal_obs = s->dev.term_obs;
    out->terminal_quat = s->dev.term_quat;
    out->timestamp = s->dev.sim_time;
    out->current_goal = s->dev.goal;
    out->active_mask = s->dev.active_mask;
    out->active_count = s->dev.active_count;
    out->max_sweeps = s->dev.max_sweeps;
    out->choice = s->dev.choice;
    out->ctrl = s->dev.ctrl_out;
    return LCR_OK;
}

int lcr_fetch_host(lcr_sim *s, lcr_host_view *out) {
    SIMCHK(s);
    if (!out) return fail(LCR_ERR_INVALID, "out is NULL");
    const size_t N = (size_t)s->dev.n;
    if (!s->host_mirror) {
        hipError_t e = hipHostMalloc((void **)&s->host_mirror, s->tobs_off + s->tobs_bytes, hipHostMallocDefault);
        if (e != hipSuccess) { s->host_mirror = nullptr; return fail(LCR_ERR_OOM, "hipHostMalloc(%zu) failed: %s", s->tobs_off + s->tobs_bytes, hipGetErrorString(e)); }
    }
    HIPCHK(hipMemcpyAsync(s->host_mirror, s->arena, s->fetch_bytes, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    const char *hb = s->host_mirror, *db = (const char *)s->arena;
    auto H = [&](const void *dev) { return hb + ((const char *)dev - db); };
    const unsigned char *dres = (const unsigned char *)H(s->dev.did_reset);
    int any = 0;
    for (size_t i = 0; i < N; i++) any |= dres[i];
    if (any) {
        HIPCHK(hipMemcpyAsync(s->host_mirror + s->tobs_off, (const char *)s->arena + s->tobs_off, s->tobs_bytes, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    out->n_envs = s->dev.n;
    out->any_reset = any;
    out->arm_qpos = (const float *)H(s->dev.qpos);
    out->arm_qvel = (const float *)H(s->dev.qvel);
    out->cube_pos = (const float *)H(s->dev.qpos + 6 * N);
    out->aux_pos = s->dev.has_target ? (const float *)H(s->dev.target) : (s->cfg.task == LCR_TASK_STACK ? (const float *)H(s->dev.qpos + 13 * N) : nullptr);
    out->reward = (const float *)H(s->dev.reward);
    out->terminated = (const unsigned char *)H(s->dev.terminated);
    out->truncated = (const unsigned char *)H(s->dev.truncated);
    out->is_success = (const unsigned char *)H(s->dev.is_success);
    out->did_reset = dres;
    out->terminal_obs = (const float *)H(s->dev.term_obs);
    return LCR_OK;
}

int lcr_get_state(lcr_sim *s, double *qpos, double *qvel, double *ee_lag, float *target, int32_t *elapsed, uint64_t *rng,
                  int32_t *current_goal, double *sim_time, float *warm) {
    SIMCHK(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t N = (size_t)s->dev.n;
    std::vector<float> tmp;
    auto pull = [&](double *dst, const float *src, size_t cnt) -> hipError_t {
        tmp.resize(cnt);
        hipError_t e = hipMemcpy(tmp.data(), src, cnt * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess) for (size_t i = 0; i < cnt; i++) dst[i] = (double)tmp[i];
        return e;
    };
    if (qpos) HIPCHK(pull(qpos, s->dev.qpos, s->nq * N));
    if (qvel) HIPCHK(pull(qvel, s->dev.qvel, s->nv * N));
    if (ee_lag) HIPCHK(pull(ee_lag, s->dev.ee_lag, 3 * N));
    if (target) HIPCHK(hipMemcpy(target, s->dev.target, 3 * N * sizeof(float), hipMemcpyDeviceToHost));
    if (elapsed) HIPCHK(hipMemcpy(elapsed, s->dev.elapsed, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (rng) HIPCHK(hipMemcpy(rng, s->dev.rng, 4 * N * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (current_goal) HIPCHK(hipMemcpy(current_goal, s->dev.goal, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sim_time) HIPCHK(hipMemcpy(sim_time, s->dev.sim_time, N * sizeof(double), hipMemcpyDeviceToHost));
    if (warm) {   // the carried constraint forces (mjData.qacc_warmstart of the reference's sim); zeros when nothing is carried
        if (s->dev.warm) HIPCHK(hipMemcpy(warm, s->dev.warm, sizeof(float) * LCR_NWARM * N, hipMemcpyDeviceToHost));
        else memset(warm, 0, sizeof(float) * LCR_NWARM * N);
    }
    return LCR_OK;
}

int lcr_set_state(lcr_sim *s, const double *qpos, const double *qvel, const double *ee_lag, const float *target,
                  const int32_t *elapsed, const uint64_t *rng, const int32_t *current_goal, const double *sim_time, const float *warm) {
    SIMCHK(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t N = (size_t)s->dev.n;
    std::vector<float> tmp;
    auto push = [&](float *dst, const double *src, size_t cnt) -> hipError_t {
        tmp.resize(cnt);
        for (size_t i = 0; i < cnt; i++) tmp[i] = (float)src[i];
        return hipMemcpy(dst, tmp.data(), cnt * sizeof(float), hipMemcpyHostToDevice);
    };
    if (qpos) HIPCHK(push(s->dev.qpos, qpos, s->nq * N));
    // a state set from outside without its constraint forces starts cold (zero forces in the first substep of the next step);
    // with them (warm != NULL: a checkpoint taken by lcr_get_state) the next step continues exactly where the saved sim would have
    if (s->dev.warm) {
        if (warm) HIPCHK(hipMemcpy(s->dev.warm, warm, sizeof(float) * LCR_NWARM * N, hipMemcpyHostToDevice));
        else if (qpos || qvel) HIPCHK(hipMemset(s->dev.warm, 0, sizeof(float) * LCR_NWARM * N));
    }
    if (qvel) HIPCHK(push(s->dev.qvel, qvel, s->nv * N));
    if (ee_lag) HIPCHK(push(s->dev.ee_lag, ee_lag, 3 * N));
    if (target) HIPCHK(hipMemcpy(s->dev.target, target, 3 * N * sizeof(float), hipMemcpyHostToDevice));
    if (elapsed) HIPCHK(hipMemcpy(s->dev.elapsed, elapsed, N * sizeof(int32_t), hipMemcpyHostToDevice));
    if (rng) HIPCHK(hipMemcpy(s->dev.rng, rng, 4 * N * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (current_goal) HIPCHK(hipMemcpy(s->dev.goal, current_goal, N * sizeof(int32_t), hipMemcpyHostToDevice));
    if (sim_time) HIPCHK(hipMemcpy(s->dev.sim_time, sim_time, N * sizeof(double), hipMemcpyHostToDevice));
    // the state has jumped: the motion vectors restart from it (this call draws no frames; the planes are zero and valid is 0 until the next step)
    if (s->flow_on) LAUNCHCHK("motion-vector kernel", launch_flow(s, s->dev, s->stream, nullptr, nullptr, false));
    return LCR_OK;
}

int lcr_malloc(lcr_sim *s, size_t bytes, void **dev_out) {
    SIMCHK(s);
    if (!dev_out) return fail(LCR_ERR_INVALID, "dev_out is NULL");
    hipError_t e = hipMalloc(dev_out, bytes);
    if (e != hipSuccess) return fail(LCR_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return LCR_OK;
}
int lcr_free(lcr_sim *s, void *dev) {
    SIMCHK(s);
    HIPCHK(hipFree(dev));
    return LCR_OK;
}
int lcr_memcpy_h2d(lcr_sim *s, void *dst_dev, const void *src_host, size_t bytes) {
    SIMCHK(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return LCR_OK;
}
int lcr_memcpy_d2h(lcr_sim *s, void *dst_host, const void *src_dev, size_t bytes) {
    SIMCHK(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return LCR_OK;
}

int lcr_timer_begin(lcr_sim *s) {
    SIMCHK(s);
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    return LCR_OK;
}
int lcr_timer_end(lcr_sim *s, float *ms_out) {
    SIMCHK(s);
    if (!ms_out) return fail(LCR_ERR_INVALID, "ms_out is NULL");
    HIPCHK(hipEventRecord(s->ev1, s->stream));
    HIPCHK(hipEventSynchronize(s->ev1));
    HIPCHK(hipEventElapsedTime(ms_out, s->ev0, s->ev1));
    return LCR_OK;
}

int lcr_fill_random_actions(lcr_sim *s, float *action_dev, uint64_t seed, uint64_t step) {
    SIMCHK_NOJOIN(s);   // (writes the caller's action buffer only)
    if (!action_dev) return fail(LCR_ERR_INVALID, "action is NULL");
    LAUNCHCHK("fill kernel", lcr_launch_fill_actions(action_dev, s->dev.n, s->k, s->dev.env_off, seed, step, s->stream));
    return LCR_OK;
}

// the variant env `env` points at (a synchronous 4-byte read)
static int look_variant_of(lcr_sim *s, int env, int *v) {
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(v, s->look_cur + env, sizeof(int), hipMemcpyDeviceToHost));
    if (*v < 0 || *v >= s->look_K) return fail(LCR_ERR_HIP, "env %d points at variant %d of %d", env, *v, s->look_K);
    return LCR_OK;
}

// ---- the four single-frame calls (lcr_render, lcr_render_state, lcr_render_planes, lcr_render_state_planes) ----
// Each checks its own arguments, then FRAMECHK; lays the scratch frame out (a Carver over render_dev: the frame or the two planes, for a caller's pose stage_pose behind
// them); and ends in one of two tails, render_colour_of or render_planes_of, which resolve the camera (single_cam), launch and copy out.

// the camera and the frame size a single-frame call accepts
#define FRAMECHK(s, camera, width, height)                                                                                                       \
    do {                                                                                                                                         \
        CAMCHK(s, camera);                                                                                                                       \
        if ((width) <= 0 || (height) <= 0 || (size_t)(width) * (height) > ((size_t)1 << 26)) return fail(LCR_ERR_INVALID, "bad frame size"); \
    } while (0)

// scene camera `camera` with the ray scale of a frame `height` rows high.  `look_env` >= 0 on a handle with a look: that env's own view, i.e. through its variant's camera
// when `camera` is an observation camera (camera_vizu stays where it is)
static int single_cam(lcr_sim *s, int camera, int height, int look_env, LcrCam &cam) {
    cam = camera == 0 ? s->cam_front : (camera == 1 ? s->cam_top : s->cam_vizu);
    cam.s = (float)(2.0 * std::tan(0.5 * 45.0 * M_PI / 180.0) / height);
    if (look_env >= 0 && s->look_K && camera < 2) {
        int v = 0;
        if (int lr = look_variant_of(s, look_env, &v)) return lr;
        make_look_camera(s->look_variants[v], camera, height, cam);
    }
    return LCR_OK;
}

// grows the scratch frame to what `C` has laid out plus a pose and stages the caller's pose there.  P1: a one-env view of the handle whose state arrays are that pose
static int stage_pose(lcr_sim *s, Carver &C, const double *qpos_host, const float *target_host, LcrDev &P1) {
    float st[32];
    const size_t o_pose = C.take(sizeof st);
    if (int rc = reserve((void **)&s->render_dev, &s->render_bytes, C.off)) return rc;
    for (int i = 0; i < s->nq; i++) st[i] = (float)qpos_host[i];
    for (int i = 0; i < 3; i++) st[s->nq + i] = target_host ? target_host[i] : 0.f;
    float *stage = (float *)(s->render_dev + o_pose);
    HIPCHK(hipMemcpyAsync(stage, st, sizeof(float) * (s->nq + 3), hipMemcpyHostToDevice, s->stream));
    P1 = s->dev;
    P1.n = 1;
    P1.qpos = stage;
    P1.target = stage + s->nq;
    return LCR_OK;
}

// one colour frame of the pose arrays of `P` (env `env`), drawn at the start of the scratch frame and copied to the host (`look_env` >= 0: with that env's look)
static int render_colour_of(lcr_sim *s, const LcrDev &P, int env, int camera, int width, int height, uint8_t *rgb_host, int look_env = -1) {
    const bool look = look_env >= 0 && s->look_K;
    if (camera == 3)   // the wrist camera of the pose
        LAUNCHCHK("render", lcr_launch_render_single_wrist(P, wrist_mount_at(s, height), env, width, height, 0.f, s->render_dev, nullptr, nullptr, look ? &s->look : nullptr, look_env, P.n, s->stream));
    else {
        LcrCam cam;
        if (int rc = single_cam(s, camera, height, look_env, cam)) return rc;
        // (a look: the variant's colours and light, the env's colours)
        if (look) LAUNCHCHK("render", lcr_launch_render_single_look(P, cam, env, width, height, s->render_dev, s->look, look_env, P.n, s->stream));
        else LAUNCHCHK("render", lcr_launch_render_single(P, cam, env, width, height, s->render_dev, s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(rgb_host, s->render_dev, (size_t)width * height * 3, hipMemcpyDeviceToHost));
    return LCR_OK;
}

int lcr_render(lcr_sim *s, int env, int camera, int width, int height, uint8_t *rgb_host) {
    SIMCHK(s);
    if (!rgb_host) return fail(LCR_ERR_INVALID, "rgb_host is NULL");
    if (env < 0 || env >= s->dev.n) return fail(LCR_ERR_INVALID, "env %d out of range", env);
    FRAMECHK(s, camera, width, height);
    if (int rc = reserve((void **)&s->render_dev, &s->render_bytes, (size_t)width * height * 3)) return rc;   // (the frame alone: nothing is staged behind it)
    return render_colour_of(s, s->dev, env, camera, width, height, rgb_host, env);
}

int lcr_render_state(lcr_sim *s, int camera, int width, int height, const double *qpos_host, const float *target_host, uint8_t *rgb_host) {
    SIMCHK(s);
    if (!rgb_host || !qpos_host) return fail(LCR_ERR_INVALID, "NULL argument");
    FRAMECHK(s, camera, width, height);
    Carver C;
    C.take((size_t)width * height * 3);
    LcrDev P1;
    if (int rc = stage_pose(s, C, qpos_host, target_host, P1)) return rc;
    return render_colour_of(s, P1, 0, camera, width, height, rgb_host);
}

int lcr_render_terminal(lcr_sim *s, const int32_t *env_ids_host, int count, uint8_t *front_host, uint8_t *top_host) {
    SIMCHK(s);
    if (count < 0 || (count > 0 && (!env_ids_host || !front_host || !top_host))) return fail(LCR_ERR_INVALID, "NULL argument");
    if (!s->has_images) return fail(LCR_ERR_UNSUPPORTED, "terminal frames need observation_mode image / both (the frame background is only kept then)");
    const size_t img = (size_t)s->dev.img_h * s->dev.img_w * 3;
    const size_t per_env[] = {img, img};   // front, top
    return render_terminal_passes(s, env_ids_host, count, per_env, [&](LcrDev &P1, const LcrLook &LK, int c, size_t done, char *const *buf) -> int {
        P1.img_front = (unsigned char *)buf[0];
        P1.img_top = (unsigned char *)buf[1];
        if (s->look_K) LAUNCHCHK("render", lcr_launch_render_obs_look(P1, LK, nullptr, s->stream));
        else LAUNCHCHK("render", lcr_launch_render_obs(P1, s->cam_front, s->cam_top, s->stream));
        HIPCHK(hipMemcpyAsync(front_host + done * img, buf[0], img * c, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipMemcpyAsync(top_host + done * img, buf[1], img * c, hipMemcpyDeviceToHost, s->stream));
        return LCR_OK;
    });
}

// ---- depth / segmentation planes of the image observations ----

int lcr_enable_image_planes(lcr_sim *s, uint32_t planes, float depth_far) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (planes == 0 || (planes & ~(uint32_t)(LCR_PLANE_DEPTH | LCR_PLANE_SEGMENTATION)))
        return fail(LCR_ERR_INVALID, "planes must be LCR_PLANE_DEPTH (1), LCR_PLANE_SEGMENTATION (2) or both (3), got %u", planes);
    uint32_t bits;
    memcpy(&bits, &depth_far, sizeof bits);   // (this file is compiled with -ffast-math: NaN and infinity are told by their exponent bits)
    if ((bits & 0x7f800000u) == 0x7f800000u) return fail(LCR_ERR_INVALID, "depth_far must be finite, in (0, 1000] metres");
    if (depth_far <= 0.f || depth_far > 1000.f) return fail(LCR_ERR_INVALID, "depth_far must lie in (0, 1000] metres, got %g", (double)depth_far);
    SIMCHK(s);
    if (!s->has_images) return fail(LCR_ERR_INVALID, "sim has no image observations (observation_mode state): there are no frames to add planes to");
    if (s->planes) {
        if (s->planes == planes && s->pl.far == depth_far) return LCR_OK;
        return fail(LCR_ERR_INVALID, "planes %u with depth_far %g are enabled already and fixed for the life of the handle (asked for planes %u, depth_far %g)", s->planes,
                    (double)s->pl.far, planes, (double)depth_far);
    }
    const size_t N = (size_t)s->dev.n, px = (size_t)s->dev.img_h * s->dev.img_w;
    const bool dep = planes & LCR_PLANE_DEPTH, seg = planes & LCR_PLANE_SEGMENTATION;
    const size_t nbg = s->look_K ? (size_t)s->look_K : 1;   // with a look: the background planes of every variant's cameras, [K][2][H][W]
    const size_t dbytes = dep ? N * px * sizeof(float) : 0, sbytes = seg ? N * px : 0;   // one camera's planes (0: not enabled, no room taken)
    Carver C;
    const size_t o_bgd = C.take(nbg * 2 * px * sizeof(float));
    const size_t o_bgs = C.take(nbg * 2 * px);
    const size_t o_d0 = C.take(dbytes);
    const size_t o_d1 = C.take(dbytes);
    const size_t o_s0 = C.take(sbytes);
    const size_t o_s1 = C.take(sbytes);
    // the planes cover the wrist camera; LCR_WRIST_GUARD bytes of LCR_WRIST_GUARD_BYTE before, between and behind them (include/lcr.h)
    const size_t o_g2 = C.skip(s->wrist_on ? LCR_WRIST_GUARD : 0);
    const size_t o_d2 = C.take(s->wrist_on ? dbytes : 0);
    if (dep && s->wrist_on) C.skip(LCR_WRIST_GUARD);
    const size_t o_s2 = C.take(s->wrist_on ? sbytes : 0);
    if (seg && s->wrist_on) C.skip(LCR_WRIST_GUARD);
    const size_t off = C.off;
    void *mem = nullptr;
    hipError_t e = hipMalloc(&mem, off);
    if (e != hipSuccess) return fail(LCR_ERR_OOM, "hipMalloc(%zu bytes) for the image planes failed: %s", off, hipGetErrorString(e));
    char *base = (char *)mem;
    LcrPlanes PL{};
    PL.bg_depth = (float *)(base + o_bgd);
    PL.bg_seg = (unsigned char *)(base + o_bgs);
    PL.depth_front = dep ? (float *)(base + o_d0) : nullptr;
    PL.depth_top = dep ? (float *)(base + o_d1) : nullptr;
    PL.seg_front = seg ? (unsigned char *)(base + o_s0) : nullptr;
    PL.seg_top = seg ? (unsigned char *)(base + o_s1) : nullptr;
    PL.far = depth_far;
    // the background planes, then colours and planes of the current state
    int rc;
    if (s->look_K) {
        rc = lcr_launch_render_bg_planes_look(s->dev, s->look, s->look_K, PL, s->stream);
        if (!rc) rc = lcr_launch_render_obs_look(s->dev, s->look, &PL, s->stream);
    } else {
        rc = lcr_launch_render_bg_planes(s->dev, s->cam_front, s->cam_top, PL, s->stream);
        if (!rc) rc = lcr_launch_render_obs_planes(s->dev, s->cam_front, s->cam_top, PL, s->stream);
    }
    LcrWrist WR = s->wrist;
    if (s->wrist_on) {
        if (!rc) rc = (int)hipMemsetAsync(base + o_g2, LCR_WRIST_GUARD_BYTE, off - o_g2, s->stream);
        WR.depth = dep ? (float *)(base + o_d2) : nullptr;
        WR.seg = seg ? (unsigned char *)(base + o_s2) : nullptr;
        WR.far = depth_far;
        if (!rc) rc = lcr_launch_render_wrist(s->dev, WR, s->look_K ? &s->look : nullptr, s->stream);
    }
    if (!rc) rc = (int)hipStreamSynchronize(s->stream);
    if (rc) { (void)hipFree(mem); return fail(LCR_ERR_HIP, "drawing the image planes failed: %s", hipGetErrorString((hipError_t)rc)); }
    s->wrist = WR;
    s->pl = PL;
    s->planes_mem = mem;
    s->planes = planes;
    return LCR_OK;
}

int lcr_get_image_planes(lcr_sim *s, lcr_planes_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the planes are drawn with the frames, on the second stream after a step: the handle's stream waits for them here)
    memset(out, 0, sizeof *out);
    if (!s->planes) return LCR_OK;
    out->planes = s->planes;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    out->depth_far = s->pl.far;
    out->depth_front = s->pl.depth_front;
    out->depth_top = s->pl.depth_top;
    out->seg_front = s->pl.seg_front;
    out->seg_top = s->pl.seg_top;
    return LCR_OK;
}

// one frame's planes of the pose arrays of `P` (env `env`), drawn into the scratch frame -- depth at its start, segmentation at `o_seg` -- and copied to the host
// (`look_env` >= 0: with that env's look, i.e. through its variant's camera when `camera` is an observation camera -- colours and light do not show in the planes)
static int render_planes_of(lcr_sim *s, const LcrDev &P, int env, int camera, int width, int height, size_t o_seg, float *depth_host, uint8_t *seg_host, int look_env = -1) {
    LcrCam cam;
    if (int rc = single_cam(s, camera, height, look_env, cam)) return rc;
    const size_t px = (size_t)width * height;
    const float far = s->planes ? s->pl.far : 10.f;
    float *depth_dev = depth_host ? (float *)s->render_dev : nullptr;
    unsigned char *seg_dev = seg_host ? s->render_dev + o_seg : nullptr;
    if (camera == 3) LAUNCHCHK("render", lcr_launch_render_single_wrist(P, wrist_mount_at(s, height), env, width, height, far, nullptr, depth_dev, seg_dev, nullptr, -1, 1, s->stream));
    else LAUNCHCHK("render", lcr_launch_render_single_planes(P, cam, env, width, height, far, depth_dev, seg_dev, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (depth_host) HIPCHK(hipMemcpy(depth_host, s->render_dev, px * sizeof(float), hipMemcpyDeviceToHost));
    if (seg_host) HIPCHK(hipMemcpy(seg_host, s->render_dev + o_seg, px, hipMemcpyDeviceToHost));
    return LCR_OK;
}

int lcr_render_planes(lcr_sim *s, int env, int camera, int width, int height, float *depth_host, uint8_t *seg_host) {
    SIMCHK(s);
    if (!depth_host && !seg_host) return fail(LCR_ERR_INVALID, "depth_host and seg_host are both NULL");
    if (env < 0 || env >= s->dev.n) return fail(LCR_ERR_INVALID, "env %d out of range", env);
    FRAMECHK(s, camera, width, height);
    Carver C;
    C.take((size_t)width * height * sizeof(float));
    const size_t o_seg = C.off;
    if (int rc = reserve((void **)&s->render_dev, &s->render_bytes, o_seg + (size_t)width * height)) return rc;   // (the last slice as long as it is: nothing is staged behind it)
    return render_planes_of(s, s->dev, env, camera, width, height, o_seg, depth_host, seg_host, env);
}

int lcr_render_state_planes(lcr_sim *s, int camera, int width, int height, const double *qpos_host, const float *target_host, float *depth_host, uint8_t *seg_host) {
    SIMCHK(s);
    if (!qpos_host || (!depth_host && !seg_host)) return fail(LCR_ERR_INVALID, "NULL argument");
    FRAMECHK(s, camera, width, height);
    Carver C;
    C.take((size_t)width * height * sizeof(float));
    const size_t o_seg = C.take((size_t)width * height);
    LcrDev P1;
    if (int rc = stage_pose(s, C, qpos_host, target_host, P1)) return rc;
    return render_planes_of(s, P1, 0, camera, width, height, o_seg, depth_host, seg_host);
}

int lcr_render_terminal_planes(lcr_sim *s, const int32_t *env_ids_host, int count, float *depth_front, float *depth_top, uint8_t *seg_front, uint8_t *seg_top) {
    SIMCHK(s);
    if (!s->planes) return fail(LCR_ERR_INVALID, "no image planes are enabled on this sim (lcr_enable_image_planes)");
    const bool dep = s->planes & LCR_PLANE_DEPTH, seg = s->planes & LCR_PLANE_SEGMENTATION;
    if (count < 0 || (count > 0 && (!env_ids_host || (dep && (!depth_front || !depth_top)) || (seg && (!seg_front || !seg_top)))))
        return fail(LCR_ERR_INVALID, "NULL argument (only the pointers of a plane that is not enabled may be NULL)");
    // the frame kernel draws the colours in the same launch: they are staged too and dropped
    const size_t px = (size_t)s->dev.img_h * s->dev.img_w, img = px * 3, dpx = dep ? px * sizeof(float) : 0, spx = seg ? px : 0;
    const size_t per_env[] = {img, img, dpx, dpx, spx, spx};   // front, top of the colours, the depths, the segmentations
    return render_terminal_passes(s, env_ids_host, count, per_env, [&](LcrDev &P1, const LcrLook &LK, int c, size_t done, char *const *buf) -> int {
        P1.img_front = (unsigned char *)buf[0];
        P1.img_top = (unsigned char *)buf[1];
        LcrPlanes PL1 = s->pl;
        PL1.depth_front = (float *)buf[2];
        PL1.depth_top = (float *)buf[3];
        PL1.seg_front = (unsigned char *)buf[4];
        PL1.seg_top = (unsigned char *)buf[5];
        if (s->look_K) LAUNCHCHK("render", lcr_launch_render_obs_look(P1, LK, &PL1, s->stream));
        else LAUNCHCHK("render", lcr_launch_render_obs_planes(P1, s->cam_front, s->cam_top, PL1, s->stream));
        if (dep) {
            HIPCHK(hipMemcpyAsync(depth_front + done * px, buf[2], dpx * c, hipMemcpyDeviceToHost, s->stream));
            HIPCHK(hipMemcpyAsync(depth_top + done * px, buf[3], dpx * c, hipMemcpyDeviceToHost, s->stream));
        }
        if (seg) {
            HIPCHK(hipMemcpyAsync(seg_front + done * px, buf[4], spx * c, hipMemcpyDeviceToHost, s->stream));
            HIPCHK(hipMemcpyAsync(seg_top + done * px, buf[5], spx * c, hipMemcpyDeviceToHost, s->stream));
        }
        return LCR_OK;
    });
}

// ---- the look of the image observations ----

// (this file is compiled with -ffast-math: NaN and infinity are told by their exponent bits, read back through a volatile word so that the test is not folded away)
static bool finite_f(float x) { uint32_t b; memcpy(&b, &x, sizeof b); volatile uint32_t vb = b; return (vb & 0x7f800000u) != 0x7f800000u; }
static bool in_range(const float *v, int n, float lo, float hi) {
    for (int i = 0; i < n; i++)
        if (!finite_f(v[i]) || v[i] < lo || v[i] > hi) return false;
    return true;
}

int lcr_look_variant_default(lcr_look_variant *v) {
    if (!v) return fail(LCR_ERR_INVALID, "v is NULL");
    memset(v, 0, sizeof *v);
    v->fovy_deg[0] = v->fovy_deg[1] = 45.f;
    const float odd[3] = {0.2f, 0.3f, 0.4f}, even[3] = {0.1f, 0.2f, 0.3f}, sky[3] = {0.15f, 0.25f, 0.35f};
    for (int i = 0; i < 3; i++) {
        v->floor_rgb[0][i] = odd[i]; v->floor_rgb[1][i] = even[i];
        v->sky_rgb[i] = sky[i]; v->sky_slope[i] = sky[i];
        v->arm_rgb[i] = 0.8f; v->finger_rgb[i] = 0.75f;
    }
    v->ambient = 0.3f; v->diffuse = 0.6f;
    return LCR_OK;
}

// the task's colours (reach_cube.xml:26 / stack_two_cubes.xml:34 / push_cube.xml:35): cube, second cube, target marker
static const float LOOK_TASK_RGB[9] = {0.5f, 0.f, 0.f, 0.f, 0.f, 0.5f, 0.f, 0.f, 1.f};

int lcr_enable_look(lcr_sim *s, int n_variants, const lcr_look_variant *variants, const lcr_look_sampler *sampler) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (n_variants < 1 || n_variants > LCR_LOOK_MAX_VARIANTS) return fail(LCR_ERR_INVALID, "n_variants must lie in 1 .. %d, got %d", LCR_LOOK_MAX_VARIANTS, n_variants);
    if (!variants) return fail(LCR_ERR_INVALID, "variants_host is NULL");
    for (int k = 0; k < n_variants; k++) {
        const lcr_look_variant &v = variants[k];
        if (!in_range(&v.cam_dpos[0][0], 6, -0.2f, 0.2f)) return fail(LCR_ERR_INVALID, "variant %d: cam_dpos must be finite and within +-0.2 m per component", k);
        for (int c = 0; c < 2; c++) {
            const float *r = v.cam_drot[c];
            if (!in_range(r, 3, -0.5f, 0.5f) || std::sqrt((double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2]) > 0.5)
                return fail(LCR_ERR_INVALID, "variant %d: cam_drot must be finite and at most 0.5 rad long", k);
        }
        if (!in_range(v.fovy_deg, 2, 20.f, 90.f)) return fail(LCR_ERR_INVALID, "variant %d: fovy_deg must be finite and in [20, 90]", k);
        if (!in_range(&v.floor_rgb[0][0], 6, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "variant %d: floor_rgb must be finite and in [0, 1]", k);
        if (!in_range(v.sky_rgb, 3, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "variant %d: sky_rgb must be finite and in [0, 1]", k);
        if (!in_range(v.sky_slope, 3, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "variant %d: sky_slope must be finite and in [0, 1]", k);
        if (!in_range(&v.ambient, 1, 0.f, 1.5f)) return fail(LCR_ERR_INVALID, "variant %d: ambient must be finite and in [0, 1.5]", k);
        if (!in_range(&v.diffuse, 1, 0.f, 1.5f)) return fail(LCR_ERR_INVALID, "variant %d: diffuse must be finite and in [0, 1.5]", k);
        if (!in_range(v.arm_rgb, 3, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "variant %d: arm_rgb must be finite and in [0, 1]", k);
        if (!in_range(v.finger_rgb, 3, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "variant %d: finger_rgb must be finite and in [0, 1]", k);
    }
    if (sampler) {
        const float *lo[3] = {sampler->cube_lo, sampler->cube2_lo, sampler->marker_lo}, *hi[3] = {sampler->cube_hi, sampler->cube2_hi, sampler->marker_hi};
        const char *nm[3] = {"cube", "cube2", "marker"};
        for (int g = 0; g < 3; g++) {
            if (!in_range(lo[g], 3, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "sampler: %s_lo must be finite and in [0, 1]", nm[g]);
            if (!in_range(hi[g], 3, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "sampler: %s_hi must be finite and in [0, 1]", nm[g]);
            for (int i = 0; i < 3; i++)
                if (lo[g][i] > hi[g][i]) return fail(LCR_ERR_INVALID, "sampler: %s_lo must not exceed %s_hi (channel %d: %g > %g)", nm[g], nm[g], i, (double)lo[g][i], (double)hi[g][i]);
        }
    }
    SIMCHK(s);
    if (!s->has_images) return fail(LCR_ERR_INVALID, "sim has no image observations (observation_mode state): there are no frames to give a look");
    for (int k = 0; k < n_variants; k++)
        for (int c = 0; c < 2; c++) {
            double p[3], X[3], Y[3];
            scene_cam_pose(c, p, X, Y);
            if (p[2] + (double)variants[k].cam_dpos[c][2] < 0.05)
                return fail(LCR_ERR_INVALID, "variant %d: cam_dpos leaves camera %d %.3f m above the floor, less than 0.05 m", k, c, p[2] + (double)variants[k].cam_dpos[c][2]);
        }
    if (s->look_K) {
        const bool same = s->look_K == n_variants && memcmp(s->look_variants, variants, sizeof(lcr_look_variant) * n_variants) == 0 && s->look_has_sampler == (sampler != nullptr) &&
                          (!sampler || (sampler->seed == s->look_sampler.seed && memcmp(sampler->cube_lo, s->look_sampler.cube_lo, sizeof(float) * 18) == 0));
        if (same) return LCR_OK;
        return fail(LCR_ERR_INVALID, "a look of %d variants is enabled already and fixed for the life of the handle", s->look_K);
    }
    if (s->stack_on) return fail(LCR_ERR_INVALID, "the observation stack is enabled already: enable the look first and the stack last");
    if (s->planes) return fail(LCR_ERR_INVALID, "the image planes are enabled already: enable the look first and the planes second (their cached backgrounds are drawn per variant)");

    const size_t N = (size_t)s->dev.n, img = (size_t)s->dev.img_h * s->dev.img_w * 3, K = (size_t)n_variants;
    Carver C;
    const size_t o_var = C.take(sizeof(LcrLookVar) * K);
    const size_t o_bg = C.take(K * 2 * img);
    const size_t o_cur = C.take(sizeof(int) * 10 * N);
    const size_t o_term = C.take(sizeof(int) * 10 * N);
    const size_t o_ep = C.take(sizeof(unsigned) * N);
    size_t o_snap[2] = {C.off, C.off};
    if (s->rstream) for (int p = 0; p < 2; p++) o_snap[p] = C.take(sizeof(int) * 10 * N);
    const size_t off = C.off;
    lcr_look_variant *copy = (lcr_look_variant *)malloc(sizeof(lcr_look_variant) * K);
    if (!copy) return fail(LCR_ERR_OOM, "host allocation failed");
    memcpy(copy, variants, sizeof(lcr_look_variant) * K);
    void *mem = nullptr;
    hipError_t e = hipMalloc(&mem, off);
    if (e != hipSuccess) { free(copy); return fail(LCR_ERR_OOM, "hipMalloc(%zu bytes) for the look failed: %s", off, hipGetErrorString(e)); }
    char *base = (char *)mem;
    // the variant table as the kernels read it: cameras in fp64 as the scene cameras are built
    std::vector<LcrLookVar> tab(K);
    for (size_t k = 0; k < K; k++) {
        const lcr_look_variant &v = variants[k];
        LcrLookVar &t = tab[k];
        memset(&t, 0, sizeof t);
        for (int c = 0; c < 2; c++) make_look_camera(v, c, s->dev.img_h, t.cam[c]);
        t.ambient = v.ambient; t.diffuse = v.diffuse;
        memcpy(t.floor_rgb, v.floor_rgb, sizeof t.floor_rgb);
        memcpy(t.sky_rgb, v.sky_rgb, sizeof t.sky_rgb); memcpy(t.sky_slope, v.sky_slope, sizeof t.sky_slope);
        memcpy(t.arm_rgb, v.arm_rgb, sizeof t.arm_rgb); memcpy(t.finger_rgb, v.finger_rgb, sizeof t.finger_rgb);
    }
    // every env: variant 0 and its task's colours
    std::vector<int> init(10 * N, 0);
    for (int j = 0; j < 9; j++) {
        int bits;
        memcpy(&bits, &LOOK_TASK_RGB[j], sizeof bits);
        for (size_t i = 0; i < N; i++) init[(size_t)(1 + j) * N + i] = bits;
    }
    LcrLookSampler SM;
    memset(&SM, 0, sizeof SM);
    SM.K = n_variants;
    if (sampler) {
        SM.on = 1; SM.seed = sampler->seed;
        const float *lo[3] = {sampler->cube_lo, sampler->cube2_lo, sampler->marker_lo}, *hi[3] = {sampler->cube_hi, sampler->cube2_hi, sampler->marker_hi};
        for (int j = 0; j < 9; j++) { SM.lo[j] = lo[j / 3][j % 3]; SM.hi[j] = hi[j / 3][j % 3]; SM.rng[j] = SM.hi[j] - SM.lo[j]; }
    }
    LcrLook LK;
    LK.var = (const LcrLookVar *)(base + o_var);
    LK.bg = (const unsigned char *)(base + o_bg);
    LK.variant = (const int *)(base + o_cur);
    LK.rgb = (const float *)(base + o_cur) + N;
    int rc = (int)hipStreamSynchronize(s->stream);
    if (!rc) rc = (int)hipMemset(mem, 0, off);
    if (!rc) rc = (int)hipMemcpy(base + o_var, tab.data(), sizeof(LcrLookVar) * K, hipMemcpyHostToDevice);
    if (!rc) rc = (int)hipMemcpy(base + o_cur, init.data(), sizeof(int) * 10 * N, hipMemcpyHostToDevice);
    if (!rc) rc = (int)hipMemcpy(base + o_term, init.data(), sizeof(int) * 10 * N, hipMemcpyHostToDevice);
    if (!rc && sampler) rc = lcr_launch_look_redraw(s->dev.n, s->dev.env_off, nullptr, 1, SM, (int *)(base + o_cur), (unsigned *)(base + o_ep), nullptr, s->stream);
    if (!rc) rc = lcr_launch_render_bg_look(s->dev, LK, n_variants, s->stream);
    if (!rc) rc = lcr_launch_render_obs_look(s->dev, LK, nullptr, s->stream);
    if (!rc) rc = (int)hipStreamSynchronize(s->stream);
    if (rc) { (void)hipFree(mem); free(copy); return fail(LCR_ERR_HIP, "drawing the look failed: %s", hipGetErrorString((hipError_t)rc)); }
    s->look = LK;
    s->look_mem = mem;
    s->look_cur = (int *)(base + o_cur);
    s->look_term = (int *)(base + o_term);
    s->look_episode = (unsigned *)(base + o_ep);
    for (int p = 0; p < 2; p++) s->snap_look[p] = s->rstream ? (int *)(base + o_snap[p]) : nullptr;
    s->look_sm = SM;
    s->look_variants = copy;
    s->look_has_sampler = sampler != nullptr;
    if (sampler) s->look_sampler = *sampler;
    s->look_K = n_variants;
    if (s->wrist_on) {   // the wrist frames take the look as well
        rc = launch_wrist_frames(s, s->dev, s->stream);
        if (!rc) rc = (int)hipStreamSynchronize(s->stream);
        if (rc) return fail(LCR_ERR_HIP, "drawing the wrist frames with the look failed: %s", hipGetErrorString((hipError_t)rc));
    }
    return LCR_OK;
}

int lcr_set_look(lcr_sim *s, const uint8_t *mask_host, const int32_t *variant_host, const float *rgb_host) {
    SIMCHK(s);
    if (!s->look_K) return fail(LCR_ERR_INVALID, "no look is enabled on this sim (lcr_enable_look)");
    const size_t N = (size_t)s->dev.n;
    for (size_t i = 0; i < N; i++) {
        if (mask_host && !mask_host[i]) continue;
        if (variant_host && (variant_host[i] < 0 || variant_host[i] >= s->look_K)) return fail(LCR_ERR_INVALID, "variant of env %zu is %d, outside 0 .. %d", i, variant_host[i], s->look_K - 1);
        if (rgb_host)
            for (int j = 0; j < 9; j++)
                if (!in_range(rgb_host + (size_t)j * N + i, 1, 0.f, 1.f)) return fail(LCR_ERR_INVALID, "rgb channel %d of env %zu must be finite and in [0, 1]", j, i);
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    std::vector<int> cur(10 * N);
    HIPCHK(hipMemcpy(cur.data(), s->look_cur, sizeof(int) * 10 * N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++) {
        if (mask_host && !mask_host[i]) continue;
        if (variant_host) cur[i] = variant_host[i];
        if (rgb_host)
            for (int j = 0; j < 9; j++) memcpy(&cur[(size_t)(1 + j) * N + i], rgb_host + (size_t)j * N + i, sizeof(float));
    }
    HIPCHK(hipMemcpy(s->look_cur, cur.data(), sizeof(int) * 10 * N, hipMemcpyHostToDevice));
    if (int rc = frames_after(s, s->dev, s->stream, nullptr, nullptr, LCR_STACK_NEWEST)) return rc;   // no time has passed: the newest slot of every env is rewritten
    HIPCHK(hipStreamSynchronize(s->stream));
    return LCR_OK;
}

int lcr_get_look(lcr_sim *s, int32_t *variant, float *rgb, uint32_t *episode) {
    SIMCHK(s);
    if (!s->look_K) return fail(LCR_ERR_INVALID, "no look is enabled on this sim (lcr_enable_look)");
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t N = (size_t)s->dev.n;
    if (variant) HIPCHK(hipMemcpy(variant, s->look_cur, sizeof(int) * N, hipMemcpyDeviceToHost));
    if (rgb) HIPCHK(hipMemcpy(rgb, s->look_cur + N, sizeof(float) * 9 * N, hipMemcpyDeviceToHost));
    if (episode) HIPCHK(hipMemcpy(episode, s->look_episode, sizeof(unsigned) * N, hipMemcpyDeviceToHost));
    return LCR_OK;
}

// ---- the wrist camera ----

int lcr_wrist_camera_default(lcr_wrist_camera *cam) {
    if (!cam) return fail(LCR_ERR_INVALID, "cam is NULL");
    memset(cam, 0, sizeof *cam);
    cam->link = 5;
    cam->pos[0] = 0.03f; cam->pos[1] = 0.0033f; cam->pos[2] = 0.045f;
    const float xy[6] = {0.f, 1.f, 0.f, -0.4226f, 0.f, 0.9063f};   // 25 degrees down along the gripper's -x
    memcpy(cam->xyaxes, xy, sizeof xy);
    cam->fovy_deg = 60.f;
    return LCR_OK;
}

// checks `cam` (include/lcr.h) and finishes its axes in fp64 as cam_finish does for the scene cameras; `height`: rows of the frames it draws
static int wrist_mount(const lcr_wrist_camera *cam, int height, LcrWristMount *out) {
    if (!cam) return fail(LCR_ERR_INVALID, "cam is NULL");
    if (cam->link < 0 || cam->link > 6) return fail(LCR_ERR_INVALID, "link must be 0 (world frame) or 1 .. 6 (link_1 .. link_6), got %d", cam->link);
    const float reach = cam->link == 0 ? 2.f : 0.5f;
    if (!in_range(cam->pos, 3, -reach, reach)) return fail(LCR_ERR_INVALID, "pos must be finite and within +-%g m per component in the frame of link %d", (double)reach, cam->link);
    if (cam->link == 0 && cam->pos[2] < 0.05f) return fail(LCR_ERR_INVALID, "pos leaves a world-frame camera %.3f m above the floor, less than 0.05 m", (double)cam->pos[2]);
    for (int i = 0; i < 6; i++)
        if (!finite_f(cam->xyaxes[i])) return fail(LCR_ERR_INVALID, "xyaxes must be finite");
    if (!in_range(&cam->fovy_deg, 1, 20.f, 120.f)) return fail(LCR_ERR_INVALID, "fovy_deg must be finite and in [20, 120]");
    double X[3], Y[3];
    for (int i = 0; i < 3; i++) { X[i] = (double)cam->xyaxes[i]; Y[i] = (double)cam->xyaxes[3 + i]; }
    const double nx = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    if (!(nx > 0.0)) return fail(LCR_ERR_INVALID, "xyaxes: X is zero");
    for (int i = 0; i < 3; i++) X[i] /= nx;
    const double d = X[0] * Y[0] + X[1] * Y[1] + X[2] * Y[2];
    for (int i = 0; i < 3; i++) Y[i] -= d * X[i];
    const double ny = std::sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]);
    if (ny < 1e-6) return fail(LCR_ERR_INVALID, "xyaxes: Y is parallel to X (norm %.3g after its projection on X is removed)", ny);
    for (int i = 0; i < 3; i++) Y[i] /= ny;
    const double Z[3] = {X[1] * Y[2] - X[2] * Y[1], X[2] * Y[0] - X[0] * Y[2], X[0] * Y[1] - X[1] * Y[0]};
    LcrWristMount &M = *out;
    M.link = cam->link;
    M.px = cam->pos[0]; M.py = cam->pos[1]; M.pz = cam->pos[2];
    M.xx = (float)X[0]; M.xy = (float)X[1]; M.xz = (float)X[2];
    M.yx = (float)Y[0]; M.yy = (float)Y[1]; M.yz = (float)Y[2];
    M.zx = (float)Z[0]; M.zy = (float)Z[1]; M.zz = (float)Z[2];
    M.s = (float)(2.0 * std::tan(0.5 * (double)cam->fovy_deg * M_PI / 180.0) / height);
    return LCR_OK;
}

int lcr_wrist_camera_check(const lcr_wrist_camera *cam) {
    LcrWristMount M;
    return wrist_mount(cam, LCR_IMG_H, &M);
}

int lcr_enable_wrist_camera(lcr_sim *s, const lcr_wrist_camera *cam) {
    // the argument first, the handle afterwards (what can be refused without a device is)
    LcrWristMount M;
    if (int rc = wrist_mount(cam, s ? s->dev.img_h : LCR_IMG_H, &M)) return rc;
    SIMCHK(s);
    if (!s->has_images) return fail(LCR_ERR_INVALID, "sim has no image observations (observation_mode state): there are no frames to add a wrist camera to");
    if (s->wrist_on) {
        if (memcmp(&s->wrist_cam, cam, sizeof *cam) == 0) return LCR_OK;
        return fail(LCR_ERR_INVALID, "a wrist camera on link %d is enabled already and fixed for the life of the handle", s->wrist_cam.link);
    }
    if (s->stack_on) return fail(LCR_ERR_INVALID, "the observation stack is enabled already: enable the wrist camera first and the stack last");
    if (s->planes) return fail(LCR_ERR_INVALID, "the image planes are enabled already: enable the wrist camera first and the planes second (they then cover it)");
    // the frames between two guard regions (include/lcr.h: LCR_WRIST_GUARD)
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    const size_t o_img = C.take((size_t)s->dev.n * s->dev.img_h * s->dev.img_w * 3);
    C.skip(LCR_WRIST_GUARD);
    const size_t bytes = C.off;
    void *mem = nullptr;
    hipError_t e = hipMalloc(&mem, bytes);
    if (e != hipSuccess) return fail(LCR_ERR_OOM, "hipMalloc(%zu bytes) for the wrist frames failed: %s", bytes, hipGetErrorString(e));
    LcrWrist WR{};
    WR.mount = M;
    WR.img = (unsigned char *)mem + o_img;
    int rc = (int)hipMemsetAsync(mem, LCR_WRIST_GUARD_BYTE, bytes, s->stream);
    if (!rc) rc = lcr_launch_render_wrist(s->dev, WR, s->look_K ? &s->look : nullptr, s->stream);
    if (!rc) rc = (int)hipStreamSynchronize(s->stream);
    if (rc) { (void)hipFree(mem); return fail(LCR_ERR_HIP, "drawing the wrist frames failed: %s", hipGetErrorString((hipError_t)rc)); }
    s->wrist = WR;
    s->wrist_mem = mem;
    s->wrist_cam = *cam;
    s->wrist_on = true;
    return LCR_OK;
}

int lcr_get_wrist_camera(lcr_sim *s, lcr_wrist_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the wrist frames are drawn on the second stream after a step: the handle's stream waits for them here)
    memset(out, 0, sizeof *out);
    if (!s->wrist_on) return LCR_OK;
    out->enabled = 1;
    out->camera = s->wrist_cam;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    out->depth_far = s->planes ? s->wrist.far : 0.f;
    out->image_wrist = s->wrist.img;
    out->depth_wrist = s->wrist.depth;
    out->seg_wrist = s->wrist.seg;
    return LCR_OK;
}

int lcr_render_terminal_wrist(lcr_sim *s, const int32_t *env_ids_host, int count, uint8_t *rgb_host, float *depth_host, uint8_t *seg_host) {
    SIMCHK(s);
    if (!s->wrist_on) return fail(LCR_ERR_INVALID, "no wrist camera is enabled on this sim (lcr_enable_wrist_camera)");
    if (count < 0 || (count > 0 && (!env_ids_host || !rgb_host))) return fail(LCR_ERR_INVALID, "NULL argument");
    if ((depth_host && !s->wrist.depth) || (seg_host && !s->wrist.seg)) return fail(LCR_ERR_INVALID, "a plane that is not enabled was asked for (lcr_enable_image_planes)");
    const size_t px = (size_t)s->dev.img_h * s->dev.img_w, img = px * 3, dpx = depth_host ? px * sizeof(float) : 0, spx = seg_host ? px : 0;
    const size_t per_env[] = {img, dpx, spx};   // the colours, the depth, the segmentation
    return render_terminal_passes(s, env_ids_host, count, per_env, [&](LcrDev &P1, const LcrLook &LK, int c, size_t done, char *const *buf) -> int {
        LcrWrist W1 = s->wrist;
        W1.img = (unsigned char *)buf[0];
        W1.depth = (float *)buf[1];
        W1.seg = (unsigned char *)buf[2];
        LAUNCHCHK("render", lcr_launch_render_wrist(P1, W1, s->look_K ? &LK : nullptr, s->stream));
        HIPCHK(hipMemcpyAsync(rgb_host + done * img, buf[0], img * c, hipMemcpyDeviceToHost, s->stream));
        if (depth_host) HIPCHK(hipMemcpyAsync(depth_host + done * px, buf[1], dpx * c, hipMemcpyDeviceToHost, s->stream));
        if (seg_host) HIPCHK(hipMemcpyAsync(seg_host + done * px, buf[2], spx * c, hipMemcpyDeviceToHost, s->stream));
        return LCR_OK;
    });
}

// ---- the observation stack ----

int lcr_obs_stack_check(const lcr_obs_stack_spec *spec) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    if (spec->frames < 1 || spec->frames > LCR_STACK_MAX_FRAMES) return fail(LCR_ERR_INVALID, "frames must lie in 1 .. %d, got %d", LCR_STACK_MAX_FRAMES, spec->frames);
    if (spec->cameras & ~(uint32_t)(LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | LCR_STACK_CAM_WRIST))
        return fail(LCR_ERR_INVALID, "cameras must be a mask of 1 (front), 2 (top) and 4 (wrist), or 0 for every camera of the handle, got %u", spec->cameras);
    if (spec->dtype != LCR_STACK_UINT8 && spec->dtype != LCR_STACK_FLOAT16 && spec->dtype != LCR_STACK_FLOAT32)
        return fail(LCR_ERR_INVALID, "dtype must be 0 (uint8), 1 (float16) or 2 (float32), got %d", spec->dtype);
    if (spec->reset_fill != LCR_STACK_FILL_REPEAT && spec->reset_fill != LCR_STACK_FILL_ZERO)
        return fail(LCR_ERR_INVALID, "reset_fill must be 0 (repeat) or 1 (zero), got %d", spec->reset_fill);
    return LCR_OK;
}

int lcr_enable_obs_stack(lcr_sim *s, const lcr_obs_stack_spec *spec) { return lcr_enable_obs_stack_terminal(s, spec, 0); }

int lcr_enable_obs_stack_terminal(lcr_sim *s, const lcr_obs_stack_spec *spec, int32_t keep_terminal) { return lcr_enable_obs_stack_planes(s, spec, keep_terminal, 0); }

int lcr_enable_obs_stack_planes(lcr_sim *s, const lcr_obs_stack_spec *spec, int32_t keep_terminal, uint32_t planes) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (int rc = lcr_obs_stack_check(spec)) return rc;
    if (keep_terminal != 0 && keep_terminal != 1) return fail(LCR_ERR_INVALID, "keep_terminal must be 0 or 1, got %d", keep_terminal);
    if (planes & ~(uint32_t)(LCR_PLANE_DEPTH | LCR_PLANE_SEGMENTATION))
        return fail(LCR_ERR_INVALID, "planes must be 0 (colours only) or LCR_PLANE_DEPTH (1), got %u", planes);
    if (planes & LCR_PLANE_SEGMENTATION)
        return fail(LCR_ERR_UNSUPPORTED, "the segmentation plane is not stacked: its ids are categorical, and a cast of them is not policy-ready (planes %u; the depth plane, 1, is)", planes);
    SIMCHK(s);
    if (!s->has_images) return fail(LCR_ERR_INVALID, "sim has no image observations (observation_mode state): there are no frames to stack");
    lcr_obs_stack_spec sp = *spec;
    if (sp.cameras == 0) sp.cameras = LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | (s->wrist_on ? LCR_STACK_CAM_WRIST : 0);
    if ((sp.cameras & LCR_STACK_CAM_WRIST) && !s->wrist_on) return fail(LCR_ERR_INVALID, "cameras selects the wrist camera (4), but the sim has none (lcr_enable_wrist_camera, before the stack)");
    if (s->stack_on) {
        if (s->stack_planes != planes)
            return fail(LCR_ERR_INVALID, "an observation stack with planes %u is enabled already and fixed for the life of the handle (asked for planes %u)", s->stack_planes, planes);
        if (memcmp(&s->stack_spec, &sp, sizeof sp) == 0 && s->stack_keep == (keep_terminal == 1)) return LCR_OK;
        if (memcmp(&s->stack_spec, &sp, sizeof sp) == 0)
            return fail(LCR_ERR_INVALID, "an observation stack with keep_terminal %d is enabled already and fixed for the life of the handle (asked for keep_terminal %d)", s->stack_keep ? 1 : 0, keep_terminal);
        return fail(LCR_ERR_INVALID, "an observation stack (frames %d, cameras %u, dtype %d, reset_fill %d) is enabled already and fixed for the life of the handle", s->stack_spec.frames,
                    s->stack_spec.cameras, s->stack_spec.dtype, s->stack_spec.reset_fill);
    }
    // the depth channel is made of the depth plane, which is not switched on silently (the rule of the cloud, the grid and the map)
    const bool dep = planes & LCR_PLANE_DEPTH;
    if (dep && !(s->planes & LCR_PLANE_DEPTH))
        return fail(LCR_ERR_INVALID, "planes asks for the depth channel, but the depth plane of this sim is not enabled (lcr_enable_image_planes with LCR_PLANE_DEPTH, before the stack)");
    LcrStack A{};
    A.cpc = dep ? 4 : 3;
    if (sp.cameras & LCR_STACK_CAM_FRONT) { A.depth[A.ncam] = dep ? s->pl.depth_front : nullptr; A.src[A.ncam++] = s->dev.img_front; }
    if (sp.cameras & LCR_STACK_CAM_TOP) { A.depth[A.ncam] = dep ? s->pl.depth_top : nullptr; A.src[A.ncam++] = s->dev.img_top; }
    if (sp.cameras & LCR_STACK_CAM_WRIST) { A.depth[A.ncam] = dep ? s->wrist.depth : nullptr; A.src[A.ncam++] = s->wrist.img; }
    if (dep) {   // the two constants of the element rule, fixed here: depth_far cannot change once planes are on
        A.inv_far = (float)(1.0 / (double)s->pl.far);
        A.s255 = (float)(255.0 / (double)s->pl.far);
    }
    const size_t N = (size_t)s->dev.n, px = (size_t)s->dev.img_h * s->dev.img_w, esize = sp.dtype == LCR_STACK_UINT8 ? 1 : sp.dtype == LCR_STACK_FLOAT16 ? 2 : 4;
    const size_t per_env = (size_t)sp.frames * A.cpc * A.ncam * px * esize;
    // guard, stack, guard (include/lcr.h: LCR_WRIST_GUARD), then the two snapshots of did_reset
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    const size_t o_dst = C.take(N * per_env);
    C.skip(LCR_WRIST_GUARD);
    // ... with keep_terminal and older slots to keep: the history and a guard behind it (the guard before it is the stack's second)
    const size_t hist_env = keep_terminal && sp.frames > 1 ? (size_t)(sp.frames - 1) * A.cpc * A.ncam * px * esize : 0;
    const size_t o_hist = C.take(N * hist_env);
    if (hist_env) C.skip(LCR_WRIST_GUARD);
    const size_t guarded = C.off;
    size_t o_snap[2] = {C.off, C.off};
    if (s->rstream) for (int p = 0; p < 2; p++) o_snap[p] = C.take(N);
    const size_t off = C.off;
    void *mem = nullptr;
    hipError_t e = hipMalloc(&mem, off);
    if (e != hipSuccess) return fail(LCR_ERR_OOM, "hipMalloc(%zu bytes) for the observation stack failed: %s", off, hipGetErrorString(e));
    char *base = (char *)mem;
    A.dst = base + o_dst;
    A.n = s->dev.n; A.pixels = (int)px; A.frames = sp.frames; A.dtype = sp.dtype;
    A.zero_fill = sp.reset_fill == LCR_STACK_FILL_ZERO;
    A.flags = nullptr; A.op = LCR_STACK_REFILL;
    A.mode = LCR_STACK_MODE_PLAIN; A.ids = nullptr;
    A.history = hist_env ? base + o_hist : nullptr;
    int rc = (int)hipMemsetAsync(mem, LCR_WRIST_GUARD_BYTE, guarded, s->stream);
    if (!rc && off > guarded) rc = (int)hipMemsetAsync(base + guarded, 0, off - guarded, s->stream);
    if (!rc && hist_env) rc = (int)hipMemsetAsync(base + o_hist, 0, N * hist_env, s->stream);   // (the history alone: the padding behind it belongs to its guard)
    if (!rc) rc = lcr_launch_obs_stack(A, s->stream);
    if (rc < 0) { (void)hipStreamSynchronize(s->stream); (void)hipFree(mem); return fail(LCR_ERR_UNSUPPORTED, "the observation stack of %d envs at %d x %d needs more workgroups than one launch takes", s->dev.n, s->dev.img_w, s->dev.img_h); }
    if (!rc) rc = (int)hipStreamSynchronize(s->stream);
    if (rc) { (void)hipFree(mem); return fail(LCR_ERR_HIP, "filling the observation stack failed: %s", hipGetErrorString((hipError_t)rc)); }
    s->stack = A;
    s->stack_mem = mem;
    s->stack_spec = sp;
    s->stack_bytes_per_env = per_env;
    s->stack_keep = keep_terminal == 1;
    s->stack_hist_bytes_per_env = hist_env;
    s->stack_planes = planes;
    for (int p = 0; p < 2; p++) s->snap_reset[p] = s->rstream ? (unsigned char *)(base + o_snap[p]) : nullptr;
    s->stack_on = true;
    return LCR_OK;
}

int lcr_get_obs_stack(lcr_sim *s, lcr_obs_stack_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the stack is made behind the frames, on the second stream after a step: the handle's stream waits for it here)
    memset(out, 0, sizeof *out);
    if (!s->stack_on) return LCR_OK;
    out->enabled = 1;
    out->spec = s->stack_spec;
    out->channels = s->stack.cpc * s->stack.ncam;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    out->data = s->stack.dst;
    out->bytes_per_env = (uint64_t)s->stack_bytes_per_env;
    return LCR_OK;
}

int lcr_get_obs_stack_planes(lcr_sim *s, uint32_t *planes, float *inv_far, float *s255) {
    if (!s || !planes || !inv_far || !s255) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (a joining entry point, as lcr_get_obs_stack is)
    const bool dep = s->stack_on && (s->stack_planes & LCR_PLANE_DEPTH);
    *planes = s->stack_on ? s->stack_planes : 0;
    *inv_far = dep ? s->stack.inv_far : 0.f;
    *s255 = dep ? s->stack.s255 : 0.f;
    return LCR_OK;
}

int lcr_get_obs_stack_terminal(lcr_sim *s, int32_t *keep_terminal, const void **history, uint64_t *history_bytes_per_env) {
    if (!s || !keep_terminal || !history || !history_bytes_per_env) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (a joining entry point, as lcr_get_obs_stack is: the history is written by the stack kernel, on the second stream after a step)
    const bool on = s->stack_on && s->stack_keep;
    *keep_terminal = on ? 1 : 0;
    *history = on ? s->stack.history : nullptr;
    *history_bytes_per_env = on ? (uint64_t)s->stack_hist_bytes_per_env : 0;
    return LCR_OK;
}

int lcr_obs_stack_terminal(lcr_sim *s, const int32_t *env_ids_host, int count, void *out_host) {
    SIMCHK(s);
    if (!s->stack_on) return fail(LCR_ERR_INVALID, "no observation stack is enabled on this sim (lcr_enable_obs_stack_terminal)");
    if (!s->stack_keep) return fail(LCR_ERR_INVALID, "the observation stack of this sim was enabled without keep_terminal: the history of an episode that ends is not kept (lcr_enable_obs_stack_terminal)");
    if (count < 0 || (count > 0 && (!env_ids_host || !out_host))) return fail(LCR_ERR_INVALID, "NULL argument");
    const size_t px = (size_t)s->dev.img_h * s->dev.img_w, img = px * 3, env_out = s->stack_bytes_per_env;
    const bool wrist = s->stack_spec.cameras & LCR_STACK_CAM_WRIST;
    // with the depth channel: the terminal depth planes too, drawn as lcr_render_terminal_planes / lcr_render_terminal_wrist draw them (0 bytes without it: no room taken)
    const bool dep = s->stack_planes & LCR_PLANE_DEPTH;
    const size_t dpx = dep ? px * sizeof(float) : 0;
    // the terminal frames of front, top and -- if it is stacked -- wrist, the terminal stacks, the terminal depth planes of the three
    const size_t per_env[] = {img, img, wrist ? img : 0, env_out, dpx, dpx, wrist ? dpx : 0};
    return render_terminal_passes(s, env_ids_host, count, per_env, [&](LcrDev &P1, const LcrLook &LK, int c, size_t done, char *const *buf) -> int {
        P1.img_front = (unsigned char *)buf[0];
        P1.img_top = (unsigned char *)buf[1];
        if (dep) {
            LcrPlanes PL1 = s->pl;
            PL1.depth_front = (float *)buf[4];
            PL1.depth_top = (float *)buf[5];
            PL1.seg_front = nullptr; PL1.seg_top = nullptr;
            if (s->look_K) LAUNCHCHK("render", lcr_launch_render_obs_look(P1, LK, &PL1, s->stream));
            else LAUNCHCHK("render", lcr_launch_render_obs_planes(P1, s->cam_front, s->cam_top, PL1, s->stream));
        } else if (s->look_K) LAUNCHCHK("render", lcr_launch_render_obs_look(P1, LK, nullptr, s->stream));
        else LAUNCHCHK("render", lcr_launch_render_obs(P1, s->cam_front, s->cam_top, s->stream));
        if (wrist) {
            LcrWrist W1 = s->wrist;
            W1.img = (unsigned char *)buf[2];
            W1.depth = (float *)buf[6]; W1.seg = nullptr;   // (buf[6] is null without the depth channel)
            LAUNCHCHK("render", lcr_launch_render_wrist(P1, W1, s->look_K ? &LK : nullptr, s->stream));
        }
        // slots 0 .. K - 2 from the history of the listed envs, slot K - 1 the terminal frames by the stack's transpose and cast
        LcrStack A = s->stack;
        A.ncam = 0;
        if (s->stack_spec.cameras & LCR_STACK_CAM_FRONT) { A.depth[A.ncam] = (const float *)buf[4]; A.src[A.ncam++] = (const unsigned char *)buf[0]; }
        if (s->stack_spec.cameras & LCR_STACK_CAM_TOP) { A.depth[A.ncam] = (const float *)buf[5]; A.src[A.ncam++] = (const unsigned char *)buf[1]; }
        if (wrist) { A.depth[A.ncam] = (const float *)buf[6]; A.src[A.ncam++] = (const unsigned char *)buf[2]; }
        A.dst = buf[3];
        A.n = c;
        A.flags = nullptr; A.op = LCR_STACK_NEWEST;
        A.mode = LCR_STACK_MODE_TERMINAL;
        A.ids = (const int *)s->term_stage;   // (the ids of this pass lie first in the staging: render_terminal_passes)
        LAUNCHCHK("stack kernel", lcr_launch_obs_stack(A, s->stream));
        HIPCHK(hipMemcpyAsync((char *)out_host + done * env_out, buf[3], env_out * c, hipMemcpyDeviceToHost, s->stream));
        return LCR_OK;
    });
}

// ---- the point cloud ----

int lcr_point_cloud_check(const lcr_point_cloud_spec *spec) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    if (spec->points < 64 || spec->points > 8192 || spec->points % 64 != 0) return fail(LCR_ERR_INVALID, "points must be a multiple of 64 in 64 .. 8192, got %d", spec->points);
    if (spec->cameras & ~(uint32_t)(LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | LCR_STACK_CAM_WRIST))
        return fail(LCR_ERR_INVALID, "cameras must be a mask of 1 (front), 2 (top) and 4 (wrist), or 0 for every camera of the handle, got %u", spec->cameras);
    if (spec->ids & ~(uint32_t)0x7FEu)
        return fail(LCR_ERR_INVALID, "ids must be a mask over the surface ids 1 .. 10 (bits 1 .. 10; bit 0 is the sky, which is no surface), or 0 for arm and cubes (0x7FC), got 0x%x", spec->ids);
    if (spec->colors != 0 && spec->colors != 1) return fail(LCR_ERR_INVALID, "colors must be 0 (x y z) or 1 (x y z r g b), got %d", spec->colors);
    return LCR_OK;
}

static const char *cloud_mode_name(int mode) { return mode == LCR_CLOUD_SAMPLE_FPS ? "fps" : "stride"; }

int lcr_point_cloud_sampling_check(const lcr_point_cloud_spec *spec, const lcr_point_cloud_sampling *sampling) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    if (!sampling) return fail(LCR_ERR_INVALID, "sampling is NULL");
    if (sampling->mode != LCR_CLOUD_SAMPLE_STRIDE && sampling->mode != LCR_CLOUD_SAMPLE_FPS)
        return fail(LCR_ERR_INVALID, "mode must be 0 (stride) or 1 (farthest-point sampling), got %d", sampling->mode);
    if (sampling->mode == LCR_CLOUD_SAMPLE_STRIDE) {
        if (sampling->pool != 0) return fail(LCR_ERR_INVALID, "pool must be 0 with mode 0 (stride): a strided cloud has no pool, got %d", sampling->pool);
        return LCR_OK;
    }
    if (sampling->pool < 64 || sampling->pool > LCR_CLOUD_MAX_POOL || sampling->pool % 64 != 0)
        return fail(LCR_ERR_INVALID, "pool must be a multiple of 64 in 64 .. %d, got %d", LCR_CLOUD_MAX_POOL, sampling->pool);
    if (sampling->pool < spec->points)
        return fail(LCR_ERR_INVALID, "pool must be at least points (farthest-point sampling picks %d points out of the pool, which caps points at %d), got %d", spec->points,
                    LCR_CLOUD_MAX_POOL, sampling->pool);
    return LCR_OK;
}

int lcr_point_cloud_crop_check(const lcr_point_cloud_crop *crop) {
    if (!crop) return fail(LCR_ERR_INVALID, "crop is NULL");
    static const char *const axis = "xyz";
    // (by the bits: this unit is built with -ffast-math, under which x != x is no NaN test)
    const auto is_nan = [](float v) { uint32_t b; memcpy(&b, &v, sizeof b); return (b & 0x7fffffffu) > 0x7f800000u; };
    for (int k = 0; k < 3; k++) {
        if (is_nan(crop->lo[k])) return fail(LCR_ERR_INVALID, "lo[%d] (%c) is NaN: every side of the crop box is finite or an infinity (an open side)", k, axis[k]);
        if (is_nan(crop->hi[k])) return fail(LCR_ERR_INVALID, "hi[%d] (%c) is NaN: every side of the crop box is finite or an infinity (an open side)", k, axis[k]);
    }
    for (int k = 0; k < 3; k++)
        if (crop->lo[k] > crop->hi[k])
            return fail(LCR_ERR_INVALID, "lo[%d] > hi[%d]: the crop box is empty along %c (lo %.9g, hi %.9g)", k, k, axis[k], (double)crop->lo[k], (double)crop->hi[k]);
    return LCR_OK;
}

int lcr_enable_point_cloud(lcr_sim *s, const lcr_point_cloud_spec *spec) { return lcr_enable_point_cloud_cropped(s, spec, nullptr, nullptr); }

int lcr_enable_point_cloud_sampled(lcr_sim *s, const lcr_point_cloud_spec *spec, const lcr_point_cloud_sampling *sampling) {
    return lcr_enable_point_cloud_cropped(s, spec, sampling, nullptr);
}

// "; crop lo (x y z) hi (x y z)" or "; no crop" into buf: how the refusals name a box
static const char *cloud_crop_text(char (&buf)[200], bool on, const lcr_point_cloud_crop &c) {
    if (!on) snprintf(buf, sizeof buf, "no crop");
    else snprintf(buf, sizeof buf, "crop lo (%.9g %.9g %.9g) hi (%.9g %.9g %.9g)", (double)c.lo[0], (double)c.lo[1], (double)c.lo[2], (double)c.hi[0], (double)c.hi[1], (double)c.hi[2]);
    return buf;
}

int lcr_enable_point_cloud_cropped(lcr_sim *s, const lcr_point_cloud_spec *spec, const lcr_point_cloud_sampling *sampling, const lcr_point_cloud_crop *crop) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (int rc = lcr_point_cloud_check(spec)) return rc;
    const lcr_point_cloud_sampling sm = sampling ? *sampling : lcr_point_cloud_sampling{LCR_CLOUD_SAMPLE_STRIDE, 0};
    if (int rc = lcr_point_cloud_sampling_check(spec, &sm)) return rc;
    if (crop)
        if (int rc = lcr_point_cloud_crop_check(crop)) return rc;
    const lcr_point_cloud_crop cr = crop ? *crop : lcr_point_cloud_crop{};
    SIMCHK(s);
    lcr_point_cloud_spec sp = *spec;
    if (int rc = planes_ready(s, &sp.cameras, "to make a point cloud of", "the point cloud needs", "the cloud")) return rc;
    if (sp.ids == 0) sp.ids = LCR_CLOUD_DEFAULT_IDS;
    if (s->cloud_on) {
        // (the boxes compare as float32 values: the comparisons the kernel makes with them are the same then; no side is a NaN)
        bool same_crop = s->cloud_crop_on == (crop != nullptr);
        for (int k = 0; k < 3 && same_crop && crop; k++) same_crop = s->cloud_crop.lo[k] == cr.lo[k] && s->cloud_crop.hi[k] == cr.hi[k];
        if (memcmp(&s->cloud_spec, &sp, sizeof sp) == 0 && s->cloud_sampling.mode == sm.mode && s->cloud_sampling.pool == sm.pool && same_crop) return LCR_OK;
        if (s->cloud_crop_on || crop) {
            char was[200], asked[200];
            return fail(LCR_ERR_INVALID, "a point cloud (points %d, cameras %u, ids 0x%x, colors %d; sampling %s, pool %d; %s) is enabled already and fixed for the life of the "
                        "handle: asked for points %d, cameras %u, ids 0x%x, colors %d; sampling %s, pool %d; %s", s->cloud_spec.points, s->cloud_spec.cameras, s->cloud_spec.ids,
                        s->cloud_spec.colors, cloud_mode_name(s->cloud_sampling.mode), s->cloud_sampling.pool, cloud_crop_text(was, s->cloud_crop_on, s->cloud_crop), sp.points,
                        sp.cameras, sp.ids, sp.colors, cloud_mode_name(sm.mode), sm.pool, cloud_crop_text(asked, crop != nullptr, cr));
        }
        if (s->cloud_sampling.mode == LCR_CLOUD_SAMPLE_STRIDE && sm.mode == LCR_CLOUD_SAMPLE_STRIDE)
            return fail(LCR_ERR_INVALID, "a point cloud (points %d, cameras %u, ids 0x%x, colors %d) is enabled already and fixed for the life of the handle", s->cloud_spec.points,
                        s->cloud_spec.cameras, s->cloud_spec.ids, s->cloud_spec.colors);
        return fail(LCR_ERR_INVALID, "a point cloud (points %d, cameras %u, ids 0x%x, colors %d; sampling %s, pool %d) is enabled already and fixed for the life of the handle: "
                    "asked for points %d, cameras %u, ids 0x%x, colors %d; sampling %s, pool %d", s->cloud_spec.points, s->cloud_spec.cameras, s->cloud_spec.ids,
                    s->cloud_spec.colors, cloud_mode_name(s->cloud_sampling.mode), s->cloud_sampling.pool, sp.points, sp.cameras, sp.ids, sp.colors, cloud_mode_name(sm.mode), sm.pool);
    }
    LcrCloud A{};
    ObsSource src[3];
    A.slots = sources(s, sp.cameras, src);
    for (int i = 0; i < A.slots; i++) { A.cam[i] = src[i].cam; A.seg[i] = src[i].seg; A.depth[i] = src[i].depth; A.rgb[i] = src[i].rgb; }
    const size_t N = (size_t)s->dev.n, P = (size_t)sp.points, Cn = sp.colors ? 6 : 3;
    // guard, points, guard (include/lcr.h: LCR_WRIST_GUARD), then count, source and the camera poses
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    const size_t o_pts = C.take(N * P * Cn * sizeof(float));
    C.skip(LCR_WRIST_GUARD);
    const size_t guarded = C.off;
    const size_t o_cnt = C.take(N * sizeof(int));
    const size_t o_src = C.take(N * P * sizeof(int));
    const size_t o_pose = C.take((size_t)A.slots * 13 * N * sizeof(float));
    A.n = s->dev.n; A.W = s->dev.img_w; A.H = s->dev.img_h;
    A.points = sp.points; A.channels = (int)Cn; A.ids = sp.ids;
    A.mount = s->wrist.mount;
    void *mem = nullptr;
    const int rc = bring_up(s, C, guarded, "the point cloud", &mem,
        [&](char *base) {
            A.out = (float *)(base + o_pts);
            A.count = (int *)(base + o_cnt);
            A.source = (int *)(base + o_src);
            A.pose = (float *)(base + o_pose);
            s->cloud = A;
            s->cloud_sampling = sm;
            s->cloud_crop_on = crop != nullptr;
            s->cloud_crop = cr;
            return launch_cloud(s, s->dev, s->stream, nullptr);
        },
        [s] { s->cloud = LcrCloud{}; s->cloud_sampling = lcr_point_cloud_sampling{}; s->cloud_crop_on = false; s->cloud_crop = lcr_point_cloud_crop{}; });
    if (rc == LCR_ERR_UNSUPPORTED) return fail(LCR_ERR_UNSUPPORTED, "the point-cloud kernel is not built for %d cameras at %d x %d", A.slots, A.W, A.H);
    if (rc) return rc;
    s->cloud_mem = mem;
    s->cloud_spec = sp;
    s->cloud_on = true;
    return LCR_OK;
}

int lcr_get_point_cloud(lcr_sim *s, lcr_point_cloud_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the cloud is made behind the frames, on the second stream after a step: the handle's stream waits for it here)
    memset(out, 0, sizeof *out);
    if (!s->cloud_on) return LCR_OK;
    out->enabled = 1;
    out->spec = s->cloud_spec;
    out->channels = s->cloud.channels;
    out->slots = s->cloud.slots;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    out->points = s->cloud.out;
    out->count = s->cloud.count;
    out->source = s->cloud.source;
    out->camera_pose = s->cloud.pose;
    out->bytes_per_env = (uint64_t)s->cloud.points * s->cloud.channels * sizeof(float);
    return LCR_OK;
}

int lcr_get_point_cloud_sampling(lcr_sim *s, lcr_point_cloud_sampling *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (a joining entry point, as lcr_get_point_cloud is)
    *out = s->cloud_on ? s->cloud_sampling : lcr_point_cloud_sampling{LCR_CLOUD_SAMPLE_STRIDE, 0};
    return LCR_OK;
}

int lcr_get_point_cloud_crop(lcr_sim *s, int32_t *enabled, lcr_point_cloud_crop *out) {
    if (!s || !enabled || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (a joining entry point, as lcr_get_point_cloud is)
    const bool on = s->cloud_on && s->cloud_crop_on;
    *enabled = on ? 1 : 0;
    *out = on ? s->cloud_crop : lcr_point_cloud_crop{};
    return LCR_OK;
}

int lcr_point_cloud_terminal(lcr_sim *s, const int32_t *env_ids_host, int count, float *points_host, int32_t *count_host, int32_t *source_host, float *pose_host) {
    SIMCHK(s);
    if (!s->cloud_on) return fail(LCR_ERR_INVALID, "no point cloud is enabled on this sim (lcr_enable_point_cloud)");
    if (count < 0 || (count > 0 && !env_ids_host)) return fail(LCR_ERR_INVALID, "NULL argument");
    const bool wrist = s->cloud_spec.cameras & LCR_STACK_CAM_WRIST;
    const size_t px = (size_t)s->dev.img_h * s->dev.img_w, img = px * 3, dpx = px * sizeof(float), wi = wrist ? img : 0, wd = wrist ? dpx : 0, ws = wrist ? px : 0;
    const size_t P = (size_t)s->cloud.points, pts = P * s->cloud.channels * sizeof(float), src = P * sizeof(int), pose = (size_t)s->cloud.slots * 13 * sizeof(float);
    // front, top of the colours, the depths, the segmentations; the wrist camera's three if it is selected; then what the cloud kernel writes: points, count, source, poses
    const size_t per_env[] = {img, img, dpx, dpx, px, px, wi, wd, ws, pts, sizeof(int), src, pose};
    return render_terminal_passes(s, env_ids_host, count, per_env, [&](LcrDev &P1, const LcrLook &LK, int c, size_t done, char *const *buf) -> int {
        P1.img_front = (unsigned char *)buf[0];
        P1.img_top = (unsigned char *)buf[1];
        LcrPlanes PL1 = s->pl;
        PL1.depth_front = (float *)buf[2];
        PL1.depth_top = (float *)buf[3];
        PL1.seg_front = (unsigned char *)buf[4];
        PL1.seg_top = (unsigned char *)buf[5];
        if (s->look_K) LAUNCHCHK("render", lcr_launch_render_obs_look(P1, LK, &PL1, s->stream));
        else LAUNCHCHK("render", lcr_launch_render_obs_planes(P1, s->cam_front, s->cam_top, PL1, s->stream));
        if (wrist) {
            LcrWrist W1 = s->wrist;
            W1.img = (unsigned char *)buf[6];
            W1.depth = (float *)buf[7];
            W1.seg = (unsigned char *)buf[8];
            LAUNCHCHK("render", lcr_launch_render_wrist(P1, W1, s->look_K ? &LK : nullptr, s->stream));
        }
        // the handle's own cloud kernel over the view: planes, frames and outputs in the staging, the wrist pose from the gathered terminal poses, the terminal looks
        LcrCloud A = s->cloud;
        A.n = c;
        for (int i = 0; i < A.slots; i++) {
            const int b = A.cam[i] == LCR_CLOUD_CAM_FRONT ? 0 : A.cam[i] == LCR_CLOUD_CAM_TOP ? 1 : 2;
            A.rgb[i] = (const unsigned char *)buf[b == 2 ? 6 : b];
            A.depth[i] = (const float *)buf[b == 2 ? 7 : 2 + b];
            A.seg[i] = (const unsigned char *)buf[b == 2 ? 8 : 4 + b];
        }
        A.out = (float *)buf[9];
        A.count = (int *)buf[10];
        A.source = (int *)buf[11];
        A.pose = (float *)buf[12];   // [slots][13][c]
        LAUNCHCHK("point-cloud kernel", launch_cloud(s, P1, s->stream, s->look_K ? LK.variant : nullptr, &A));
        if (points_host) HIPCHK(hipMemcpyAsync((char *)points_host + done * pts, buf[9], pts * c, hipMemcpyDeviceToHost, s->stream));
        if (count_host) HIPCHK(hipMemcpyAsync(count_host + done, buf[10], sizeof(int) * c, hipMemcpyDeviceToHost, s->stream));
        if (source_host) HIPCHK(hipMemcpyAsync(source_host + done * P, buf[11], src * c, hipMemcpyDeviceToHost, s->stream));
        if (pose_host)   // the pass's columns of [slots][13][count]
            HIPCHK(hipMemcpy2DAsync(pose_host + done, sizeof(float) * count, buf[12], sizeof(float) * c, sizeof(float) * c, (size_t)s->cloud.slots * 13, hipMemcpyDeviceToHost, s->stream));
        return LCR_OK;
    });
}

// ---- the voxel grid ----

static const char *voxel_dtype_name(int dtype) { return dtype == LCR_STACK_FLOAT32 ? "float32" : "uint8"; }

int lcr_voxel_grid_check(const lcr_voxel_grid_spec *spec) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    static const char *const axis = "xyz";
    // (by the bits, read as an integer from the struct: this unit is built with -ffast-math, under which no test of a float VALUE for NaN or infinity survives)
    const auto finite = [](const float *v) { uint32_t b; memcpy(&b, v, sizeof b); return (b & 0x7f800000u) != 0x7f800000u; };
    for (int k = 0; k < 3; k++) {
        if (!finite(&spec->lo[k])) return fail(LCR_ERR_INVALID, "lo[%d] (%c) is not finite: the box of a voxel grid has no open sides", k, axis[k]);
        if (!finite(&spec->hi[k])) return fail(LCR_ERR_INVALID, "hi[%d] (%c) is not finite: the box of a voxel grid has no open sides", k, axis[k]);
    }
    for (int k = 0; k < 3; k++)
        if (!(spec->lo[k] < spec->hi[k]))
            return fail(LCR_ERR_INVALID, "lo[%d] >= hi[%d]: the box is empty along %c (lo %.9g, hi %.9g)", k, k, axis[k], (double)spec->lo[k], (double)spec->hi[k]);
    for (int k = 0; k < 3; k++)
        if (spec->dims[k] < 1 || spec->dims[k] > LCR_VOXEL_MAX_DIM)
            return fail(LCR_ERR_INVALID, "dims[%d] (%c) must be in 1 .. %d, got %d", k, axis[k], LCR_VOXEL_MAX_DIM, spec->dims[k]);
    if (spec->dims[0] % 4 != 0) return fail(LCR_ERR_INVALID, "dims[0] (x) must be a multiple of 4 (the kernel writes four voxels along x at a time), got %d", spec->dims[0]);
    if ((int64_t)spec->dims[0] * spec->dims[1] * spec->dims[2] > LCR_VOXEL_MAX_CELLS)
        return fail(LCR_ERR_INVALID, "dims %d x %d x %d are %lld voxels: at most %d", spec->dims[0], spec->dims[1], spec->dims[2],
                    (long long)spec->dims[0] * spec->dims[1] * spec->dims[2], LCR_VOXEL_MAX_CELLS);
    if (spec->cameras & ~(uint32_t)(LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | LCR_STACK_CAM_WRIST))
        return fail(LCR_ERR_INVALID, "cameras must be a mask of 1 (front), 2 (top) and 4 (wrist), or 0 for every camera of the handle, got %u", spec->cameras);
    if (spec->ids & ~(uint32_t)0x7FEu)
        return fail(LCR_ERR_INVALID, "ids must be a mask over the surface ids 1 .. 10 (bits 1 .. 10; bit 0 is the sky, which is no surface), or 0 for arm and cubes (0x7FC), got 0x%x", spec->ids);
    if (spec->features & ~(uint32_t)(LCR_VOXEL_OCCUPANCY | LCR_VOXEL_RGB))
        return fail(LCR_ERR_INVALID, "features must be a mask of 1 (occupancy, implied) and 2 (rgb), got %u", spec->features);
    if (spec->dtype != LCR_STACK_UINT8 && spec->dtype != LCR_STACK_FLOAT32)
        return fail(LCR_ERR_INVALID, "dtype must be 0 (uint8) or 2 (float32): a voxel grid has no float16 elements, got %d", spec->dtype);
    if (spec->source != 0 && spec->source != 1) return fail(LCR_ERR_INVALID, "source must be 0 or 1, got %d", spec->source);
    return LCR_OK;
}

// "box (x y z) .. (x y z), dims a x b x c, cameras, ids, features, dtype, source" into buf: how the refusal names a spec
static const char *voxel_spec_text(char (&buf)[320], const lcr_voxel_grid_spec &v) {
    snprintf(buf, sizeof buf, "box (%.9g %.9g %.9g) .. (%.9g %.9g %.9g), dims %d x %d x %d, cameras %u, ids 0x%x, features %u, dtype %s, source %d", (double)v.lo[0], (double)v.lo[1],
             (double)v.lo[2], (double)v.hi[0], (double)v.hi[1], (double)v.hi[2], v.dims[0], v.dims[1], v.dims[2], v.cameras, v.ids, v.features, voxel_dtype_name(v.dtype), v.source);
    return buf;
}

int lcr_enable_voxel_grid(lcr_sim *s, const lcr_voxel_grid_spec *spec) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (int rc = lcr_voxel_grid_check(spec)) return rc;
    SIMCHK(s);
    lcr_voxel_grid_spec sp = *spec;
    if (int rc = planes_ready(s, &sp.cameras, "to make a voxel grid of", "the voxel grid needs", "the grid")) return rc;
    if (sp.ids == 0) sp.ids = LCR_CLOUD_DEFAULT_IDS;
    sp.features |= LCR_VOXEL_OCCUPANCY;
    if (s->voxel_on) {
        // (the boxes compare as float32 values: the kernel then forms the same cells; no corner is a NaN)
        bool same = memcmp(sp.dims, s->voxel_spec.dims, sizeof sp.dims) == 0 && sp.cameras == s->voxel_spec.cameras && sp.ids == s->voxel_spec.ids &&
                    sp.features == s->voxel_spec.features && sp.dtype == s->voxel_spec.dtype && sp.source == s->voxel_spec.source;
        for (int k = 0; k < 3 && same; k++) same = sp.lo[k] == s->voxel_spec.lo[k] && sp.hi[k] == s->voxel_spec.hi[k];
        if (same) return LCR_OK;
        char was[320], asked[320];
        return fail(LCR_ERR_INVALID, "a voxel grid (%s) is enabled already and fixed for the life of the handle: asked for %s", voxel_spec_text(was, s->voxel_spec), voxel_spec_text(asked, sp));
    }
    LcrVoxel A{};
    ObsSource src[3];
    A.slots = sources(s, sp.cameras, src);
    for (int i = 0; i < A.slots; i++) { A.cam[i] = src[i].cam; A.seg[i] = src[i].seg; A.depth[i] = src[i].depth; A.rgb[i] = src[i].rgb; }
    const size_t N = (size_t)s->dev.n, V = (size_t)sp.dims[0] * sp.dims[1] * sp.dims[2], Cn = (sp.features & LCR_VOXEL_RGB) ? 4 : 1, esize = sp.dtype == LCR_STACK_FLOAT32 ? 4 : 1;
    // guard, voxels, guard (include/lcr.h: LCR_WRIST_GUARD), then source, count, occupied and the camera poses
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    const size_t o_vox = C.take(N * Cn * V * esize);
    C.skip(LCR_WRIST_GUARD);
    const size_t guarded = C.off;
    const size_t o_src = C.take(sp.source ? N * V * sizeof(int) : 0);
    const size_t o_cnt = C.take(N * sizeof(int));
    const size_t o_occ = C.take(N * sizeof(int));
    const size_t o_pose = C.take((size_t)A.slots * 13 * N * sizeof(float));
    A.n = s->dev.n; A.W = s->dev.img_w; A.H = s->dev.img_h;
    A.ids = sp.ids;
    for (int k = 0; k < 3; k++) {
        A.lo[k] = sp.lo[k];
        A.inv[k] = (float)((double)sp.dims[k] / ((double)sp.hi[k] - (double)sp.lo[k]));   // the header's inv_k: formed once, here, and reported
        A.D[k] = sp.dims[k];
    }
    A.channels = (int)Cn; A.f32 = sp.dtype == LCR_STACK_FLOAT32;
    const char *lds = getenv("LCR_VOXEL_LDS");
    A.lds = lds && !strcmp(lds, "big") ? LCR_VOXEL_LDS_BIG : lds && !strcmp(lds, "slab") ? LCR_VOXEL_LDS_SLAB : LCR_VOXEL_LDS_AUTO;
    A.mount = s->wrist.mount;
    void *mem = nullptr;
    const int rc = bring_up(s, C, guarded, "the voxel grid", &mem,
        [&](char *base) {
            A.out = base + o_vox;
            A.source = sp.source ? (int *)(base + o_src) : nullptr;
            A.count = (int *)(base + o_cnt);
            A.occupied = (int *)(base + o_occ);
            A.pose = (float *)(base + o_pose);
            s->voxel = A;
            return launch_voxel(s, s->dev, s->stream, nullptr);
        },
        [s] { s->voxel = LcrVoxel{}; });
    if (rc == LCR_ERR_UNSUPPORTED)
        return fail(LCR_ERR_UNSUPPORTED, "the voxel-grid kernel is not built for %d cameras at %d x %d with cells of %.9g x %.9g x %.9g per metre", A.slots, A.W, A.H, (double)A.inv[0],
                    (double)A.inv[1], (double)A.inv[2]);
    if (rc) return rc;
    s->voxel_mem = mem;
    s->voxel_spec = sp;
    s->voxel_bytes_per_env = Cn * V * esize;
    s->voxel_on = true;
    return LCR_OK;
}

int lcr_get_voxel_grid(lcr_sim *s, lcr_voxel_grid_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the grid is made behind the frames, on the second stream after a step: the handle's stream waits for it here)
    memset(out, 0, sizeof *out);
    if (!s->voxel_on) return LCR_OK;
    out->enabled = 1;
    out->spec = s->voxel_spec;
    for (int k = 0; k < 3; k++) out->inv_cell[k] = s->voxel.inv[k];
    out->channels = s->voxel.channels;
    out->slots = s->voxel.slots;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    out->voxels = s->voxel.out;
    out->source = s->voxel.source;
    out->count = s->voxel.count;
    out->occupied = s->voxel.occupied;
    out->camera_pose = s->voxel.pose;
    out->bytes_per_env = (uint64_t)s->voxel_bytes_per_env;
    return LCR_OK;
}

// ---- the heightmap ----

int lcr_heightmap_check(const lcr_heightmap_spec *spec) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    static const char *const axis = "xyz";
    // (by the bits, read as an integer from the struct: this unit is built with -ffast-math, under which no test of a float VALUE for NaN or infinity survives)
    const auto finite = [](const float *v) { uint32_t b; memcpy(&b, v, sizeof b); return (b & 0x7f800000u) != 0x7f800000u; };
    for (int k = 0; k < 3; k++) {
        if (!finite(&spec->lo[k])) return fail(LCR_ERR_INVALID, "lo[%d] (%c) is not finite: the box of a heightmap has no open sides", k, axis[k]);
        if (!finite(&spec->hi[k])) return fail(LCR_ERR_INVALID, "hi[%d] (%c) is not finite: the box of a heightmap has no open sides", k, axis[k]);
    }
    for (int k = 0; k < 3; k++)
        if (!(spec->lo[k] < spec->hi[k]))
            return fail(LCR_ERR_INVALID, "lo[%d] >= hi[%d]: the box is empty along %c (lo %.9g, hi %.9g)", k, k, axis[k], (double)spec->lo[k], (double)spec->hi[k]);
    for (int k = 0; k < 2; k++)
        if (spec->dims[k] < 1 || spec->dims[k] > LCR_HEIGHTMAP_MAX_DIM)
            return fail(LCR_ERR_INVALID, "dims[%d] (%c) must be in 1 .. %d, got %d", k, axis[k], LCR_HEIGHTMAP_MAX_DIM, spec->dims[k]);
    if (spec->dims[0] % 4 != 0) return fail(LCR_ERR_INVALID, "dims[0] (x) must be a multiple of 4 (the kernel writes four cells along x at a time), got %d", spec->dims[0]);
    if ((int64_t)spec->dims[0] * spec->dims[1] > LCR_HEIGHTMAP_MAX_CELLS)
        return fail(LCR_ERR_INVALID, "dims %d x %d are %lld cells: at most %d", spec->dims[0], spec->dims[1], (long long)spec->dims[0] * spec->dims[1], LCR_HEIGHTMAP_MAX_CELLS);
    if (spec->cameras & ~(uint32_t)(LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | LCR_STACK_CAM_WRIST))
        return fail(LCR_ERR_INVALID, "cameras must be a mask of 1 (front), 2 (top) and 4 (wrist), or 0 for every camera of the handle, got %u", spec->cameras);
    if (spec->ids & ~(uint32_t)0x7FEu)
        return fail(LCR_ERR_INVALID, "ids must be a mask over the surface ids 1 .. 10 (bits 1 .. 10; bit 0 is the sky, which is no surface), or 0 for arm and cubes (0x7FC), got 0x%x", spec->ids);
    if (spec->features & ~(uint32_t)(LCR_HEIGHTMAP_HEIGHT | LCR_HEIGHTMAP_RGB))
        return fail(LCR_ERR_INVALID, "features must be a mask of 1 (height, implied) and 2 (rgb), got %u", spec->features);
    if (spec->source != 0 && spec->source != 1) return fail(LCR_ERR_INVALID, "source must be 0 or 1, got %d", spec->source);
    return LCR_OK;
}

// "box (x y z) .. (x y z), dims a x b, cameras, ids, features, source" into buf: how the refusal names a spec
static const char *heightmap_spec_text(char (&buf)[320], const lcr_heightmap_spec &v) {
    snprintf(buf, sizeof buf, "box (%.9g %.9g %.9g) .. (%.9g %.9g %.9g), dims %d x %d, cameras %u, ids 0x%x, features %u, source %d", (double)v.lo[0], (double)v.lo[1],
             (double)v.lo[2], (double)v.hi[0], (double)v.hi[1], (double)v.hi[2], v.dims[0], v.dims[1], v.cameras, v.ids, v.features, v.source);
    return buf;
}

int lcr_enable_heightmap(lcr_sim *s, const lcr_heightmap_spec *spec) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (int rc = lcr_heightmap_check(spec)) return rc;
    SIMCHK(s);
    lcr_heightmap_spec sp = *spec;
    if (int rc = planes_ready(s, &sp.cameras, "to make a heightmap of", "the heightmap needs", "the map")) return rc;
    if (sp.ids == 0) sp.ids = LCR_CLOUD_DEFAULT_IDS;
    sp.features |= LCR_HEIGHTMAP_HEIGHT;
    if (s->height_on) {
        // (the boxes compare as float32 values: the kernel then forms the same cells; no corner is a NaN)
        bool same = memcmp(sp.dims, s->height_spec.dims, sizeof sp.dims) == 0 && sp.cameras == s->height_spec.cameras && sp.ids == s->height_spec.ids &&
                    sp.features == s->height_spec.features && sp.source == s->height_spec.source;
        for (int k = 0; k < 3 && same; k++) same = sp.lo[k] == s->height_spec.lo[k] && sp.hi[k] == s->height_spec.hi[k];
        if (same) return LCR_OK;
        char was[320], asked[320];
        return fail(LCR_ERR_INVALID, "a heightmap (%s) is enabled already and fixed for the life of the handle: asked for %s", heightmap_spec_text(was, s->height_spec), heightmap_spec_text(asked, sp));
    }
    LcrHeightmap A{};
    ObsSource src[3];
    A.slots = sources(s, sp.cameras, src);
    for (int i = 0; i < A.slots; i++) { A.cam[i] = src[i].cam; A.seg[i] = src[i].seg; A.depth[i] = src[i].depth; A.rgb[i] = src[i].rgb; }
    const size_t N = (size_t)s->dev.n, M = (size_t)sp.dims[0] * sp.dims[1], Cn = (sp.features & LCR_HEIGHTMAP_RGB) ? 4 : 1;
    // guard, map, guard (include/lcr.h: LCR_WRIST_GUARD), then source, count, filled and the camera poses
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    const size_t o_map = C.take(N * Cn * M * sizeof(float));
    C.skip(LCR_WRIST_GUARD);
    const size_t guarded = C.off;
    const size_t o_src = C.take(sp.source ? N * M * sizeof(int) : 0);
    const size_t o_cnt = C.take(N * sizeof(int));
    const size_t o_fil = C.take(N * sizeof(int));
    const size_t o_pose = C.take((size_t)A.slots * 13 * N * sizeof(float));
    A.n = s->dev.n; A.W = s->dev.img_w; A.H = s->dev.img_h;
    A.ids = sp.ids;
    for (int k = 0; k < 3; k++) A.lo[k] = sp.lo[k];
    A.hi_z = sp.hi[2];
    for (int k = 0; k < 2; k++) {
        A.inv[k] = (float)((double)sp.dims[k] / ((double)sp.hi[k] - (double)sp.lo[k]));   // the header's inv_k: formed once, here, and reported
        A.D[k] = sp.dims[k];
    }
    A.channels = (int)Cn;
    const char *rounds = getenv("LCR_HEIGHTMAP_ROUNDS");
    A.rounds = rounds && !strcmp(rounds, "1") ? 1 : rounds && !strcmp(rounds, "4") ? 4 : 0;
    A.mount = s->wrist.mount;
    void *mem = nullptr;
    const int rc = bring_up(s, C, guarded, "the heightmap", &mem,
        [&](char *base) {
            A.out = (float *)(base + o_map);
            A.source = sp.source ? (int *)(base + o_src) : nullptr;
            A.count = (int *)(base + o_cnt);
            A.filled = (int *)(base + o_fil);
            A.pose = (float *)(base + o_pose);
            s->height = A;
            return launch_heightmap(s, s->dev, s->stream, nullptr);
        },
        [s] { s->height = LcrHeightmap{}; });
    if (rc == LCR_ERR_UNSUPPORTED)
        return fail(LCR_ERR_UNSUPPORTED, "the heightmap kernel is not built for %d cameras at %d x %d with cells of %.9g x %.9g per metre", A.slots, A.W, A.H, (double)A.inv[0], (double)A.inv[1]);
    if (rc) return rc;
    s->height_mem = mem;
    s->height_spec = sp;
    s->height_bytes_per_env = Cn * M * sizeof(float);
    s->height_on = true;
    return LCR_OK;
}

int lcr_get_heightmap(lcr_sim *s, lcr_heightmap_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the map is made behind the frames, on the second stream after a step: the handle's stream waits for it here)
    memset(out, 0, sizeof *out);
    if (!s->height_on) return LCR_OK;
    out->enabled = 1;
    out->spec = s->height_spec;
    for (int k = 0; k < 2; k++) out->inv_cell[k] = s->height.inv[k];
    out->channels = s->height.channels;
    out->slots = s->height.slots;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    out->heightmap = s->height.out;
    out->source = s->height.source;
    out->count = s->height.count;
    out->filled = s->height.filled;
    out->camera_pose = s->height.pose;
    out->bytes_per_env = (uint64_t)s->height_bytes_per_env;
    return LCR_OK;
}

// ---- the object boxes ----

int lcr_object_boxes_check(const lcr_object_boxes_spec *spec) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    if (spec->cameras == 0 || (spec->cameras & ~(uint32_t)(LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | LCR_STACK_CAM_WRIST)))
        return fail(LCR_ERR_INVALID, "cameras must be a non-empty mask of 1 (front), 2 (top) and 4 (wrist), got %u", spec->cameras);
    if (spec->n_objects < 1 || spec->n_objects > LCR_BOXES_MAX_OBJECTS) return fail(LCR_ERR_INVALID, "n_objects must be in 1 .. %d, got %d", LCR_BOXES_MAX_OBJECTS, spec->n_objects);
    for (int o = 0; o < spec->n_objects; o++) {
        const uint32_t m = spec->objects[o];
        if (m == 0) return fail(LCR_ERR_INVALID, "objects[%d] is empty: an object is a mask over the surface ids 1 .. 10 (bits 1 .. 10) and the marker (0x80000000)", o);
        if (m & 1u) return fail(LCR_ERR_INVALID, "objects[%d] selects bit 0, the sky, which is no object (got 0x%x)", o, m);
        if (m & ~(uint32_t)(0x7FEu | LCR_BOXES_MARKER))
            return fail(LCR_ERR_INVALID, "objects[%d] selects bits 11 .. 30, which are no surface ids: a mask over bits 1 .. 10 and the marker (0x80000000), got 0x%x", o, m);
    }
    if (spec->depth != 0 && spec->depth != 1) return fail(LCR_ERR_INVALID, "depth must be 0 or 1, got %d", spec->depth);
    return LCR_OK;
}

// "cameras, n objects (masks), depth" into buf: how the refusal names a spec
static const char *boxes_spec_text(char (&buf)[320], const lcr_object_boxes_spec &v) {
    int at = snprintf(buf, sizeof buf, "cameras %u, %d objects (", v.cameras, v.n_objects);
    for (int o = 0; o < v.n_objects && at < (int)sizeof buf; o++) at += snprintf(buf + at, sizeof buf - at, o ? " 0x%x" : "0x%x", v.objects[o]);
    if (at < (int)sizeof buf) snprintf(buf + at, sizeof buf - at, "), depth %d", v.depth);
    return buf;
}

int lcr_enable_object_boxes(lcr_sim *s, const lcr_object_boxes_spec *spec) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (int rc = lcr_object_boxes_check(spec)) return rc;
    SIMCHK(s);
    if (!s->has_images) return fail(LCR_ERR_INVALID, "sim has no image observations (observation_mode state): there are no frames to find objects in");
    if (!(s->planes & LCR_PLANE_SEGMENTATION))
        return fail(LCR_ERR_INVALID, "the object boxes are made of the segmentation plane (lcr_enable_image_planes with the segmentation bit, before the boxes): the segmentation plane is missing");
    if (spec->depth && !(s->planes & LCR_PLANE_DEPTH))
        return fail(LCR_ERR_INVALID, "depth = 1 keeps the nearest depth of every record, but the depth plane is missing (lcr_enable_image_planes with planes = 3, before the boxes)");
    if ((spec->cameras & LCR_STACK_CAM_WRIST) && !s->wrist_on) return fail(LCR_ERR_INVALID, "cameras selects the wrist camera (4), but the sim has none (lcr_enable_wrist_camera, before the planes and the boxes)");
    lcr_object_boxes_spec sp{};
    sp.cameras = spec->cameras; sp.n_objects = spec->n_objects; sp.depth = spec->depth;
    for (int o = 0; o < sp.n_objects; o++) sp.objects[o] = spec->objects[o];
    if (s->boxes_on) {
        if (memcmp(&sp, &s->boxes_spec, sizeof sp) == 0) return LCR_OK;
        char was[320], asked[320];
        return fail(LCR_ERR_INVALID, "object boxes (%s) are enabled already and fixed for the life of the handle: asked for %s", boxes_spec_text(was, s->boxes_spec), boxes_spec_text(asked, sp));
    }
    LcrBoxes A{};
    ObsSource src[3];
    A.slots = sources(s, sp.cameras, src);
    for (int i = 0; i < A.slots; i++) { A.seg[i] = src[i].seg; A.depth[i] = sp.depth ? (const unsigned *)src[i].depth : nullptr; }
    A.n = s->dev.n; A.W = s->dev.img_w; A.H = s->dev.img_h;
    A.n_objects = sp.n_objects;
    for (int o = 0; o < sp.n_objects; o++) A.masks[o] = sp.objects[o];
    // guard, records, guard (include/lcr.h: LCR_WRIST_GUARD)
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    const size_t o_out = C.take((size_t)A.n * A.slots * sp.n_objects * 8 * sizeof(int32_t));
    C.skip(LCR_WRIST_GUARD);
    void *mem = nullptr;   // (all of it guard-filled; nothing is put on the handle before the launch, so there is nothing to take back)
    const int rc = bring_up(s, C, C.off, "the object boxes", &mem,
        [&](char *base) { A.out = (int *)(base + o_out); return lcr_launch_object_boxes(A, s->stream); }, [] {});
    if (rc == LCR_ERR_UNSUPPORTED) return fail(LCR_ERR_UNSUPPORTED, "the object-boxes kernel is not built for %d cameras at %d x %d with %d objects", A.slots, A.W, A.H, A.n_objects);
    if (rc) return rc;
    s->boxes = A;
    s->boxes_mem = mem;
    s->boxes_spec = sp;
    s->boxes_on = true;
    return LCR_OK;
}

int lcr_get_object_boxes(lcr_sim *s, lcr_object_boxes_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the records are made behind the frames, on the second stream after a step: the handle's stream waits for them here)
    memset(out, 0, sizeof *out);
    if (!s->boxes_on) return LCR_OK;
    out->enabled = 1;
    out->spec = s->boxes_spec;
    out->slots = s->boxes.slots;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    out->boxes = s->boxes.out;
    out->bytes_per_env = (uint64_t)s->boxes.slots * s->boxes.n_objects * 8 * sizeof(int32_t);
    return LCR_OK;
}

// ---- the surface normals ----

int lcr_normals_check(const lcr_normals_spec *spec) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    if (spec->cameras & ~(uint32_t)(LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | LCR_STACK_CAM_WRIST))
        return fail(LCR_ERR_INVALID, "cameras must be 0 (every camera the handle has) or a mask of 1 (front), 2 (top) and 4 (wrist), got %u", spec->cameras);
    if (spec->frame != LCR_NORMALS_WORLD && spec->frame != LCR_NORMALS_CAMERA) return fail(LCR_ERR_INVALID, "frame must be 0 (world) or 1 (camera), got %d", spec->frame);
    return LCR_OK;
}

int lcr_enable_normals(lcr_sim *s, const lcr_normals_spec *spec) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (int rc = lcr_normals_check(spec)) return rc;
    SIMCHK(s);
    lcr_normals_spec sp = *spec;
    if (int rc = planes_ready(s, &sp.cameras, "to give normals to", "the surface normals need", "the normals")) return rc;
    if (s->normals_on) {
        if (sp.cameras == s->normals_spec.cameras && sp.frame == s->normals_spec.frame) return LCR_OK;
        return fail(LCR_ERR_INVALID, "surface normals (cameras %u, frame %d) are enabled already and fixed for the life of the handle: asked for cameras %u, frame %d",
                    s->normals_spec.cameras, s->normals_spec.frame, sp.cameras, sp.frame);
    }
    LcrNormals A{};
    ObsSource src[3];
    A.slots = sources(s, sp.cameras, src);
    for (int i = 0; i < A.slots; i++) { A.cam[i] = src[i].cam; A.seg[i] = src[i].seg; A.depth[i] = src[i].depth; }
    const size_t N = (size_t)s->dev.n, plane = N * s->dev.img_w * s->dev.img_h * 4;
    // guard, then per slot the plane and a guard (include/lcr.h: LCR_WRIST_GUARD), then the boxes and the camera poses
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    size_t o_plane[3] = {0, 0, 0};
    for (int i = 0; i < A.slots; i++) { o_plane[i] = C.take(plane); C.skip(LCR_WRIST_GUARD); }
    const size_t guarded = C.off;
    const size_t o_boxes = C.take((size_t)LCR_NORMALS_BOXES * LCR_NORMALS_BOX_FLOATS * N * sizeof(float));
    const size_t o_pose = C.take((size_t)A.slots * 13 * N * sizeof(float));
    A.n = s->dev.n; A.W = s->dev.img_w; A.H = s->dev.img_h;
    A.frame = sp.frame;
    A.ncube = s->dev.task == 4 ? 2 : 1;
    A.mount = s->wrist.mount;
    void *mem = nullptr;
    const int rc = bring_up(s, C, guarded, "the surface normals", &mem,
        [&](char *base) {
            for (int i = 0; i < A.slots; i++) A.out[i] = (unsigned *)(base + o_plane[i]);
            A.boxes = (float *)(base + o_boxes);
            A.pose = (float *)(base + o_pose);
            s->normals = A;
            return launch_normals(s, s->dev, s->stream, nullptr);
        },
        [s] { s->normals = LcrNormals{}; });
    if (rc == LCR_ERR_UNSUPPORTED) return fail(LCR_ERR_UNSUPPORTED, "the normals kernel is not built for %d cameras at %d x %d", A.slots, A.W, A.H);
    if (rc) return rc;
    s->normals_mem = mem;
    s->normals_spec = sp;
    s->normals_on = true;
    return LCR_OK;
}

int lcr_get_normals(lcr_sim *s, lcr_normals_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the planes are made behind the frames, on the second stream after a step: the handle's stream waits for them here)
    memset(out, 0, sizeof *out);
    if (!s->normals_on) return LCR_OK;
    out->enabled = 1;
    out->spec = s->normals_spec;
    out->slots = s->normals.slots;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    for (int i = 0; i < s->normals.slots; i++) {
        const int8_t *p = (const int8_t *)s->normals.out[i];
        if (s->normals.cam[i] == LCR_CLOUD_CAM_FRONT) out->normals_front = p;
        else if (s->normals.cam[i] == LCR_CLOUD_CAM_TOP) out->normals_top = p;
        else out->normals_wrist = p;
    }
    out->boxes = s->normals.boxes;
    out->camera_pose = s->normals.pose;
    out->bytes_per_env = (uint64_t)s->normals.slots * s->dev.img_w * s->dev.img_h * 4;
    return LCR_OK;
}

// ---- the motion vectors ----

int lcr_motion_check(const lcr_motion_spec *spec) {
    if (!spec) return fail(LCR_ERR_INVALID, "spec is NULL");
    if (spec->cameras & ~(uint32_t)(LCR_STACK_CAM_FRONT | LCR_STACK_CAM_TOP | LCR_STACK_CAM_WRIST))
        return fail(LCR_ERR_INVALID, "cameras must be 0 (every camera the handle has) or a mask of 1 (front), 2 (top) and 4 (wrist), got %u", spec->cameras);
    return LCR_OK;
}

int lcr_enable_motion_vectors(lcr_sim *s, const lcr_motion_spec *spec) {
    // the arguments first, the handle afterwards (what can be refused without a device is)
    if (int rc = lcr_motion_check(spec)) return rc;
    SIMCHK(s);
    lcr_motion_spec sp = *spec;
    if (int rc = planes_ready(s, &sp.cameras, "to give motion vectors to", "the motion vectors need", "the motion vectors")) return rc;
    if (s->flow_on) {
        if (sp.cameras == s->flow_spec.cameras) return LCR_OK;
        return fail(LCR_ERR_INVALID, "motion vectors (cameras %u) are enabled already and fixed for the life of the handle: asked for cameras %u", s->flow_spec.cameras, sp.cameras);
    }
    LcrFlow A{};
    ObsSource src[3];
    A.slots = sources(s, sp.cameras, src);
    for (int i = 0; i < A.slots; i++) { A.cam[i] = src[i].cam; A.seg[i] = src[i].seg; A.depth[i] = src[i].depth; }
    const size_t N = (size_t)s->dev.n, plane = N * s->dev.img_w * s->dev.img_h * 4;
    // guard, then per slot the plane and a guard (include/lcr.h: LCR_WRIST_GUARD), then the boxes and the camera poses (now, before), valid and the snapshots of did_reset
    Carver C;
    C.skip(LCR_WRIST_GUARD);
    size_t o_plane[3] = {0, 0, 0};
    for (int i = 0; i < A.slots; i++) { o_plane[i] = C.take(plane); C.skip(LCR_WRIST_GUARD); }
    const size_t guarded = C.off;
    const size_t o_boxes = C.take(2 * (size_t)LCR_FLOW_BOXES * LCR_FLOW_BOX_FLOATS * N * sizeof(float));
    const size_t o_pose = C.take(2 * (size_t)A.slots * 13 * N * sizeof(float));
    const size_t o_valid = C.take(N);
    const size_t o_snap[2] = {C.take(N), C.take(N)};
    A.n = s->dev.n; A.W = s->dev.img_w; A.H = s->dev.img_h;
    A.ncube = s->dev.task == 4 ? 2 : 1;
    A.mount = s->wrist.mount;
    void *mem = nullptr;
    const int rc = bring_up(s, C, guarded, "the motion vectors", &mem,
        [&](char *base) {
            for (int i = 0; i < A.slots; i++) A.out[i] = (unsigned *)(base + o_plane[i]);
            A.boxes = (float *)(base + o_boxes);
            A.pose = (float *)(base + o_pose);
            A.valid = (unsigned char *)(base + o_valid);
            s->flow = A;
            return launch_flow(s, s->dev, s->stream, nullptr, nullptr, false);   // a restart: zero planes, valid 0, "before" a copy of "now"
        },
        [s] { s->flow = LcrFlow{}; });
    if (rc == LCR_ERR_UNSUPPORTED) return fail(LCR_ERR_UNSUPPORTED, "the motion-vector kernel is not built for %d cameras at %d x %d", A.slots, A.W, A.H);
    if (rc) return rc;
    for (int p = 0; p < 2; p++) s->flow_reset[p] = (unsigned char *)mem + o_snap[p];
    s->flow_mem = mem;
    s->flow_spec = sp;
    s->flow_on = true;
    return LCR_OK;
}

int lcr_get_motion_vectors(lcr_sim *s, lcr_motion_view *out) {
    if (!s || !out) return fail(LCR_ERR_INVALID, "NULL argument");
    SIMCHK(s);   // (the planes are made behind the frames, on the second stream after a step: the handle's stream waits for them here)
    memset(out, 0, sizeof *out);
    if (!s->flow_on) return LCR_OK;
    out->enabled = 1;
    out->spec = s->flow_spec;
    out->slots = s->flow.slots;
    out->image_width = s->dev.img_w;
    out->image_height = s->dev.img_h;
    for (int i = 0; i < s->flow.slots; i++) {
        const uint16_t *p = (const uint16_t *)s->flow.out[i];
        if (s->flow.cam[i] == LCR_CLOUD_CAM_FRONT) out->flow_front = p;
        else if (s->flow.cam[i] == LCR_CLOUD_CAM_TOP) out->flow_top = p;
        else out->flow_wrist = p;
    }
    out->valid = s->flow.valid;
    out->boxes = s->flow.boxes;
    out->camera_pose = s->flow.pose;
    out->bytes_per_env = (uint64_t)s->flow.slots * s->dev.img_w * s->dev.img_h * 4;
    return LCR_OK;
}

int lcr_calibrate_copy(lcr_sim *s, float *dst_dev, size_t n_floats) {
    SIMCHK(s);
    if (!dst_dev) return fail(LCR_ERR_INVALID, "dst is NULL");
    if (n_floats * sizeof(float) > s->arena_bytes) return fail(LCR_ERR_INVALID, "n_floats exceeds the state arena (%zu bytes)", s->arena_bytes);
    LAUNCHCHK("calibration kernel", lcr_launch_calib_copy((const float *)s->arena, dst_dev, n_floats, s->stream));
    return LCR_OK;
}

}  // extern "C"
