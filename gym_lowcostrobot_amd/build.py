"""Build liblcr_hip.so (the C ABI of include/lcr.h) in-tree with hipcc for gfx950.

    python -m gym_lowcostrobot_amd.build [--force]

hipcc cross-compiles without a GPU.  The .so stays next to this file so that it travels with the
source snapshot to the GPU box; it is git-ignored.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "liblcr_hip.so")
SOURCES = ["lcr_capi.hip", "lcr_kernels.hip", "lcr_kernels2.hip", "lcr_render.hip", "lcr_stack.hip", "lcr_cloud.hip", "lcr_cloud_fps.hip", "lcr_cloud_crop.hip", "lcr_voxel.hip", "lcr_heightmap.hip", "lcr_boxes.hip", "lcr_normals.hip", "lcr_flow.hip"]   # (bench.kernel_sha16 and the tools hash / compile these)
HEADERS = ["lcr_device.h", "lcr_arm.h", "lcr_model_gen.h", "lcr_step_common.h", "lcr_newton.h", "lcr_newton_coop.h", "lcr_stack.h", "lcr_cloud.h", "lcr_cloud_dev.h", "lcr_obs_cameras.inc.h", "lcr_cloud_pass1.inc.h", "lcr_cloud_point.inc.h", "lcr_cloud_fps_dev.h", "lcr_cloud_fps_loop.inc.h", "lcr_cloud_crop_pass1.inc.h", "lcr_cloud_crop_point.inc.h", "lcr_voxel.h", "lcr_heightmap.h", "lcr_boxes.h", "lcr_normals.h", "lcr_flow.h", "lcr_opaque_boxes.h", "lcr_wrist_pose.h", os.path.join("..", "..", "include", "lcr.h")]
# -ffast-math: the kernels carry no NaN/inf/signed-zero semantics (the -0.0 sparse reward is built from its bit pattern,
# the fp64 reset sampling uses explicitly rounded __dmul_rn/__dadd_rn); -fno-slp-vectorize: packed-f32 formation by the
# SLP vectoriser costs more moves than it saves here (measured on MI355X: 0.340 ms -> 0.286 ms per 65 536-env step).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-ffast-math", "-fno-slp-vectorize"]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


# (source, object, extra flags): lcr_kernels.hip is compiled seven times, LCR_PART selecting the step-kernel instantiations a unit emits
# (0 one-cube kernels + dispatcher + small kernels, 2 / 3 the two StackTwoCubes variants, 4 / 5 the Newton kernels, 6 / 7 PushCubeLoop's sweep /
# Newton kernels) -- kernels of ~50-100 KB code each: 80 s in one unit, ~30 s as units compiled concurrently
NO_POST_RA = ["-mllvm", "-enable-post-misched=0"]
ITER_ILP = ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]
UNITS = [("lcr_capi.hip", "lcr_capi.o", []),
         # the frame kernels: the default 320 x 240 build (+ background, single-frame and gather kernels) and the builds for run-time sizes, a code object each (lcr_render.hip)
         ("lcr_render.hip", "lcr_render.o", ["-DLCR_RENDER_PART=0"]), ("lcr_render.hip", "lcr_render_sizes.o", ["-DLCR_RENDER_PART=1"]),
         # the frame kernels that also draw the depth / segmentation planes (run-time sizes only), their background and single-frame kernels
         ("lcr_render.hip", "lcr_render_planes.o", ["-DLCR_RENDER_PART=3"]),
         # the kernels that draw with a look (lcr_enable_look): frame kernels with and without planes, the backgrounds of the variants, the single-frame and redraw kernels
         ("lcr_render.hip", "lcr_render_look.o", ["-DLCR_RENDER_PART=4"]),
         # the kernels of the wrist camera (lcr_enable_wrist_camera): the batched frame kernel with and without planes and looks, and its single-frame kernel
         ("lcr_render.hip", "lcr_render_wrist.o", ["-DLCR_RENDER_PART=5"]),
         # the observation stack (lcr_enable_obs_stack): one kernel per element type and depth, each also with the depth channel (lcr_enable_obs_stack_planes), a unit of its own.
         # The project's flags: the depth element its header pins to the bit is kept from -ffast-math inside the source (depth_unit, depth_u8)
         ("lcr_stack.hip", "lcr_stack.o", []),
         # the point cloud (lcr_enable_point_cloud): one kernel with and one without colours, a unit of its own
         ("lcr_cloud.hip", "lcr_cloud.o", []),
         # the cloud by farthest-point sampling (lcr_enable_point_cloud_sampled): a kernel per 2 / 4 / 8 / 16 pool entries a thread, a unit of its own.  The project's flags:
         # the distance its header pins to the bit is kept from -ffast-math inside the source (fps_dist), the rest is the code the strided kernel runs
         ("lcr_cloud_fps.hip", "lcr_cloud_fps.o", []),
         # the cloud inside a crop box (lcr_enable_point_cloud_cropped): a strided kernel with and one without colours and four farthest-point kernels, a unit of its own.
         # The project's flags: the point its header pins to the bit is kept from -ffast-math inside the source (pinned_point, lcr_cloud_dev.h)
         ("lcr_cloud_crop.hip", "lcr_cloud_crop.o", []),
         # the voxel grid (lcr_enable_voxel_grid): a kernel per element type, with and without colours, each also in a build with 128 KiB of LDS; a unit of its own.  The
         # project's flags: the point and the voxel its header pins to the bit are kept from -ffast-math inside the source (pinned_point, cell_axis: lcr_cloud_dev.h)
         ("lcr_voxel.hip", "lcr_voxel.o", []),
         # the heightmap (lcr_enable_heightmap): a kernel with and one without colours, each with one and with four rounds of the scan in flight; a unit of its own.  The
         # project's flags: the point, the cell and the height its header pins to the bit are kept from -ffast-math inside the source (pinned_point, cell_axis: lcr_cloud_dev.h; height_word)
         ("lcr_heightmap.hip", "lcr_heightmap.o", []),
         # the object boxes (lcr_enable_object_boxes): one kernel, integer arithmetic throughout; a unit of its own
         ("lcr_boxes.hip", "lcr_boxes.o", []),
         # the surface normals (lcr_enable_normals): one kernel; a unit of its own.  The project's flags: the point, the box coordinates and the quantisation
         # its header pins to the bit are kept from -ffast-math inside the source (pinned_point, lcr_cloud_dev.h; pinned_dot, quantise)
         ("lcr_normals.hip", "lcr_normals.o", []),
         # the motion vectors (lcr_enable_motion_vectors): one kernel; a unit of its own, and the one unit NOT built with -ffast-math.  Its header pins gx = a / den as one
         # correctly rounded float32 division, and under -ffast-math every spelling of it (/, __fdiv_rn, #pragma clang fp reciprocal(off), float_control) compiles to
         # v_rcp_f32 and a multiply on gfx950; with the two flags appended it is the IEEE sequence v_div_scale / v_div_fmas / v_div_fixup, and nothing is contracted
         ("lcr_flow.hip", "lcr_flow.o", ["-fno-fast-math", "-ffp-contract=off"]),
         ("lcr_kernels.hip", "lcr_kernels.o", ["-DLCR_PART=0"]), ("lcr_kernels.hip", "lcr_kernels_loop.o", ["-DLCR_PART=6"]),
         ("lcr_kernels.hip", "lcr_kernels_loop_newton.o", ["-DLCR_PART=7"] + ITER_ILP),   # (PushCubeLoop's Newton kernels: 6.60 -> 5.98 ms with it, its sweep kernels 0.652 -> 0.730: two units)
         ("lcr_kernels.hip", "lcr_kernels_stack.o", ["-DLCR_PART=2"]), ("lcr_kernels.hip", "lcr_kernels_stack_big.o", ["-DLCR_PART=3"]),
         # the Newton kernels of the faithful preset: one cube / StackTwoCubes (eight cube<->cube slots).  Iterative-ILP scheduling, measured in round 6 against the default
         # (same box, tools/quick_times.py): ReachCube 65 536 envs 2.209 -> 2.082 ms, PushCube 3.499 -> 3.312, Stack 32 768 envs 7.06 -> 6.88, PushCubeLoop 6.60 -> 5.98;
         # no post-RA scheduler 2.362 (worse), both 2.230, max-ilp 2.179, max-memory-clause 2.188
         ("lcr_kernels.hip", "lcr_kernels_newton.o", ["-DLCR_PART=4"] + ITER_ILP),
         ("lcr_kernels.hip", "lcr_kernels_newton_stack.o", ["-DLCR_PART=5"] + ITER_ILP),
         # the two-cooperating-waves family (lcr_kernels2.hip): 10 / 14 one cube built for one / two waves per SIMD, 12 StackTwoCubes, 13 StackTwoCubes with the eight-point
         # manifold.  Instruction-scheduling flags per unit, each measured on the MI355X against the default (tools/quick_times.py; results are bit-identical, the flags only
         # reorder instructions): no post-RA scheduler for the 256-register build (Reach 65 536 envs 0.2578 -> 0.2554 ms, Push 0.3128 -> 0.3064, PickPlace-ee 0.3106 -> 0.3068);
         # no post-RA scheduler + the iterative-ILP strategy for the one-wave-per-SIMD build (PickPlace-ee 32 768 envs 0.2292 -> 0.2180); iterative-ILP for Stack (0.4307 -> 0.4202).
         # The one-wave kernels lose with each of them (Stack 65 536 envs 0.779 -> 0.90 / 1.16): default scheduling there.
         ("lcr_kernels2.hip", "lcr_kernels2.o", ["-DLCR_PART=10"] + NO_POST_RA + ITER_ILP), ("lcr_kernels2.hip", "lcr_kernels2_occ2.o", ["-DLCR_PART=14"] + NO_POST_RA),
         ("lcr_kernels2.hip", "lcr_kernels2_stack.o", ["-DLCR_PART=12"] + ITER_ILP), ("lcr_kernels2.hip", "lcr_kernels2_stack_cc8.o", ["-DLCR_PART=13"])]


def build(force=False, verbose=False):
    from concurrent.futures import ThreadPoolExecutor

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    deps = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]   # (the per-unit flags live in this file)
    # a tree that carries the library but not the objects (a source snapshot shipped with its .so) is current when the .so is newer than everything it is made of
    if not force and os.path.exists(LIB) and not _newer(LIB, [os.path.join(CSRC, src) for src in SOURCES] + deps):
        return LIB
    objs, jobs = [], []
    for src, obj, extra in UNITS:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, obj)
        if force or _newer(o, [s] + deps):
            jobs.append([hipcc] + FLAGS + extra + ["-c", s, "-o", o])
        objs.append(o)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(run, jobs))   # (re-raises the first failure)
    if force or _newer(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
