"""ctypes binding of the C ABI declared in include/lcr.h (liblcr_hip.so).

There is deliberately NO fallback: if the HIP library is missing or no MI355X is visible, importing the
library / creating a simulator raises -- the product path never routes through a CPU implementation.
"""
import ctypes
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LCR_LIB_PATH") or os.path.join(_HERE, "liblcr_hip.so")  # override: A/B builds of the same ABI

ABI_VERSION = 7
NWARM = 124   # LCR_NWARM: floats per env of carried constraint forces (layout: include/lcr.h)
TASKS = {"reach": 0, "lift": 1, "push": 2, "pick_place": 3, "stack": 4, "push_loop": 5}
ACTION_MODES = {"joint": 0, "ee": 1}
OBS_MODES = {"image": 0, "state": 1, "both": 2}
REWARD_TYPES = {"sparse": 0, "dense": 1}
STEP_KERNELS = {"auto": 0, "single": 1, "coop": 2}   # lcr_config.step_kernel
SOLVERS = {"pgs": 0, "newton": 1}                     # lcr_config.solver
PRESETS = {"faithful": 0, "fast": 1}                  # lcr_config_preset
COOP_SHARE = {None: 0, "owner": 1, "shared": 2, "handoff": 3, "ahead": 4, "early": 5}   # lcr_config.coop_share (one-cube Newton kernel; bit-identical results; None: "early")
PROFILE_MODES = {None: None, "wave_cycles": 2, "phase_cycles": 3}   # lcr_config.diagnostics values 2, 3 (per-wave cycle read-back; see include/lcr.h)
COMPAT_ZERO_QVEL_ON_RESET = 1
COMPAT_COLD_SOLVE_EACH_STEP = 2   # contact solver starts every control step from zero forces (default: forces carried across steps)
IMG_H, IMG_W = 240, 320   # LCR_IMG_H / LCR_IMG_W: the default size of the image observations (lcr_config.image_width = image_height = 0)

PLANE_DEPTH, PLANE_SEGMENTATION = 1, 2   # LCR_PLANE_*: bits of lcr_enable_image_planes
IMAGE_PLANES = {"depth": PLANE_DEPTH, "segmentation": PLANE_SEGMENTATION}

LOOK_MAX_VARIANTS = 64   # LCR_LOOK_MAX_VARIANTS
WRIST_GUARD, WRIST_GUARD_BYTE = 4096, 0xA5   # LCR_WRIST_GUARD, LCR_WRIST_GUARD_BYTE: the guard regions around the wrist camera's buffers
# the observation stack (lcr_enable_obs_stack): LCR_STACK_CAM_* bits in channel order, lcr_obs_stack_dtype, lcr_obs_stack_fill, LCR_STACK_MAX_FRAMES
STACK_CAMERAS = {"front": 1, "top": 2, "wrist": 4}
STACK_DTYPES = {"uint8": 0, "float16": 1, "float32": 2}
STACK_FILLS = {"repeat": 0, "zero": 1}
STACK_MAX_FRAMES = 8
# the point cloud (lcr_enable_point_cloud): its cameras are STACK_CAMERAS bits; the surface ids of the segmentation plane by name ("arm": base_link, link_1 .. link_6)
CLOUD_IDS = {"floor": 1 << 1, "arm": 0x7F << 2, "cube": 1 << 9, "cube2": 1 << 10}
CLOUD_DEFAULT_IDS = 0x7FC   # LCR_CLOUD_DEFAULT_IDS: arm, cube, cube2
CLOUD_MIN_POINTS, CLOUD_MAX_POINTS = 64, 8192
CLOUD_SAMPLINGS = {"stride": 0, "fps": 1}   # LCR_CLOUD_SAMPLE_*: the strided selection, or farthest-point sampling from a strided pool (lcr_enable_point_cloud_sampled)
CLOUD_MAX_POOL = 4096                       # LCR_CLOUD_MAX_POOL
# the voxel grid (lcr_enable_voxel_grid): LCR_VOXEL_* feature bits, LCR_VOXEL_MAX_DIM, LCR_VOXEL_MAX_CELLS; its cameras, ids and dtypes are the cloud's and the stack's
VOXEL_FEATURES = {"occupancy": 1, "rgb": 2}
VOXEL_MAX_DIM, VOXEL_MAX_CELLS = 64, 32768
# the heightmap (lcr_enable_heightmap): LCR_HEIGHTMAP_* feature bits, LCR_HEIGHTMAP_MAX_DIM, LCR_HEIGHTMAP_MAX_CELLS; its cameras and ids are the cloud's
HEIGHTMAP_FEATURES = {"height": 1, "rgb": 2}
HEIGHTMAP_MAX_DIM, HEIGHTMAP_MAX_CELLS = 256, 16384
# the object boxes (lcr_enable_object_boxes): LCR_BOXES_MAX_OBJECTS, LCR_BOXES_MARKER, the names of an object's parts as masks over the surface ids, the eight fields of a record
BOXES_MAX_OBJECTS, BOXES_MARKER = 16, 0x80000000
BOXES_OBJECTS = {"floor": 1 << 1, "arm": 0x7F << 2, "cube": 1 << 9, "cube2": 1 << 10, "marker": BOXES_MARKER, "base_link": 1 << 2,
                 **{f"link_{i}": 1 << (2 + i) for i in range(1, 7)}}
BOXES_DEFAULT_OBJECTS = ("arm", "cube", "cube2", "marker")   # the same for every task: an object a task does not have gives empty records, the shape does not depend on the task
BOXES_FIELDS = ("x0", "y0", "x1", "y1", "count", "sum_x", "sum_y", "nearest")
# the surface normals (lcr_enable_normals): LCR_NORMALS_WORLD / LCR_NORMALS_CAMERA, the number of opaque boxes and the floats of one (centre, X, Y, Z, half-extents)
NORMALS_FRAMES = {"world": 0, "camera": 1}
NORMALS_BOXES, NORMALS_BOX_FLOATS = 9, 15
LOOK_TASK_RGB = (0.5, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 1.0)   # the task's colours: cube, second cube (StackTwoCubes), target marker (PushCube / PickPlaceCube)

LCR_OK, LCR_ERR_INVALID, LCR_ERR_NO_DEVICE, LCR_ERR_HIP, LCR_ERR_OOM, LCR_ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5

# every symbol include/lcr.h declares (tests check the .so exports exactly these)
SYMBOLS = [
    "lcr_abi_version", "lcr_last_error", "lcr_config_default", "lcr_config_preset", "lcr_action_dim", "lcr_nq", "lcr_nv",
    "lcr_create", "lcr_destroy", "lcr_set_stream", "lcr_sync", "lcr_reset", "lcr_step", "lcr_step_host",
    "lcr_get_obs", "lcr_get_outputs", "lcr_fetch_host", "lcr_get_state", "lcr_set_state", "lcr_malloc", "lcr_free",
    "lcr_memcpy_h2d", "lcr_memcpy_d2h", "lcr_timer_begin", "lcr_timer_end", "lcr_fill_random_actions",
    "lcr_calibrate_copy", "lcr_render", "lcr_render_state", "lcr_render_terminal", "lcr_step_kernel_family", "lcr_get_redo_flags",
    "lcr_enable_image_planes", "lcr_get_image_planes", "lcr_render_planes", "lcr_render_state_planes", "lcr_render_terminal_planes",
    "lcr_look_variant_default", "lcr_enable_look", "lcr_set_look", "lcr_get_look",
    "lcr_wrist_camera_default", "lcr_wrist_camera_check", "lcr_enable_wrist_camera", "lcr_get_wrist_camera", "lcr_render_terminal_wrist",
    "lcr_obs_stack_check", "lcr_enable_obs_stack", "lcr_get_obs_stack",
    "lcr_point_cloud_check", "lcr_enable_point_cloud", "lcr_get_point_cloud",
    "lcr_point_cloud_sampling_check", "lcr_enable_point_cloud_sampled", "lcr_get_point_cloud_sampling",
    "lcr_point_cloud_crop_check", "lcr_enable_point_cloud_cropped", "lcr_get_point_cloud_crop",
    "lcr_enable_obs_stack_terminal", "lcr_get_obs_stack_terminal", "lcr_obs_stack_terminal", "lcr_point_cloud_terminal",
    "lcr_voxel_grid_check", "lcr_enable_voxel_grid", "lcr_get_voxel_grid",
    "lcr_heightmap_check", "lcr_enable_heightmap", "lcr_get_heightmap",
    "lcr_object_boxes_check", "lcr_enable_object_boxes", "lcr_get_object_boxes",
    "lcr_normals_check", "lcr_enable_normals", "lcr_get_normals",
    "lcr_motion_check", "lcr_enable_motion_vectors", "lcr_get_motion_vectors",
    "lcr_enable_obs_stack_planes", "lcr_get_obs_stack_planes",
]


class LcrConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("task", ctypes.c_int32),
        ("n_envs", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("env_id_offset", ctypes.c_int64),
        ("action_mode", ctypes.c_int32),
        ("obs_mode", ctypes.c_int32),
        ("reward_type", ctypes.c_int32),
        ("block_gripper", ctypes.c_int32),
        ("distance_threshold", ctypes.c_double),
        ("cube_xy_range", ctypes.c_double),
        ("target_xy_range", ctypes.c_double),
        ("goal_z_range", ctypes.c_double),
        ("height_threshold", ctypes.c_double),
        ("impratio", ctypes.c_double),
        ("n_substeps", ctypes.c_int32),
        ("max_episode_steps", ctypes.c_int32),
        ("pgs_iters", ctypes.c_int32),
        ("compat", ctypes.c_uint32),
        ("auto_reset", ctypes.c_int32),
        ("arm_collision", ctypes.c_int32),
        ("base_seed", ctypes.c_uint64),
        ("pgs_tol", ctypes.c_double),
        ("diagnostics", ctypes.c_int32),
        ("finger_cube_condim", ctypes.c_int32),
        ("step_kernel", ctypes.c_int32),
        ("cc_points", ctypes.c_int32),
        ("global_envs", ctypes.c_int64),   # ABI v4: envs of the whole job (0 = n_envs); the step_kernel = 0 dispatch looks at it, never at the shard size
        ("solver", ctypes.c_int32),        # ABI v5: SOLVERS
        ("newton_iters", ctypes.c_int32),
        ("ls_iters", ctypes.c_int32),
        ("finger_floor_condim", ctypes.c_int32),
        ("newton_tol", ctypes.c_double),
        ("ls_tol", ctypes.c_double),
        ("coop_share", ctypes.c_int32),    # ABI v6: COOP_SHARE
        ("image_width", ctypes.c_int32),   # ABI v7: size of the image observations, multiples of 4 in [16, 512]; 0, 0 = 320 x 240
        ("image_height", ctypes.c_int32),
    ]


class LcrObsView(ctypes.Structure):
    _fields_ = [
        ("n_envs", ctypes.c_int32),
        ("has_aux", ctypes.c_int32),
        ("arm_qpos", ctypes.c_void_p),
        ("arm_qvel", ctypes.c_void_p),
        ("cube_pos", ctypes.c_void_p),
        ("aux_pos", ctypes.c_void_p),
        ("image_front", ctypes.c_void_p),
        ("image_top", ctypes.c_void_p),
        ("image_width", ctypes.c_int32),   # ABI v7: the size in use (0, 0 without images)
        ("image_height", ctypes.c_int32),
    ]


class LcrPlanesView(ctypes.Structure):
    _fields_ = [
        ("planes", ctypes.c_uint32),       # LCR_PLANE_* bits in use (0: none, every pointer NULL)
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("depth_far", ctypes.c_float),
        ("depth_front", ctypes.c_void_p),  # [N][H][W] float32 metres along the optical axis
        ("depth_top", ctypes.c_void_p),
        ("seg_front", ctypes.c_void_p),    # [N][H][W] uint8 ids
        ("seg_top", ctypes.c_void_p),
    ]


class LookVariant(ctypes.Structure):
    """lcr_look_variant: everything the cached background of the frames depends on (include/lcr.h).  Index 0 = camera_front, 1 = camera_top."""
    _fields_ = [
        ("cam_dpos", (ctypes.c_float * 3) * 2),    # metres, world frame, added to the scene camera's position
        ("cam_drot", (ctypes.c_float * 3) * 2),    # rotation vector, world frame
        ("fovy_deg", ctypes.c_float * 2),
        ("floor_rgb", (ctypes.c_float * 3) * 2),   # checker cells: odd, even
        ("sky_rgb", ctypes.c_float * 3),
        ("sky_slope", ctypes.c_float * 3),
        ("ambient", ctypes.c_float),
        ("diffuse", ctypes.c_float),
        ("arm_rgb", ctypes.c_float * 3),
        ("finger_rgb", ctypes.c_float * 3),
    ]

    def as_dict(self):
        import numpy as np

        return {name: (np.array(getattr(self, name), np.float32) if not isinstance(getattr(self, name), float) else float(getattr(self, name))) for name, _ in self._fields_}

    @classmethod
    def from_any(cls, v):
        """a LookVariant, or a dict of some of its fields over the default variant"""
        if isinstance(v, cls):
            return v
        import numpy as np

        out = cls()
        check(load().lcr_look_variant_default(ctypes.byref(out)))
        shapes = {"cam_dpos": (2, 3), "cam_drot": (2, 3), "fovy_deg": (2,), "floor_rgb": (2, 3), "sky_rgb": (3,), "sky_slope": (3,), "arm_rgb": (3,), "finger_rgb": (3,)}
        for name, val in dict(v).items():
            if name in ("ambient", "diffuse"):
                setattr(out, name, float(val))
            elif name in shapes:
                a = np.broadcast_to(np.asarray(val, np.float32), shapes[name])
                fld = getattr(out, name)
                for idx in np.ndindex(*shapes[name]):
                    if len(idx) == 1:
                        fld[idx[0]] = float(a[idx])
                    else:
                        fld[idx[0]][idx[1]] = float(a[idx])
            else:
                raise ValueError(f"unknown look variant field {name!r}")
        return out


class LookSampler(ctypes.Structure):
    """lcr_look_sampler: per-channel uniform boxes of the per-env colours, redrawn at every reset of an env"""
    _fields_ = [("seed", ctypes.c_uint64)] + [(f"{g}_{e}", ctypes.c_float * 3) for g in ("cube", "cube2", "marker") for e in ("lo", "hi")]

    @classmethod
    def from_any(cls, v):
        """a LookSampler, or a dict: seed, and per group cube / cube2 / marker a (lo, hi) pair under its name or `<group>_lo` / `<group>_hi`; a group not named keeps its task colour"""
        if isinstance(v, cls):
            return v
        import numpy as np

        v = dict(v)
        out = cls()
        out.seed = int(v.pop("seed", 0))
        for g, base in (("cube", LOOK_TASK_RGB[0:3]), ("cube2", LOOK_TASK_RGB[3:6]), ("marker", LOOK_TASK_RGB[6:9])):
            lo, hi = v.pop(g, (base, base))
            lo, hi = v.pop(g + "_lo", lo), v.pop(g + "_hi", hi)
            for i in range(3):
                getattr(out, g + "_lo")[i] = float(np.broadcast_to(np.asarray(lo, np.float32), (3,))[i])
                getattr(out, g + "_hi")[i] = float(np.broadcast_to(np.asarray(hi, np.float32), (3,))[i])
        if v:
            raise ValueError(f"unknown look sampler fields {sorted(v)}")
        return out


class WristCamera(ctypes.Structure):
    """lcr_wrist_camera: the mount of the optional third observation camera (include/lcr.h)"""
    _fields_ = [
        ("link", ctypes.c_int32),          # 0 = world frame, 1 .. 6 = body frame of link_1 .. link_6
        ("pos", ctypes.c_float * 3),       # metres in that frame
        ("xyaxes", ctypes.c_float * 6),    # MuJoCo's camera xyaxes in that frame: X then Y
        ("fovy_deg", ctypes.c_float),
    ]

    def as_dict(self):
        return {"link": int(self.link), "pos": tuple(float(x) for x in self.pos), "xyaxes": tuple(float(x) for x in self.xyaxes), "fovy_deg": float(self.fovy_deg)}

    @classmethod
    def from_any(cls, v):
        """a WristCamera, True (the default mount), or a dict of some of link / pos / xyaxes / fovy_deg over the default mount"""
        if isinstance(v, cls):
            return v
        out = cls()
        check(load().lcr_wrist_camera_default(ctypes.byref(out)))
        if v is True:
            return out
        if not isinstance(v, dict):
            raise ValueError(f"wrist_camera must be None, True or a dict of link / pos / xyaxes / fovy_deg, got {v!r}")
        v = dict(v)
        try:
            if "link" in v:
                out.link = int(v.pop("link"))
            if "fovy_deg" in v:
                out.fovy_deg = float(v.pop("fovy_deg"))
            for name, cnt in (("pos", 3), ("xyaxes", 6)):
                if name in v:
                    vals = [float(x) for x in v.pop(name)]
                    if len(vals) != cnt:
                        raise ValueError(f"wrist_camera: {name} takes {cnt} numbers, got {len(vals)}")
                    for i, x in enumerate(vals):
                        getattr(out, name)[i] = x
        except TypeError:
            raise ValueError("wrist_camera: link is an integer, fovy_deg a number, pos three and xyaxes six numbers") from None
        if v:
            raise ValueError(f"unknown wrist camera fields {sorted(v)}")
        return out


class LcrWristView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("camera", WristCamera),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("depth_far", ctypes.c_float),
        ("image_wrist", ctypes.c_void_p),  # [N][H][W][3] uint8
        ("depth_wrist", ctypes.c_void_p),  # [N][H][W] float32 or NULL
        ("seg_wrist", ctypes.c_void_p),    # [N][H][W] uint8 or NULL
    ]


class ObsStackSpec(ctypes.Structure):
    """lcr_obs_stack_spec: depth, cameras, element type and refill rule of the observation stack (include/lcr.h)"""
    _fields_ = [
        ("frames", ctypes.c_int32),      # K, 1 .. 8
        ("cameras", ctypes.c_uint32),    # STACK_CAMERAS bits; 0 = every camera the handle has
        ("dtype", ctypes.c_int32),       # STACK_DTYPES
        ("reset_fill", ctypes.c_int32),  # STACK_FILLS
    ]

    def as_dict(self):
        return {"frames": int(self.frames), "cameras": tuple(n for n, b in STACK_CAMERAS.items() if self.cameras & b),
                "dtype": {v: k for k, v in STACK_DTYPES.items()}[int(self.dtype)], "reset_fill": {v: k for k, v in STACK_FILLS.items()}[int(self.reset_fill)]}

    @classmethod
    def from_any(cls, v):
        """an ObsStackSpec, an int (that many frames of every camera, uint8, repeat), or a dict of some of frames / cameras / dtype / reset_fill"""
        import numpy as np

        if isinstance(v, cls):
            return v
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer, dict)):
            raise ValueError(f"obs_stack must be None, a number of frames or a dict of frames / cameras / dtype / reset_fill, got {v!r}")
        v = {"frames": v} if not isinstance(v, dict) else dict(v)
        out = cls(frames=1)
        frames = v.pop("frames", 1)
        if isinstance(frames, (bool, np.bool_)) or not isinstance(frames, (int, np.integer)) or not 1 <= frames <= STACK_MAX_FRAMES:
            raise ValueError(f"obs_stack: frames must be an integer in 1 .. {STACK_MAX_FRAMES}, got {frames!r}")
        out.frames = int(frames)
        cams = v.pop("cameras", None)
        if cams is not None:
            if isinstance(cams, str) or not all(isinstance(c, str) and c in STACK_CAMERAS for c in cams) or len(cams) == 0:
                raise ValueError(f"obs_stack: cameras must be a non-empty tuple drawn from 'front', 'top' and 'wrist', got {cams!r}")
            out.cameras = sum(STACK_CAMERAS[c] for c in set(cams))
        dtype = v.pop("dtype", "uint8")
        try:
            dtype = dtype if isinstance(dtype, str) else np.dtype(dtype).name
        except TypeError:
            pass
        if dtype not in STACK_DTYPES:
            raise ValueError(f"obs_stack: dtype must be 'uint8', 'float16' or 'float32', got {dtype!r}")
        out.dtype = STACK_DTYPES[dtype]
        fill = v.pop("reset_fill", "repeat")
        if fill not in STACK_FILLS:
            raise ValueError(f"obs_stack: reset_fill must be 'repeat' or 'zero', got {fill!r}")
        out.reset_fill = STACK_FILLS[fill]
        if v:
            raise ValueError(f"unknown obs_stack fields {sorted(v)}")
        return out


def take_terminal(v, what):
    """(what is left of the obs_stack / point_cloud argument `what`, its `terminal` flag): takes `terminal` out of a dict -- a bool, default False: the caller wants the
    stacks / clouds of episodes that end (VecSim.obs_stack_terminal / point_cloud_terminal, and the keys the vector adapters add); anything else has none"""
    import numpy as np

    if not isinstance(v, dict) or "terminal" not in v:
        return v, False
    v = dict(v)
    terminal = v.pop("terminal")
    if not isinstance(terminal, (bool, np.bool_)):
        raise ValueError(f"{what}: terminal must be a bool, got {terminal!r}")
    return v, bool(terminal)


def take_stack_planes(v, image_planes):
    """(what is left of the obs_stack argument, the LCR_PLANE_* mask of its `planes`): takes `planes` out of a dict -- a tuple or list of plane names, default (): the
    planes the stack carries as channels beside the colours (lcr_enable_obs_stack_planes).  Only 'depth' is stacked, and only when `image_planes` has it: the plane is
    not switched on silently"""
    if not isinstance(v, dict) or "planes" not in v:
        return v, 0
    v = dict(v)
    planes = v.pop("planes")
    if not isinstance(planes, (tuple, list)) or not all(isinstance(p, str) for p in planes):
        raise ValueError(f"obs_stack: planes must be a tuple or list of plane names, () or ('depth',), got {planes!r}")
    unknown = sorted(set(planes) - set(IMAGE_PLANES))
    if unknown:
        raise ValueError(f"obs_stack: planes has unknown names {unknown}: () or ('depth',)")
    if "segmentation" in planes:
        raise ValueError("obs_stack: planes: 'segmentation' is unsupported in the stack (its ids are categorical: a cast of them is not policy-ready); () or ('depth',)")
    if "depth" in planes and "depth" not in image_planes:
        raise ValueError(f"obs_stack: planes=('depth',) is made of the depth plane: pass 'depth' in image_planes (got {tuple(image_planes)!r})")
    return v, (PLANE_DEPTH if "depth" in planes else 0)


class LcrObsStackView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("spec", ObsStackSpec),          # cameras resolved to the bits in use
        ("channels", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("data", ctypes.c_void_p),       # [N][K][C][H][W] of the element type
        ("bytes_per_env", ctypes.c_uint64),
    ]


class PointCloudSpec(ctypes.Structure):
    """lcr_point_cloud_spec: points per env, cameras, surface ids and channels of the point cloud (include/lcr.h)"""
    _fields_ = [
        ("points", ctypes.c_int32),      # P, a multiple of 64 in 64 .. 8192
        ("cameras", ctypes.c_uint32),    # STACK_CAMERAS bits; 0 = every camera the handle has
        ("ids", ctypes.c_uint32),        # bit i: surface id i is a candidate (1 .. 10); 0 = CLOUD_DEFAULT_IDS
        ("colors", ctypes.c_int32),      # 0: x y z, 1: x y z r g b
    ]

    def as_dict(self):
        return {"points": int(self.points), "cameras": tuple(n for n, b in STACK_CAMERAS.items() if self.cameras & b),
                "ids": tuple(i for i in range(32) if self.ids >> i & 1), "colors": bool(self.colors)}

    @classmethod
    def from_any(cls, v):
        """a PointCloudSpec, an int (that many points of every camera, arm and cubes, x y z), or a dict of some of points / cameras / ids / colors"""
        import numpy as np

        if isinstance(v, cls):
            return v
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer, dict)):
            raise ValueError(f"point_cloud must be None, a number of points or a dict of points / cameras / ids / colors, got {v!r}")
        v = {"points": v} if not isinstance(v, dict) else dict(v)
        out = cls()
        points = v.pop("points", 1024)
        if isinstance(points, (bool, np.bool_)) or not isinstance(points, (int, np.integer)) or not CLOUD_MIN_POINTS <= points <= CLOUD_MAX_POINTS or points % 64:
            raise ValueError(f"point_cloud: points must be a multiple of 64 in {CLOUD_MIN_POINTS} .. {CLOUD_MAX_POINTS}, got {points!r}")
        out.points = int(points)
        cams = v.pop("cameras", None)
        if cams is not None:
            if isinstance(cams, str) or not all(isinstance(c, str) and c in STACK_CAMERAS for c in cams) or len(cams) == 0:
                raise ValueError(f"point_cloud: cameras must be a non-empty tuple drawn from 'front', 'top' and 'wrist', got {cams!r}")
            out.cameras = sum(STACK_CAMERAS[c] for c in set(cams))
        ids = v.pop("ids", None)
        if ids is not None:
            mask = 0
            ok = not isinstance(ids, str) and hasattr(ids, "__iter__")
            for i in (ids if ok else ()):
                if isinstance(i, str) and i in CLOUD_IDS:
                    mask |= CLOUD_IDS[i]
                elif isinstance(i, (int, np.integer)) and not isinstance(i, (bool, np.bool_)) and 1 <= i <= 10:
                    mask |= 1 << int(i)
                else:
                    ok = False
            if not ok or mask == 0:
                raise ValueError(f"point_cloud: ids must be a non-empty tuple drawn from 'arm', 'cube', 'cube2', 'floor' and the surface ids 1 .. 10, got {ids!r}")
            out.ids = mask
        colors = v.pop("colors", False)
        if not isinstance(colors, (bool, np.bool_)):
            raise ValueError(f"point_cloud: colors must be a bool, got {colors!r}")
        out.colors = int(colors)
        if v:
            raise ValueError(f"unknown point_cloud fields {sorted(v)}")
        return out


class PointCloudSampling(ctypes.Structure):
    """lcr_point_cloud_sampling: how the cloud's points are picked -- the strided rule, or farthest-point sampling (FPS) out of a strided pool (include/lcr.h)"""
    _fields_ = [
        ("mode", ctypes.c_int32),        # CLOUD_SAMPLINGS
        ("pool", ctypes.c_int32),        # Q under "fps": a multiple of 64, points <= pool <= CLOUD_MAX_POOL; 0 under "stride"
    ]

    def as_dict(self):
        return {"mode": {v: k for k, v in CLOUD_SAMPLINGS.items()}.get(int(self.mode), int(self.mode)), "pool": int(self.pool)}

    @classmethod
    def take(cls, v):
        """(what is left of the point_cloud argument, its PointCloudSampling): takes `sampling` and `pool` out of a dict; anything else is a strided cloud"""
        import numpy as np

        out = cls()
        if not isinstance(v, dict) or not ("sampling" in v or "pool" in v):
            return v, out
        v = dict(v)
        sampling, pool = v.pop("sampling", "stride"), v.pop("pool", None)
        if not isinstance(sampling, str) or sampling not in CLOUD_SAMPLINGS:
            raise ValueError(f"point_cloud: sampling must be 'stride' or 'fps', got {sampling!r}")
        out.mode = CLOUD_SAMPLINGS[sampling]
        if sampling == "stride":
            if pool is not None:
                raise ValueError(f"point_cloud: pool goes with sampling='fps' (a strided cloud has no pool), got pool {pool!r}")
            return v, out
        if pool is None:
            raise ValueError("point_cloud: sampling='fps' needs a pool (the candidates the points are picked from: the caller chooses the cost)")
        if isinstance(pool, (bool, np.bool_)) or not isinstance(pool, (int, np.integer)) or not 64 <= pool <= CLOUD_MAX_POOL or pool % 64:
            raise ValueError(f"point_cloud: pool must be a multiple of 64 in 64 .. {CLOUD_MAX_POOL}, got {pool!r}")
        out.pool = int(pool)
        return v, out


class PointCloudCrop(ctypes.Structure):
    """lcr_point_cloud_crop: an axis-aligned box in the world frame; a candidate of the cloud must have its point inside it (include/lcr.h)"""
    _fields_ = [
        ("lo", ctypes.c_float * 3),      # x, y, z of the lower corner; -inf: an open side
        ("hi", ctypes.c_float * 3),      # x, y, z of the upper corner; +inf: an open side
    ]

    def as_dict(self):
        """the float32 values in use, as Python floats"""
        return {"lo": tuple(float(v) for v in self.lo), "hi": tuple(float(v) for v in self.hi)}

    @classmethod
    def take(cls, v):
        """(what is left of the point_cloud argument, its PointCloudCrop or None): takes `crop` out of a dict -- ((x0, y0, z0), (x1, y1, z1)), None inside a triple an open
        side; crop=None, or no crop, is a cloud without a box"""
        import numpy as np

        if not isinstance(v, dict) or "crop" not in v:
            return v, None
        v = dict(v)
        crop = v.pop("crop")
        if crop is None:
            return v, None
        what = "point_cloud: crop must be ((x0, y0, z0), (x1, y1, z1)), the lower and the upper corner of a box in the world frame (None: an open side)"
        try:
            lo, hi = crop
            lo, hi = list(lo), list(hi)
        except (TypeError, ValueError):
            raise ValueError(f"{what}, got {crop!r}") from None
        if isinstance(crop, str) or len(lo) != 3 or len(hi) != 3:
            raise ValueError(f"{what}, got {crop!r}")
        out = cls()
        for name, side, dst, open_side in (("lo", lo, out.lo, -np.inf), ("hi", hi, out.hi, np.inf)):
            for k, x in enumerate(side):
                if x is None:
                    x = open_side
                if isinstance(x, (bool, np.bool_, str)) or not isinstance(x, (int, float, np.integer, np.floating)):
                    raise ValueError(f"{what}; {name}[{k}] is {x!r}")
                x = np.float32(x)   # (the float32 value the kernel compares with)
                if np.isnan(x):
                    raise ValueError(f"point_cloud: crop {name}[{k}] is NaN (None or an infinity is an open side)")
                dst[k] = float(x)
        for k, axis in enumerate("xyz"):
            if out.lo[k] > out.hi[k]:
                raise ValueError(f"point_cloud: crop lo[{k}] > hi[{k}]: the box is empty along {axis} (lo {out.lo[k]!r}, hi {out.hi[k]!r})")
        return v, out


class LcrPointCloudView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("spec", PointCloudSpec),        # cameras and ids resolved to the bits in use
        ("channels", ctypes.c_int32),
        ("slots", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("points", ctypes.c_void_p),       # [N][P][C] float32
        ("count", ctypes.c_void_p),        # [N] int32
        ("source", ctypes.c_void_p),       # [N][P] int32
        ("camera_pose", ctypes.c_void_p),  # [slots][13][N] float32
        ("bytes_per_env", ctypes.c_uint64),
    ]


class VoxelGridSpec(ctypes.Structure):
    """lcr_voxel_grid_spec: box, cells, cameras, surface ids, channels and element type of the voxel grid (include/lcr.h)"""
    _fields_ = [
        ("lo", ctypes.c_float * 3),      # x, y, z of the box's lower corner, world frame; finite
        ("hi", ctypes.c_float * 3),      # x, y, z of the upper corner; finite, lo[k] < hi[k]
        ("dims", ctypes.c_int32 * 3),    # Dx (a multiple of 4), Dy, Dz: each 1 .. VOXEL_MAX_DIM, at most VOXEL_MAX_CELLS voxels
        ("cameras", ctypes.c_uint32),    # STACK_CAMERAS bits; 0 = every camera the handle has
        ("ids", ctypes.c_uint32),        # bit i: surface id i is a candidate (1 .. 10); 0 = CLOUD_DEFAULT_IDS
        ("features", ctypes.c_uint32),   # VOXEL_FEATURES bits; occupancy is implied
        ("dtype", ctypes.c_int32),       # STACK_DTYPES: uint8 or float32
        ("source", ctypes.c_int32),      # 0 | 1: keep the source index of every voxel
    ]

    def as_dict(self):
        """the float32 corners in use as Python floats, cameras / features as names, ids as a tuple, as PointCloudSpec.as_dict has them"""
        return {"lo": tuple(float(v) for v in self.lo), "hi": tuple(float(v) for v in self.hi), "dims": tuple(int(v) for v in self.dims),
                "cameras": tuple(n for n, b in STACK_CAMERAS.items() if self.cameras & b), "ids": tuple(i for i in range(32) if self.ids >> i & 1),
                "features": tuple(n for n, b in VOXEL_FEATURES.items() if self.features & b),
                "dtype": {v: k for k, v in STACK_DTYPES.items()}.get(int(self.dtype), int(self.dtype)), "source": bool(self.source)}

    @classmethod
    def from_any(cls, v):
        """a VoxelGridSpec, or a dict with box=((x0, y0, z0), (x1, y1, z1)) and dims=(Dx, Dy, Dz) -- neither has a default: the caller chooses the memory -- and some of
        cameras / ids / features / dtype / source"""
        import numpy as np

        if isinstance(v, cls):
            return v
        if not isinstance(v, dict):
            raise ValueError(f"voxel_grid must be None or a dict of box / dims / cameras / ids / features / dtype / source, got {v!r}")
        v = dict(v)
        out = cls()
        if "box" not in v or "dims" not in v:
            raise ValueError("voxel_grid needs box=((x0, y0, z0), (x1, y1, z1)) and dims=(Dx, Dy, Dz): neither has a default, the caller chooses the memory")
        box, dims = v.pop("box"), v.pop("dims")
        what = "voxel_grid: box must be ((x0, y0, z0), (x1, y1, z1)), the lower and the upper corner of a box in the world frame, six finite numbers"
        try:
            lo, hi = box
            lo, hi = list(lo), list(hi)
        except (TypeError, ValueError):
            raise ValueError(f"{what}, got {box!r}") from None
        if isinstance(box, str) or len(lo) != 3 or len(hi) != 3:
            raise ValueError(f"{what}, got {box!r}")
        for name, side, dst in (("lo", lo, out.lo), ("hi", hi, out.hi)):
            for k, x in enumerate(side):
                if isinstance(x, (bool, np.bool_, str)) or not isinstance(x, (int, float, np.integer, np.floating)):
                    raise ValueError(f"{what}; {name}[{k}] is {x!r}")
                x = np.float32(x)   # (the float32 value the kernel subtracts)
                if not np.isfinite(x):
                    raise ValueError(f"voxel_grid: box {name}[{k}] is not finite: the box of a voxel grid has no open sides")
                dst[k] = float(x)
        for k, axis in enumerate("xyz"):
            if not out.lo[k] < out.hi[k]:
                raise ValueError(f"voxel_grid: box lo[{k}] >= hi[{k}]: the box is empty along {axis} (lo {out.lo[k]!r}, hi {out.hi[k]!r})")
        try:
            dims = list(dims)
        except TypeError:
            dims = []
        if len(dims) != 3 or any(isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, np.integer)) or not 1 <= d <= VOXEL_MAX_DIM for d in dims):
            raise ValueError(f"voxel_grid: dims must be (Dx, Dy, Dz), each an integer in 1 .. {VOXEL_MAX_DIM}, got {dims!r}")
        if dims[0] % 4:
            raise ValueError(f"voxel_grid: dims[0] (x) must be a multiple of 4, got {dims[0]!r}")
        if dims[0] * dims[1] * dims[2] > VOXEL_MAX_CELLS:
            raise ValueError(f"voxel_grid: dims {tuple(dims)!r} are {dims[0] * dims[1] * dims[2]} voxels: at most {VOXEL_MAX_CELLS}")
        for k in range(3):
            out.dims[k] = int(dims[k])
        cams = v.pop("cameras", None)
        if cams is not None:
            if isinstance(cams, str) or not all(isinstance(c, str) and c in STACK_CAMERAS for c in cams) or len(cams) == 0:
                raise ValueError(f"voxel_grid: cameras must be a non-empty tuple drawn from 'front', 'top' and 'wrist', got {cams!r}")
            out.cameras = sum(STACK_CAMERAS[c] for c in set(cams))
        ids = v.pop("ids", None)
        if ids is not None:
            mask = 0
            ok = not isinstance(ids, str) and hasattr(ids, "__iter__")
            for i in (ids if ok else ()):
                if isinstance(i, str) and i in CLOUD_IDS:
                    mask |= CLOUD_IDS[i]
                elif isinstance(i, (int, np.integer)) and not isinstance(i, (bool, np.bool_)) and 1 <= i <= 10:
                    mask |= 1 << int(i)
                else:
                    ok = False
            if not ok or mask == 0:
                raise ValueError(f"voxel_grid: ids must be a non-empty tuple drawn from 'arm', 'cube', 'cube2', 'floor' and the surface ids 1 .. 10, got {ids!r}")
            out.ids = mask
        feats = v.pop("features", ("occupancy",))
        if isinstance(feats, str) or not hasattr(feats, "__iter__") or not all(isinstance(f, str) and f in VOXEL_FEATURES for f in feats):
            raise ValueError(f"voxel_grid: features must be a tuple drawn from 'occupancy' (implied) and 'rgb', got {feats!r}")
        out.features = VOXEL_FEATURES["occupancy"] | sum(VOXEL_FEATURES[f] for f in set(feats))
        dtype = v.pop("dtype", "uint8")
        try:
            dtype = dtype if isinstance(dtype, str) else np.dtype(dtype).name
        except TypeError:
            pass
        if dtype not in ("uint8", "float32"):
            raise ValueError(f"voxel_grid: dtype must be 'uint8' or 'float32', got {dtype!r}")
        out.dtype = STACK_DTYPES[dtype]
        source = v.pop("source", False)
        if not isinstance(source, (bool, np.bool_)):
            raise ValueError(f"voxel_grid: source must be a bool, got {source!r}")
        out.source = int(source)
        if v:
            raise ValueError(f"unknown voxel_grid fields {sorted(v)}")
        return out


class LcrVoxelGridView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("spec", VoxelGridSpec),           # cameras and ids resolved to the bits in use, the occupancy bit set
        ("inv_cell", ctypes.c_float * 3),  # cells per metre along x, y, z: the float32 values the kernel multiplies with
        ("channels", ctypes.c_int32),
        ("slots", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("voxels", ctypes.c_void_p),       # [N][C][Dz][Dy][Dx] of the element type
        ("source", ctypes.c_void_p),       # [N][Dz][Dy][Dx] int32, or NULL
        ("count", ctypes.c_void_p),        # [N] int32
        ("occupied", ctypes.c_void_p),     # [N] int32
        ("camera_pose", ctypes.c_void_p),  # [slots][13][N] float32
        ("bytes_per_env", ctypes.c_uint64),
    ]


class HeightmapSpec(ctypes.Structure):
    """lcr_heightmap_spec: box, cells, cameras, surface ids and channels of the heightmap (include/lcr.h)"""
    _fields_ = [
        ("lo", ctypes.c_float * 3),      # x, y, z of the box's lower corner, world frame; finite
        ("hi", ctypes.c_float * 3),      # x, y, z of the upper corner; finite, lo[k] < hi[k]
        ("dims", ctypes.c_int32 * 2),    # Hx (a multiple of 4), Hy: each 1 .. HEIGHTMAP_MAX_DIM, at most HEIGHTMAP_MAX_CELLS cells
        ("cameras", ctypes.c_uint32),    # STACK_CAMERAS bits; 0 = every camera the handle has
        ("ids", ctypes.c_uint32),        # bit i: surface id i is a candidate (1 .. 10); 0 = CLOUD_DEFAULT_IDS
        ("features", ctypes.c_uint32),   # HEIGHTMAP_FEATURES bits; the height is implied
        ("source", ctypes.c_int32),      # 0 | 1: keep the source index of every cell
    ]

    def as_dict(self):
        """the float32 corners in use as Python floats, cameras / features as names, ids as a tuple, as VoxelGridSpec.as_dict has them"""
        return {"lo": tuple(float(v) for v in self.lo), "hi": tuple(float(v) for v in self.hi), "dims": tuple(int(v) for v in self.dims),
                "cameras": tuple(n for n, b in STACK_CAMERAS.items() if self.cameras & b), "ids": tuple(i for i in range(32) if self.ids >> i & 1),
                "features": tuple(n for n, b in HEIGHTMAP_FEATURES.items() if self.features & b), "source": bool(self.source)}

    @classmethod
    def from_any(cls, v):
        """a HeightmapSpec, or a dict with box=((x0, y0, z0), (x1, y1, z1)) and dims=(Hx, Hy) -- neither has a default: the caller chooses the memory -- and some of
        cameras / ids / features / source"""
        import numpy as np

        if isinstance(v, cls):
            return v
        if not isinstance(v, dict):
            raise ValueError(f"heightmap must be None or a dict of box / dims / cameras / ids / features / source, got {v!r}")
        v = dict(v)
        out = cls()
        if "box" not in v or "dims" not in v:
            raise ValueError("heightmap needs box=((x0, y0, z0), (x1, y1, z1)) and dims=(Hx, Hy): neither has a default, the caller chooses the memory")
        box, dims = v.pop("box"), v.pop("dims")
        what = "heightmap: box must be ((x0, y0, z0), (x1, y1, z1)), the lower and the upper corner of a box in the world frame, six finite numbers"
        try:
            lo, hi = box
            lo, hi = list(lo), list(hi)
        except (TypeError, ValueError):
            raise ValueError(f"{what}, got {box!r}") from None
        if isinstance(box, str) or len(lo) != 3 or len(hi) != 3:
            raise ValueError(f"{what}, got {box!r}")
        for name, side, dst in (("lo", lo, out.lo), ("hi", hi, out.hi)):
            for k, x in enumerate(side):
                if isinstance(x, (bool, np.bool_, str)) or not isinstance(x, (int, float, np.integer, np.floating)):
                    raise ValueError(f"{what}; {name}[{k}] is {x!r}")
                x = np.float32(x)   # (the float32 value the kernel subtracts)
                if not np.isfinite(x):
                    raise ValueError(f"heightmap: box {name}[{k}] is not finite: the box of a heightmap has no open sides")
                dst[k] = float(x)
        for k, axis in enumerate("xyz"):
            if not out.lo[k] < out.hi[k]:
                raise ValueError(f"heightmap: box lo[{k}] >= hi[{k}]: the box is empty along {axis} (lo {out.lo[k]!r}, hi {out.hi[k]!r})")
        try:
            dims = list(dims)
        except TypeError:
            dims = []
        if len(dims) != 2 or any(isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, np.integer)) or not 1 <= d <= HEIGHTMAP_MAX_DIM for d in dims):
            raise ValueError(f"heightmap: dims must be (Hx, Hy), each an integer in 1 .. {HEIGHTMAP_MAX_DIM}, got {dims!r}")
        if dims[0] % 4:
            raise ValueError(f"heightmap: dims[0] (x) must be a multiple of 4, got {dims[0]!r}")
        if dims[0] * dims[1] > HEIGHTMAP_MAX_CELLS:
            raise ValueError(f"heightmap: dims {tuple(dims)!r} are {dims[0] * dims[1]} cells: at most {HEIGHTMAP_MAX_CELLS}")
        for k in range(2):
            out.dims[k] = int(dims[k])
        cams = v.pop("cameras", None)
        if cams is not None:
            if isinstance(cams, str) or not all(isinstance(c, str) and c in STACK_CAMERAS for c in cams) or len(cams) == 0:
                raise ValueError(f"heightmap: cameras must be a non-empty tuple drawn from 'front', 'top' and 'wrist', got {cams!r}")
            out.cameras = sum(STACK_CAMERAS[c] for c in set(cams))
        ids = v.pop("ids", None)
        if ids is not None:
            mask = 0
            ok = not isinstance(ids, str) and hasattr(ids, "__iter__")
            for i in (ids if ok else ()):
                if isinstance(i, str) and i in CLOUD_IDS:
                    mask |= CLOUD_IDS[i]
                elif isinstance(i, (int, np.integer)) and not isinstance(i, (bool, np.bool_)) and 1 <= i <= 10:
                    mask |= 1 << int(i)
                else:
                    ok = False
            if not ok or mask == 0:
                raise ValueError(f"heightmap: ids must be a non-empty tuple drawn from 'arm', 'cube', 'cube2', 'floor' and the surface ids 1 .. 10, got {ids!r}")
            out.ids = mask
        feats = v.pop("features", ("height",))
        if isinstance(feats, str) or not hasattr(feats, "__iter__") or not all(isinstance(f, str) and f in HEIGHTMAP_FEATURES for f in feats):
            raise ValueError(f"heightmap: features must be a tuple drawn from 'height' (implied) and 'rgb', got {feats!r}")
        out.features = HEIGHTMAP_FEATURES["height"] | sum(HEIGHTMAP_FEATURES[f] for f in set(feats))
        source = v.pop("source", False)
        if not isinstance(source, (bool, np.bool_)):
            raise ValueError(f"heightmap: source must be a bool, got {source!r}")
        out.source = int(source)
        if v:
            raise ValueError(f"unknown heightmap fields {sorted(v)}")
        return out


class LcrHeightmapView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("spec", HeightmapSpec),           # cameras and ids resolved to the bits in use, the height bit set
        ("inv_cell", ctypes.c_float * 2),  # cells per metre along x, y: the float32 values the kernel multiplies with
        ("channels", ctypes.c_int32),
        ("slots", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("heightmap", ctypes.c_void_p),    # [N][C][Hy][Hx] float32
        ("source", ctypes.c_void_p),       # [N][Hy][Hx] int32, or NULL
        ("count", ctypes.c_void_p),        # [N] int32
        ("filled", ctypes.c_void_p),       # [N] int32
        ("camera_pose", ctypes.c_void_p),  # [slots][13][N] float32
        ("bytes_per_env", ctypes.c_uint64),
    ]


class ObjectBoxesSpec(ctypes.Structure):
    """lcr_object_boxes_spec: cameras, objects (masks over the surface ids and the marker) and the depth switch of the object boxes (include/lcr.h)"""
    _fields_ = [
        ("cameras", ctypes.c_uint32),                      # STACK_CAMERAS bits, at least one
        ("n_objects", ctypes.c_int32),                     # 1 .. BOXES_MAX_OBJECTS
        ("objects", ctypes.c_uint32 * BOXES_MAX_OBJECTS),  # [i < n_objects]: bits 1 .. 10 and BOXES_MARKER
        ("depth", ctypes.c_int32),                         # 0 | 1: keep the nearest depth word of every record
    ]
    given = None   # the objects as the caller named them (from_any)

    def as_dict(self):
        """cameras as names, the objects as given (the masks where a raw spec gave none), the masks, depth as a bool"""
        masks = tuple(int(self.objects[i]) for i in range(self.n_objects))
        return {"cameras": tuple(n for n, b in STACK_CAMERAS.items() if self.cameras & b), "objects": masks if self.given is None else self.given, "masks": masks,
                "depth": bool(self.depth)}

    @staticmethod
    def mask_of(obj):
        """the mask of one object: a name of BOXES_OBJECTS, a surface id 1 .. 10, or a tuple of those (their union); None if it is none of these"""
        import numpy as np

        if isinstance(obj, str):
            return BOXES_OBJECTS.get(obj)
        if isinstance(obj, (int, np.integer)) and not isinstance(obj, (bool, np.bool_)):
            return 1 << int(obj) if 1 <= obj <= 10 else None
        if isinstance(obj, (tuple, list)) and len(obj) > 0:
            parts = [None if isinstance(o, (tuple, list)) else ObjectBoxesSpec.mask_of(o) for o in obj]
            if None not in parts:
                m = 0
                for x in parts:
                    m |= x
                return m
        return None

    @classmethod
    def from_any(cls, v, wrist=False):
        """an ObjectBoxesSpec, True (the defaults), or a dict with some of objects / cameras / depth.  `wrist`: the handle has a wrist camera (the default cameras are every
        camera the handle has)"""
        import numpy as np

        if isinstance(v, cls):
            return v
        if v is True:
            v = {}
        if not isinstance(v, dict):
            raise ValueError(f"object_boxes must be None, True or a dict of objects / cameras / depth, got {v!r}")
        v = dict(v)
        out = cls()
        names = "'" + "', '".join(BOXES_OBJECTS) + "'"
        objects = v.pop("objects", BOXES_DEFAULT_OBJECTS)
        what = (f"object_boxes: objects must be a non-empty tuple of at most {BOXES_MAX_OBJECTS} objects, each a name drawn from {names}, a surface id 1 .. 10 "
                f"or a tuple of those (their union)")
        if isinstance(objects, str) or not isinstance(objects, (tuple, list)) or not 1 <= len(objects) <= BOXES_MAX_OBJECTS:
            raise ValueError(f"{what}, got {objects!r}")
        for i, obj in enumerate(objects):
            m = cls.mask_of(obj)
            if m is None:
                raise ValueError(f"{what}; objects[{i}] is {obj!r}")
            out.objects[i] = m
        out.n_objects = len(objects)
        out.given = tuple(tuple(o) if isinstance(o, list) else o for o in objects)
        cams = v.pop("cameras", None)
        if cams is None:
            out.cameras = STACK_CAMERAS["front"] | STACK_CAMERAS["top"] | (STACK_CAMERAS["wrist"] if wrist else 0)
        else:
            if isinstance(cams, str) or not hasattr(cams, "__iter__") or not all(isinstance(c, str) and c in STACK_CAMERAS for c in cams) or len(cams) == 0:
                raise ValueError(f"object_boxes: cameras must be a non-empty tuple drawn from 'front', 'top' and 'wrist', got {cams!r}")
            out.cameras = sum(STACK_CAMERAS[c] for c in set(cams))
        depth = v.pop("depth", False)
        if not isinstance(depth, (bool, np.bool_)):
            raise ValueError(f"object_boxes: depth must be a bool, got {depth!r}")
        out.depth = int(depth)
        if v:
            raise ValueError(f"unknown object_boxes fields {sorted(v)}")
        return out


class LcrObjectBoxesView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("spec", ObjectBoxesSpec),           # as enabled; the masks beyond n_objects are 0
        ("slots", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("boxes", ctypes.c_void_p),          # [N][slots][O][8] int32
        ("bytes_per_env", ctypes.c_uint64),
    ]


class NormalsSpec(ctypes.Structure):
    """lcr_normals_spec: cameras and frame of the surface normals (include/lcr.h)"""
    _fields_ = [
        ("cameras", ctypes.c_uint32),   # STACK_CAMERAS bits; 0 = every camera the handle has
        ("frame", ctypes.c_int32),      # NORMALS_FRAMES
    ]

    def as_dict(self):
        """cameras and frame as names"""
        return {"cameras": tuple(n for n, b in STACK_CAMERAS.items() if self.cameras & b), "frame": {v: k for k, v in NORMALS_FRAMES.items()}[int(self.frame)]}

    @classmethod
    def from_any(cls, v, wrist=False):
        """a NormalsSpec, True (the defaults), or a dict with some of cameras / frame.  `wrist`: the handle has a wrist camera (the default cameras are every camera the
        handle has)"""
        if isinstance(v, cls):
            return v
        if v is True:
            v = {}
        if not isinstance(v, dict):
            raise ValueError(f"surface_normals must be None, True or a dict of cameras / frame, got {v!r}")
        v = dict(v)
        out = cls()
        cams = v.pop("cameras", None)
        if cams is None:
            out.cameras = STACK_CAMERAS["front"] | STACK_CAMERAS["top"] | (STACK_CAMERAS["wrist"] if wrist else 0)
        else:
            if isinstance(cams, str) or not hasattr(cams, "__iter__") or not all(isinstance(c, str) and c in STACK_CAMERAS for c in cams) or len(cams) == 0:
                raise ValueError(f"surface_normals: cameras must be a non-empty tuple drawn from 'front', 'top' and 'wrist', got {cams!r}")
            out.cameras = sum(STACK_CAMERAS[c] for c in set(cams))
        frame = v.pop("frame", "world")
        if not isinstance(frame, str) or frame not in NORMALS_FRAMES:
            raise ValueError(f"surface_normals: frame must be 'world' or 'camera', got {frame!r}")
        out.frame = NORMALS_FRAMES[frame]
        if v:
            raise ValueError(f"unknown surface_normals fields {sorted(v)}")
        return out


class LcrNormalsView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("spec", NormalsSpec),                  # as enabled, cameras resolved
        ("slots", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("normals_front", ctypes.c_void_p),     # [N][H][W][4] int8, or NULL
        ("normals_top", ctypes.c_void_p),
        ("normals_wrist", ctypes.c_void_p),
        ("boxes", ctypes.c_void_p),             # [9][15][N] float32
        ("camera_pose", ctypes.c_void_p),       # [slots][13][N] float32
        ("bytes_per_env", ctypes.c_uint64),
    ]


class MotionSpec(ctypes.Structure):
    """lcr_motion_spec: the cameras of the motion vectors (include/lcr.h)"""
    _fields_ = [
        ("cameras", ctypes.c_uint32),   # STACK_CAMERAS bits; 0 = every camera the handle has
    ]

    def as_dict(self):
        """cameras as names"""
        return {"cameras": tuple(n for n, b in STACK_CAMERAS.items() if self.cameras & b)}

    @classmethod
    def from_any(cls, v, wrist=False):
        """a MotionSpec, True (the defaults), or a dict with cameras.  `wrist`: the handle has a wrist camera (the default cameras are every camera the handle has)"""
        if isinstance(v, cls):
            return v
        if v is True:
            v = {}
        if not isinstance(v, dict):
            raise ValueError(f"motion_vectors must be None, True or a dict of cameras, got {v!r}")
        v = dict(v)
        out = cls()
        cams = v.pop("cameras", None)
        if cams is None:
            out.cameras = STACK_CAMERAS["front"] | STACK_CAMERAS["top"] | (STACK_CAMERAS["wrist"] if wrist else 0)
        else:
            if isinstance(cams, str) or not hasattr(cams, "__iter__") or not all(isinstance(c, str) and c in STACK_CAMERAS for c in cams) or len(cams) == 0:
                raise ValueError(f"motion_vectors: cameras must be a non-empty tuple drawn from 'front', 'top' and 'wrist', got {cams!r}")
            out.cameras = sum(STACK_CAMERAS[c] for c in set(cams))
        if v:
            raise ValueError(f"unknown motion_vectors fields {sorted(v)}")
        return out


class LcrMotionView(ctypes.Structure):
    _fields_ = [
        ("enabled", ctypes.c_int32),
        ("spec", MotionSpec),                   # as enabled, cameras resolved
        ("slots", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("flow_front", ctypes.c_void_p),        # [N][H][W][2] float16, or NULL
        ("flow_top", ctypes.c_void_p),
        ("flow_wrist", ctypes.c_void_p),
        ("valid", ctypes.c_void_p),             # [N] uint8
        ("boxes", ctypes.c_void_p),             # [2][9][15][N] float32: now, before
        ("camera_pose", ctypes.c_void_p),       # [2][slots][13][N] float32: now, before
        ("bytes_per_env", ctypes.c_uint64),
    ]


class LcrOutView(ctypes.Structure):
    _fields_ = [
        ("n_envs", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
        ("reward", ctypes.c_void_p),
        ("terminated", ctypes.c_void_p),
        ("truncated", ctypes.c_void_p),
        ("is_success", ctypes.c_void_p),
        ("did_reset", ctypes.c_void_p),
        ("terminal_obs", ctypes.c_void_p),
        ("terminal_quat", ctypes.c_void_p),
        ("timestamp", ctypes.c_void_p),
        ("current_goal", ctypes.c_void_p),
        ("active_mask", ctypes.c_void_p),
        ("active_count", ctypes.c_void_p),
        ("max_sweeps", ctypes.c_void_p),
        ("choice", ctypes.c_void_p),
        ("ctrl", ctypes.c_void_p),
    ]


class LcrHostView(ctypes.Structure):
    _fields_ = [
        ("n_envs", ctypes.c_int32),
        ("any_reset", ctypes.c_int32),
        ("arm_qpos", ctypes.c_void_p),
        ("arm_qvel", ctypes.c_void_p),
        ("cube_pos", ctypes.c_void_p),
        ("aux_pos", ctypes.c_void_p),
        ("reward", ctypes.c_void_p),
        ("terminated", ctypes.c_void_p),
        ("truncated", ctypes.c_void_p),
        ("is_success", ctypes.c_void_p),
        ("did_reset", ctypes.c_void_p),
        ("terminal_obs", ctypes.c_void_p),
    ]


class LcrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lcr error {code}: {msg}")
        self.code = code
        self.msg = msg


_lib = None


def load():
    """Load liblcr_hip.so; raises OSError with a build hint if it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(
            f"{LIB_PATH} not found: build it with `python -m gym_lowcostrobot_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    # PyTorch-ROCm wheels bundle their own HIP/HSA runtime (torch/lib/libamdhip64.so, same SONAME as the system one).  Two HIP
    # runtimes in one process do not coexist, so whichever of torch and this library comes first must settle on ONE copy.
    # If torch is installed but not imported yet, its bundled runtime is pre-loaded here BY PATH (no `import torch`): the
    # dynamic linker then resolves liblcr_hip.so's DT_NEEDED libamdhip64.so.7 to that already-loaded object, and a later
    # `import torch` finds its own runtime in place -- the import order no longer matters.  LCR_NO_TORCH_PRELOAD=1 skips this
    # (processes that never use torch run on the system runtime of /opt/rocm).
    if "torch" not in sys.modules and os.environ.get("LCR_NO_TORCH_PRELOAD") != "1":
        try:
            spec = importlib.util.find_spec("torch")
            rt = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so") if spec and spec.submodule_search_locations else None
            if rt and os.path.exists(rt):
                ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
        except Exception:
            pass
    L = ctypes.CDLL(LIB_PATH)
    _check_single_hip_runtime()
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    L.lcr_abi_version.restype = ctypes.c_int
    L.lcr_last_error.restype = ctypes.c_char_p
    L.lcr_config_default.argtypes = [ctypes.POINTER(LcrConfig), ctypes.c_int]
    L.lcr_config_preset.argtypes = [ctypes.POINTER(LcrConfig), ctypes.c_int, ctypes.c_int]
    L.lcr_action_dim.argtypes = [ctypes.POINTER(LcrConfig)]
    L.lcr_nq.argtypes = [ctypes.c_int]
    L.lcr_nv.argtypes = [ctypes.c_int]
    L.lcr_create.argtypes = [ctypes.POINTER(LcrConfig), ctypes.POINTER(vp)]
    L.lcr_destroy.argtypes = [vp]
    L.lcr_destroy.restype = None
    L.lcr_step_kernel_family.argtypes = [vp]
    L.lcr_get_redo_flags.argtypes = [vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.lcr_set_stream.argtypes = [vp, vp]
    L.lcr_sync.argtypes = [vp]
    L.lcr_reset.argtypes = [vp, vp, vp]
    L.lcr_step.argtypes = [vp, vp]
    L.lcr_step_host.argtypes = [vp, vp]
    L.lcr_get_obs.argtypes = [vp, ctypes.POINTER(LcrObsView)]
    L.lcr_get_outputs.argtypes = [vp, ctypes.POINTER(LcrOutView)]
    L.lcr_fetch_host.argtypes = [vp, ctypes.POINTER(LcrHostView)]
    L.lcr_get_state.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lcr_set_state.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lcr_malloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.lcr_free.argtypes = [vp, vp]
    L.lcr_memcpy_h2d.argtypes = [vp, vp, vp, ctypes.c_size_t]
    L.lcr_memcpy_d2h.argtypes = [vp, vp, vp, ctypes.c_size_t]
    L.lcr_timer_begin.argtypes = [vp]
    L.lcr_timer_end.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.lcr_fill_random_actions.argtypes = [vp, vp, u64, u64]
    L.lcr_calibrate_copy.argtypes = [vp, vp, ctypes.c_size_t]
    L.lcr_render.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.lcr_render_state.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    L.lcr_render_terminal.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    L.lcr_enable_image_planes.argtypes = [vp, ctypes.c_uint32, ctypes.c_float]
    L.lcr_get_image_planes.argtypes = [vp, ctypes.POINTER(LcrPlanesView)]
    L.lcr_render_planes.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    L.lcr_render_state_planes.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    L.lcr_render_terminal_planes.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp]
    L.lcr_look_variant_default.argtypes = [ctypes.POINTER(LookVariant)]
    L.lcr_enable_look.argtypes = [vp, ctypes.c_int, ctypes.POINTER(LookVariant), ctypes.POINTER(LookSampler)]
    L.lcr_set_look.argtypes = [vp, vp, vp, vp]
    L.lcr_get_look.argtypes = [vp, vp, vp, vp]
    L.lcr_wrist_camera_default.argtypes = [ctypes.POINTER(WristCamera)]
    L.lcr_wrist_camera_check.argtypes = [ctypes.POINTER(WristCamera)]
    L.lcr_enable_wrist_camera.argtypes = [vp, ctypes.POINTER(WristCamera)]
    L.lcr_get_wrist_camera.argtypes = [vp, ctypes.POINTER(LcrWristView)]
    L.lcr_render_terminal_wrist.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
    L.lcr_obs_stack_check.argtypes = [ctypes.POINTER(ObsStackSpec)]
    L.lcr_enable_obs_stack.argtypes = [vp, ctypes.POINTER(ObsStackSpec)]
    L.lcr_get_obs_stack.argtypes = [vp, ctypes.POINTER(LcrObsStackView)]
    L.lcr_point_cloud_check.argtypes = [ctypes.POINTER(PointCloudSpec)]
    L.lcr_enable_point_cloud.argtypes = [vp, ctypes.POINTER(PointCloudSpec)]
    L.lcr_get_point_cloud.argtypes = [vp, ctypes.POINTER(LcrPointCloudView)]
    L.lcr_point_cloud_sampling_check.argtypes = [ctypes.POINTER(PointCloudSpec), ctypes.POINTER(PointCloudSampling)]
    L.lcr_enable_point_cloud_sampled.argtypes = [vp, ctypes.POINTER(PointCloudSpec), ctypes.POINTER(PointCloudSampling)]
    L.lcr_get_point_cloud_sampling.argtypes = [vp, ctypes.POINTER(PointCloudSampling)]
    L.lcr_point_cloud_crop_check.argtypes = [ctypes.POINTER(PointCloudCrop)]
    L.lcr_enable_point_cloud_cropped.argtypes = [vp, ctypes.POINTER(PointCloudSpec), ctypes.POINTER(PointCloudSampling), ctypes.POINTER(PointCloudCrop)]
    L.lcr_get_point_cloud_crop.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(PointCloudCrop)]
    L.lcr_enable_obs_stack_terminal.argtypes = [vp, ctypes.POINTER(ObsStackSpec), i32]
    L.lcr_get_obs_stack_terminal.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(vp), ctypes.POINTER(u64)]
    L.lcr_obs_stack_terminal.argtypes = [vp, vp, ctypes.c_int, vp]
    L.lcr_enable_obs_stack_planes.argtypes = [vp, ctypes.POINTER(ObsStackSpec), i32, ctypes.c_uint32]
    L.lcr_get_obs_stack_planes.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.lcr_point_cloud_terminal.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp]
    L.lcr_voxel_grid_check.argtypes = [ctypes.POINTER(VoxelGridSpec)]
    L.lcr_enable_voxel_grid.argtypes = [vp, ctypes.POINTER(VoxelGridSpec)]
    L.lcr_get_voxel_grid.argtypes = [vp, ctypes.POINTER(LcrVoxelGridView)]
    L.lcr_heightmap_check.argtypes = [ctypes.POINTER(HeightmapSpec)]
    L.lcr_enable_heightmap.argtypes = [vp, ctypes.POINTER(HeightmapSpec)]
    L.lcr_get_heightmap.argtypes = [vp, ctypes.POINTER(LcrHeightmapView)]
    L.lcr_object_boxes_check.argtypes = [ctypes.POINTER(ObjectBoxesSpec)]
    L.lcr_enable_object_boxes.argtypes = [vp, ctypes.POINTER(ObjectBoxesSpec)]
    L.lcr_get_object_boxes.argtypes = [vp, ctypes.POINTER(LcrObjectBoxesView)]
    L.lcr_normals_check.argtypes = [ctypes.POINTER(NormalsSpec)]
    L.lcr_enable_normals.argtypes = [vp, ctypes.POINTER(NormalsSpec)]
    L.lcr_get_normals.argtypes = [vp, ctypes.POINTER(LcrNormalsView)]
    L.lcr_motion_check.argtypes = [ctypes.POINTER(MotionSpec)]
    L.lcr_enable_motion_vectors.argtypes = [vp, ctypes.POINTER(MotionSpec)]
    L.lcr_get_motion_vectors.argtypes = [vp, ctypes.POINTER(LcrMotionView)]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name not in ("lcr_last_error", "lcr_destroy"):
            fn.restype = ctypes.c_int
    if L.lcr_abi_version() != ABI_VERSION:
        raise OSError(f"liblcr_hip.so ABI {L.lcr_abi_version()} != binding ABI {ABI_VERSION}: rebuild")
    _lib = L
    return L


def _check_single_hip_runtime():
    """Two HIP runtimes in one process do not coexist (the second one sees no GPU).  The by-path preload above only unifies them when
    torch's bundled libamdhip64 has the SONAME liblcr_hip.so was linked against (libamdhip64.so.7 for ROCm 7.x wheels); with a torch
    wheel built for another ROCm major both would be mapped: say so loudly instead of failing later with 'no HIP device'."""
    try:
        with open("/proc/self/maps") as f:
            libs = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    real = {os.path.realpath(p) for p in libs}
    if len(real) > 1:
        import warnings

        warnings.warn("two HIP runtimes are mapped in this process (" + ", ".join(sorted(real)) + "): liblcr_hip.so was built against the "
                      "ROCm 7 runtime (libamdhip64.so.7); use a PyTorch-ROCm wheel of the same ROCm major, or set LCR_NO_TORCH_PRELOAD=1 and "
                      "import torch in a different process", RuntimeWarning, stacklevel=3)


def check(rc):
    if rc < 0:
        L = load()
        msg = L.lcr_last_error().decode("utf-8", "replace")
        if rc == LCR_ERR_INVALID:
            raise ValueError(msg)
        raise LcrError(rc, msg)
    return rc
