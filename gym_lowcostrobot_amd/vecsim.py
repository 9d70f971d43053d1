"""VecSim: N independent low-cost-robot environments stepped in lockstep on one MI355X.

Thin host-side mirror of the reference env classes' reset()/step() for a batch (reference:
gym_lowcostrobot/envs/reach_cube_env.py:297-333 and the four sibling files).  All arithmetic happens in
the HIP kernels behind the C ABI (include/lcr.h); this file only owns handles and moves bytes.
"""
import ctypes
import os

import numpy as np

from . import _capi
from ._capi import ACTION_MODES, OBS_MODES, REWARD_TYPES, TASKS, LcrConfig, LcrHostView, LcrObsView, LcrOutView, LcrPlanesView, check

CAMERAS = {"camera_front": 0, "camera_top": 1, "camera_vizu": 2, "camera_wrist": 3}   # (camera_wrist: on a sim with a wrist camera)


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class DeviceArray:
    """A typed view of device memory exposing __cuda_array_interface__ (zero-copy into torch on ROCm)."""

    def __init__(self, sim, ptr, shape, dtype, readonly=True):
        self._sim = sim  # keeps the owner alive
        self.ptr = int(ptr)
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.__cuda_array_interface__ = {
            "shape": self.shape,
            "typestr": self.dtype.str,
            "data": (self.ptr, False),  # torch rejects read-only exports; observation views are read-only by convention
            "version": 3,
            "strides": None,
        }

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        check(self._sim.L.lcr_memcpy_d2h(self._sim.handle, _vp(out), ctypes.c_void_p(self.ptr), self.nbytes))
        return out

    def torch(self):
        """zero-copy torch view; image views, planes, wrist frames, the stack and the point cloud are read on the handle's stream after VecSim.wait_frames() or any other joining call (lcr.h: lcr_step)"""
        import torch

        return torch.as_tensor(self, device=f"cuda:{self._sim.device}")


class VecSim:
    def __init__(
        self,
        task,
        n_envs=1,
        *,
        device=0,
        env_id_offset=0,
        observation_mode="state",
        action_mode="joint",
        reward_type="sparse",
        block_gripper=None,
        distance_threshold=0.05,
        cube_xy_range=0.3,
        target_xy_range=0.3,
        goal_z_range=0.1,
        height_threshold=0.1,
        n_substeps=20,
        max_episode_steps=50,
        impratio=100.0,
        pgs_iters=None,
        compat=0,
        auto_reset=True,
        base_seed=0,
        arm_collision=True,
        pgs_tol=1e-6,
        diagnostics=False,
        finger_cube_condim=None,
        step_kernel="auto",
        cc_points=None,
        global_envs=None,
        profile=None,
        preset=None,
        solver=None,
        newton_iters=None,
        ls_iters=None,
        newton_tol=None,
        ls_tol=None,
        finger_floor_condim=None,
        coop_share=None,
        image_size=None,
        image_planes=(),
        depth_far=10.0,
        look_variants=None,
        look_sampler=None,
        wrist_camera=None,
        obs_stack=None,
        point_cloud=None,
        voxel_grid=None,
        heightmap=None,
        object_boxes=None,
        surface_normals=None,
        motion_vectors=None,
    ):
        self.L = _capi.load()
        if action_mode not in ACTION_MODES:
            raise ValueError("Invalid action mode, must be 'ee' or 'joint'")  # reach_cube_env.py:269-270
        if observation_mode not in OBS_MODES:
            raise ValueError(f"invalid observation_mode {observation_mode!r}")
        if reward_type not in REWARD_TYPES:
            raise ValueError(f"invalid reward_type {reward_type!r}")
        # depth / segmentation planes beside the colour frames (lcr_enable_image_planes): checked here, before the library is asked for a device
        if isinstance(image_planes, str) or any(p not in _capi.IMAGE_PLANES for p in image_planes):
            raise ValueError(f"image_planes must be a tuple drawn from 'depth' and 'segmentation', got {image_planes!r}")
        image_planes = tuple(p for p in _capi.IMAGE_PLANES if p in image_planes)   # (canonical order, no repeats)
        if image_planes and observation_mode == "state":
            raise ValueError("image_planes need image observations: observation_mode 'image' or 'both'")
        try:
            depth_far = float(depth_far)
        except (TypeError, ValueError):
            raise ValueError(f"depth_far must be a number of metres in (0, 1000], got {depth_far!r}") from None
        if not (np.isfinite(depth_far) and 0.0 < depth_far <= 1000.0):
            raise ValueError(f"depth_far must be finite and in (0, 1000] metres, got {depth_far!r}")
        # the look of the frames (lcr_enable_look): a list of variants (LookVariant or dicts over the default variant) and an optional sampler of the per-env colours
        if look_sampler is not None and look_variants is None:
            look_variants = [{}]
        if look_variants is not None:
            if observation_mode == "state":
                raise ValueError("look_variants need image observations: observation_mode 'image' or 'both'")
            look_variants = [_capi.LookVariant.from_any(v) for v in look_variants]
            look_sampler = None if look_sampler is None else _capi.LookSampler.from_any(look_sampler)
        # the wrist camera (lcr_enable_wrist_camera): None / False = none, True = the default mount, or a dict of link / pos / xyaxes / fovy_deg over it.  The library checks
        # the mount itself here, without a handle (lcr_wrist_camera_check), as it does again when it is enabled
        if wrist_camera is None or wrist_camera is False:
            wrist_camera = None
        else:
            if observation_mode == "state":
                raise ValueError("wrist_camera needs image observations: observation_mode 'image' or 'both'")
            wrist_camera = _capi.WristCamera.from_any(wrist_camera)
            check(self.L.lcr_wrist_camera_check(ctypes.byref(wrist_camera)))
        # the observation stack (lcr_enable_obs_stack): None = none, an int = that many frames of every camera as uint8, or a dict of frames / cameras / dtype / reset_fill.
        # Checked here and by the library without a handle (lcr_obs_stack_check), before it is asked for a device
        # terminal=True in the dict (lcr_enable_obs_stack_terminal): the library keeps the history of an episode that ends, obs_stack_terminal() returns its stack
        # planes=("depth",) in the dict (lcr_enable_obs_stack_planes): every camera contributes r, g, b, d -- the depth plane, which image_planes must have, as a channel
        stack_terminal = cloud_terminal = False
        stack_planes = 0
        if obs_stack is not None:
            if observation_mode == "state":
                raise ValueError("obs_stack needs image observations: observation_mode 'image' or 'both'")
            obs_stack, stack_terminal = _capi.take_terminal(obs_stack, "obs_stack")
            obs_stack, stack_planes = _capi.take_stack_planes(obs_stack, image_planes)
            obs_stack = _capi.ObsStackSpec.from_any(obs_stack)
            if obs_stack.cameras & _capi.STACK_CAMERAS["wrist"] and wrist_camera is None:
                raise ValueError("obs_stack: cameras selects 'wrist', but no wrist_camera is given")
            check(self.L.lcr_obs_stack_check(ctypes.byref(obs_stack)))
        # the point cloud (lcr_enable_point_cloud): None = none, an int = that many points of every camera (arm and cubes, x y z), or a dict of points / cameras / ids / colors
        # and, for farthest-point sampling from a strided pool (lcr_enable_point_cloud_sampled), sampling="fps" and pool=Q; and, for a workspace crop box in the world frame
        # (lcr_enable_point_cloud_cropped), crop=((x0, y0, z0), (x1, y1, z1)) with None for an open side.
        # Checked here and by the library without a handle (lcr_point_cloud_check), before it is asked for a device.  It is made of both planes: they are not switched on silently
        if point_cloud is not None:
            if observation_mode == "state":
                raise ValueError("point_cloud needs image observations: observation_mode 'image' or 'both'")
            # (`terminal`: the caller's declaration that they want the clouds of episodes that end -- point_cloud_terminal() needs no state and works without it)
            point_cloud, cloud_terminal = _capi.take_terminal(point_cloud, "point_cloud")
            point_cloud, cloud_crop = _capi.PointCloudCrop.take(point_cloud)           # (`crop`: None without one)
            point_cloud, cloud_sampling = _capi.PointCloudSampling.take(point_cloud)   # (`sampling` and `pool`: the spec keeps its four fields)
            point_cloud = _capi.PointCloudSpec.from_any(point_cloud)
            if point_cloud.cameras & _capi.STACK_CAMERAS["wrist"] and wrist_camera is None:
                raise ValueError("point_cloud: cameras selects 'wrist', but no wrist_camera is given")
            if set(image_planes) != set(_capi.IMAGE_PLANES):
                raise ValueError(f"point_cloud is made of the depth and the segmentation plane: pass both, image_planes=('depth', 'segmentation') (got {image_planes!r})")
            check(self.L.lcr_point_cloud_check(ctypes.byref(point_cloud)))
            if cloud_sampling.mode == _capi.CLOUD_SAMPLINGS["fps"] and cloud_sampling.pool < point_cloud.points:
                raise ValueError(f"point_cloud: pool must be at least points ({point_cloud.points}), got {cloud_sampling.pool}")
            check(self.L.lcr_point_cloud_sampling_check(ctypes.byref(point_cloud), ctypes.byref(cloud_sampling)))
            if cloud_crop is not None:
                check(self.L.lcr_point_cloud_crop_check(ctypes.byref(cloud_crop)))
        # the voxel grid (lcr_enable_voxel_grid): None = none, or a dict of box=((x0, y0, z0), (x1, y1, z1)) and dims=(Dx, Dy, Dz) -- no defaults: the caller chooses the memory --
        # and some of cameras / ids / features ("occupancy", "rgb") / dtype ("uint8" | "float32") / source.  Checked here and by the library without a handle
        # (lcr_voxel_grid_check), before it is asked for a device.  It is made of both planes: they are not switched on silently
        if voxel_grid is not None:
            if observation_mode == "state":
                raise ValueError("voxel_grid needs image observations: observation_mode 'image' or 'both'")
            voxel_grid = _capi.VoxelGridSpec.from_any(voxel_grid)
            if voxel_grid.cameras & _capi.STACK_CAMERAS["wrist"] and wrist_camera is None:
                raise ValueError("voxel_grid: cameras selects 'wrist', but no wrist_camera is given")
            if set(image_planes) != set(_capi.IMAGE_PLANES):
                raise ValueError(f"voxel_grid is made of the depth and the segmentation plane: pass both, image_planes=('depth', 'segmentation') (got {image_planes!r})")
            check(self.L.lcr_voxel_grid_check(ctypes.byref(voxel_grid)))
        # the heightmap (lcr_enable_heightmap): None = none, or a dict of box=((x0, y0, z0), (x1, y1, z1)) and dims=(Hx, Hy) -- no defaults: the caller chooses the memory --
        # and some of cameras / ids / features ("height", "rgb") / source.  Checked here and by the library without a handle (lcr_heightmap_check), before it is asked for a
        # device.  It is made of both planes: they are not switched on silently
        if heightmap is not None:
            if observation_mode == "state":
                raise ValueError("heightmap needs image observations: observation_mode 'image' or 'both'")
            heightmap = _capi.HeightmapSpec.from_any(heightmap)
            if heightmap.cameras & _capi.STACK_CAMERAS["wrist"] and wrist_camera is None:
                raise ValueError("heightmap: cameras selects 'wrist', but no wrist_camera is given")
            if set(image_planes) != set(_capi.IMAGE_PLANES):
                raise ValueError(f"heightmap is made of the depth and the segmentation plane: pass both, image_planes=('depth', 'segmentation') (got {image_planes!r})")
            check(self.L.lcr_heightmap_check(ctypes.byref(heightmap)))
        # the object boxes (lcr_enable_object_boxes): None / False = none, True = the defaults, or a dict with some of objects (names, surface ids, tuples of those) /
        # cameras / depth.  Checked here and by the library without a handle (lcr_object_boxes_check), before it is asked for a device.  They are made of the segmentation
        # plane and, with depth=True, the depth plane: neither is switched on silently
        if object_boxes is None or object_boxes is False:
            object_boxes = None
        else:
            if observation_mode == "state":
                raise ValueError("object_boxes needs image observations: observation_mode 'image' or 'both'")
            object_boxes = _capi.ObjectBoxesSpec.from_any(object_boxes, wrist=wrist_camera is not None)
            if object_boxes.cameras & _capi.STACK_CAMERAS["wrist"] and wrist_camera is None:
                raise ValueError("object_boxes: cameras selects 'wrist', but no wrist_camera is given")
            if "segmentation" not in image_planes:
                raise ValueError(f"object_boxes is made of the segmentation plane: pass it, image_planes=('segmentation',) (got {image_planes!r})")
            if object_boxes.depth and "depth" not in image_planes:
                raise ValueError(f"object_boxes: depth=True keeps the nearest depth of every record and needs the depth plane: image_planes=('depth', 'segmentation') (got {image_planes!r})")
            check(self.L.lcr_object_boxes_check(ctypes.byref(object_boxes)))
        # the surface normals (lcr_enable_normals): None / False = none, True = the defaults (every camera the handle has, world frame), or a dict with some of cameras /
        # frame ("world" | "camera").  Checked here and by the library without a handle (lcr_normals_check), before it is asked for a device.  They are made of the depth and
        # the segmentation plane: neither is switched on silently
        if surface_normals is None or surface_normals is False:
            surface_normals = None
        else:
            if observation_mode == "state":
                raise ValueError("surface_normals needs image observations: observation_mode 'image' or 'both'")
            surface_normals = _capi.NormalsSpec.from_any(surface_normals, wrist=wrist_camera is not None)
            if surface_normals.cameras & _capi.STACK_CAMERAS["wrist"] and wrist_camera is None:
                raise ValueError("surface_normals: cameras selects 'wrist', but no wrist_camera is given")
            for plane in _capi.IMAGE_PLANES:
                if plane not in image_planes:
                    raise ValueError(f"surface_normals is made of the depth and the segmentation plane: the {plane} plane is missing, pass both, "
                                     f"image_planes=('depth', 'segmentation') (got {image_planes!r})")
            check(self.L.lcr_normals_check(ctypes.byref(surface_normals)))
        # the motion vectors (lcr_enable_motion_vectors): None / False = none, True = every camera the handle has, or a dict with cameras.  Checked here and by the library
        # without a handle (lcr_motion_check), before it is asked for a device.  They are made of the depth and the segmentation plane: neither is switched on silently
        if motion_vectors is None or motion_vectors is False:
            motion_vectors = None
        else:
            if observation_mode == "state":
                raise ValueError("motion_vectors needs image observations: observation_mode 'image' or 'both'")
            motion_vectors = _capi.MotionSpec.from_any(motion_vectors, wrist=wrist_camera is not None)
            if motion_vectors.cameras & _capi.STACK_CAMERAS["wrist"] and wrist_camera is None:
                raise ValueError("motion_vectors: cameras selects 'wrist', but no wrist_camera is given")
            for plane in _capi.IMAGE_PLANES:
                if plane not in image_planes:
                    raise ValueError(f"motion_vectors is made of the depth and the segmentation plane: the {plane} plane is missing, pass both, "
                                     f"image_planes=('depth', 'segmentation') (got {image_planes!r})")
            check(self.L.lcr_motion_check(ctypes.byref(motion_vectors)))
        self.task_name = task if isinstance(task, str) else {v: k for k, v in TASKS.items()}[task]
        cfg = LcrConfig()
        # preset: "faithful" (the reference's contact model solved by Newton's method) | "fast" (rounds 1-4: four sweeps, fewer rows); None = the library's default
        if preset is None:
            preset = os.environ.get("LCR_PRESET") or None   # (what the single-env facade classes, whose constructors are the reference's, can be switched with)
        if preset is None:
            check(self.L.lcr_config_default(ctypes.byref(cfg), TASKS[self.task_name]))
        else:
            if preset not in _capi.PRESETS:
                raise ValueError(f"invalid preset {preset!r} (faithful | fast)")
            check(self.L.lcr_config_preset(ctypes.byref(cfg), TASKS[self.task_name], _capi.PRESETS[preset]))
        cfg.n_envs = int(n_envs)
        cfg.device = int(device)
        cfg.env_id_offset = int(env_id_offset)
        cfg.action_mode = ACTION_MODES[action_mode]
        cfg.obs_mode = OBS_MODES[observation_mode]
        cfg.reward_type = REWARD_TYPES[reward_type]
        cfg.block_gripper = -1 if block_gripper is None else int(bool(block_gripper))
        cfg.distance_threshold = distance_threshold
        cfg.cube_xy_range = cube_xy_range
        cfg.target_xy_range = target_xy_range
        cfg.goal_z_range = goal_z_range
        cfg.height_threshold = height_threshold
        cfg.impratio = impratio
        cfg.n_substeps = int(n_substeps)
        cfg.max_episode_steps = int(max_episode_steps)
        if pgs_iters is not None:
            cfg.pgs_iters = int(pgs_iters)
        if solver is not None:
            if solver not in _capi.SOLVERS:
                raise ValueError(f"invalid solver {solver!r} (pgs | newton)")
            cfg.solver = _capi.SOLVERS[solver]
        for name, val in (("newton_iters", newton_iters), ("ls_iters", ls_iters), ("finger_floor_condim", finger_floor_condim)):
            if val is not None:
                setattr(cfg, name, int(val))
        for name, val in (("newton_tol", newton_tol), ("ls_tol", ls_tol)):
            if val is not None:
                setattr(cfg, name, float(val))
        cfg.compat = int(compat)
        cfg.auto_reset = int(bool(auto_reset))
        cfg.base_seed = int(base_seed)
        cfg.arm_collision = int(bool(arm_collision))
        cfg.pgs_tol = float(pgs_tol)
        # diagnostics is a boolean here (the decision signature + data.ctrl of every step); the profiling aids that reuse those arrays as
        # per-wave cycle counters are a separate, named argument: profile="wave_cycles" (one-wave kernels) | "phase_cycles" (two-wave kernels)
        if diagnostics not in (False, True, 0, 1):
            raise ValueError(f"diagnostics must be a bool, got {diagnostics!r} (cycle read-back: profile='wave_cycles' | 'phase_cycles')")
        if profile not in _capi.PROFILE_MODES:
            raise ValueError(f"invalid profile {profile!r} (None | 'wave_cycles' | 'phase_cycles')")
        cfg.diagnostics = _capi.PROFILE_MODES[profile] if profile is not None else int(bool(diagnostics))
        if finger_cube_condim is not None:   # default: lcr_config_default's choice for the task (6 for PushCubeLoop, else 4)
            cfg.finger_cube_condim = int(finger_cube_condim)
        if step_kernel not in _capi.STEP_KERNELS:
            raise ValueError(f"invalid step_kernel {step_kernel!r} (auto | single | coop)")
        cfg.step_kernel = _capi.STEP_KERNELS[step_kernel]   # kernel family: "auto" = by task and JOB size (global_envs), never by shard size
        if global_envs is not None:   # envs of the whole job this sim is a shard of: every shard declares the same number -> same family, same bits
            cfg.global_envs = int(global_envs)
        if cc_points is not None:   # StackTwoCubes: 4 (default) or 8 cube<->cube manifold points
            cfg.cc_points = int(cc_points)
        if coop_share not in _capi.COOP_SHARE:   # one-cube Newton kernel: who solves a wave's coupled envs (None = the library's default; "owner" | "shared" | "handoff" | "ahead" | "early": A/B runs, bit-identical)
            raise ValueError(f"invalid coop_share {coop_share!r} (None | 'owner' | 'shared' | 'handoff' | 'ahead' | 'early')")
        cfg.coop_share = _capi.COOP_SHARE[coop_share]
        if image_size is not None:   # (height, width) of the image observations, numpy order as the arrays are (N, H, W, 3); None = 240 x 320.  The library checks the values
            try:
                ih, iw = (int(v) for v in image_size)
            except (TypeError, ValueError):
                raise ValueError(f"image_size must be None or (height, width), got {image_size!r}") from None
            cfg.image_height, cfg.image_width = ih, iw
        self.cfg = cfg
        self.n = int(n_envs)
        self.device = int(device)
        self.action_dim = check(self.L.lcr_action_dim(ctypes.byref(cfg)))
        self.nq = self.L.lcr_nq(cfg.task)
        self.nv = self.L.lcr_nv(cfg.task)
        h = ctypes.c_void_p()
        check(self.L.lcr_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.handle = h
        fam = self.L.lcr_step_kernel_family(self.handle)
        self.step_kernel_family = {0: "one wave per 64 envs (lcr_step_kernel)", 1: "two cooperating waves per 64 envs (lcr_step2_kernel, one wave per SIMD)",
                                   2: "two cooperating waves per 64 envs (lcr_step2_kernel, two waves per SIMD)"}[fam]
        self.step_kernel_name = "lcr_step_kernel" if fam == 0 else "lcr_step2_kernel"
        ov, out = LcrObsView(), LcrOutView()
        check(self.L.lcr_get_obs(self.handle, ctypes.byref(ov)))
        check(self.L.lcr_get_outputs(self.handle, ctypes.byref(out)))
        N = self.n
        self.has_aux = bool(ov.has_aux)
        self.aux_name = {"push": "target_pos", "pick_place": "target_pos", "stack": "cube_blue_pos"}.get(self.task_name)
        self.cube_name = "cube_red_pos" if self.task_name == "stack" else "cube_pos"
        self.arm_qpos = DeviceArray(self, ov.arm_qpos, (6, N), np.float32)
        self.arm_qvel = DeviceArray(self, ov.arm_qvel, (6, N), np.float32)
        self.cube_pos = DeviceArray(self, ov.cube_pos, (3, N), np.float32)
        self.aux_pos = DeviceArray(self, ov.aux_pos, (3, N), np.float32) if ov.has_aux else None
        self.image_size = (int(ov.image_height), int(ov.image_width)) if ov.image_front else (int(cfg.image_height) or _capi.IMG_H, int(cfg.image_width) or _capi.IMG_W)
        img = (N,) + self.image_size + (3,)
        self.image_front = DeviceArray(self, ov.image_front, img, np.uint8) if ov.image_front else None
        self.image_top = DeviceArray(self, ov.image_top, img, np.uint8) if ov.image_top else None
        self.look_variants, self.look_sampler = look_variants, look_sampler
        if look_variants is not None:   # (before the planes: their cached backgrounds are drawn per variant)
            try:
                arr = (_capi.LookVariant * len(look_variants))(*look_variants)
                check(self.L.lcr_enable_look(self.handle, len(look_variants), arr, None if look_sampler is None else ctypes.byref(look_sampler)))
            except Exception:
                self.close()
                raise
        self.wrist_camera = None
        self.image_wrist = self.depth_wrist = self.seg_wrist = None
        if wrist_camera is not None:   # (before the planes: planes enabled afterwards cover the wrist camera)
            try:
                check(self.L.lcr_enable_wrist_camera(self.handle, ctypes.byref(wrist_camera)))
                wv = _capi.LcrWristView()
                check(self.L.lcr_get_wrist_camera(self.handle, ctypes.byref(wv)))
            except Exception:
                self.close()
                raise
            self.wrist_camera = wv.camera.as_dict()
            self.image_wrist = DeviceArray(self, wv.image_wrist, img, np.uint8)
        self.image_planes, self.depth_far = image_planes, depth_far
        self.depth_front = self.depth_top = self.seg_front = self.seg_top = None
        if image_planes:
            try:
                check(self.L.lcr_enable_image_planes(self.handle, sum(_capi.IMAGE_PLANES[p] for p in image_planes), depth_far))
                pv = LcrPlanesView()
                check(self.L.lcr_get_image_planes(self.handle, ctypes.byref(pv)))
            except Exception:
                self.close()
                raise
            self.depth_far = float(pv.depth_far)   # (as the library holds it: float32)
            pl = (N,) + self.image_size
            self.depth_front = DeviceArray(self, pv.depth_front, pl, np.float32) if pv.depth_front else None
            self.depth_top = DeviceArray(self, pv.depth_top, pl, np.float32) if pv.depth_top else None
            self.seg_front = DeviceArray(self, pv.seg_front, pl, np.uint8) if pv.seg_front else None
            self.seg_top = DeviceArray(self, pv.seg_top, pl, np.uint8) if pv.seg_top else None
            if self.wrist_camera is not None:
                wv = _capi.LcrWristView()
                check(self.L.lcr_get_wrist_camera(self.handle, ctypes.byref(wv)))
                self.depth_wrist = DeviceArray(self, wv.depth_wrist, pl, np.float32) if wv.depth_wrist else None
                self.seg_wrist = DeviceArray(self, wv.seg_wrist, pl, np.uint8) if wv.seg_wrist else None
        self.obs_stack = self.obs_stack_spec = None
        self.obs_stack_keeps_terminal = False   # obs_stack=dict(..., terminal=True): obs_stack_terminal() works
        self.obs_stack_history = None           # ... and, with more than one frame, the history (N, K - 1, C, H, W) the library keeps for it
        self.obs_stack_planes = ()              # obs_stack=dict(..., planes=("depth",)): ("depth",), every camera's channels are r, g, b, d
        self.obs_stack_depth_scale = None       # ... and {"inv_far": ..., "s255": ...}, the float32 constants of the depth element as the library holds them
        self.point_cloud_wants_terminal = cloud_terminal   # point_cloud=dict(..., terminal=True): what the vector adapters look at; point_cloud_terminal() works either way
        if obs_stack is not None:   # (last: behind look, wrist camera and planes)
            try:
                # (planes 0: lcr_enable_obs_stack_terminal; terminal False too: lcr_enable_obs_stack)
                check(self.L.lcr_enable_obs_stack_planes(self.handle, ctypes.byref(obs_stack), int(stack_terminal), int(stack_planes)))
                sv = _capi.LcrObsStackView()
                check(self.L.lcr_get_obs_stack(self.handle, ctypes.byref(sv)))
                pmask, inv_far, s255 = ctypes.c_uint32(0), ctypes.c_float(0), ctypes.c_float(0)
                check(self.L.lcr_get_obs_stack_planes(self.handle, ctypes.byref(pmask), ctypes.byref(inv_far), ctypes.byref(s255)))
                keep, hist, hist_bytes = ctypes.c_int32(0), ctypes.c_void_p(), ctypes.c_uint64(0)
                check(self.L.lcr_get_obs_stack_terminal(self.handle, ctypes.byref(keep), ctypes.byref(hist), ctypes.byref(hist_bytes)))
            except Exception:
                self.close()
                raise
            self.obs_stack_keeps_terminal = bool(keep.value)
            if pmask.value & _capi.PLANE_DEPTH:
                self.obs_stack_planes = ("depth",)
                self.obs_stack_depth_scale = {"inv_far": float(inv_far.value), "s255": float(s255.value)}
            if hist.value:
                self.obs_stack_history = DeviceArray(self, hist.value, (N, int(sv.spec.frames) - 1, int(sv.channels)) + self.image_size, np.dtype(sv.spec.as_dict()["dtype"]))
            self.obs_stack_spec = sv.spec.as_dict()
            self.obs_stack = DeviceArray(self, sv.data, (N, int(sv.spec.frames), int(sv.channels)) + self.image_size, np.dtype(self.obs_stack_spec["dtype"]))
        self.point_cloud = self.point_cloud_count = self.point_cloud_source = self.point_cloud_pose = self.point_cloud_spec = None
        self.point_cloud_sampling = None   # {"mode": "stride" | "fps", "pool": Q or 0} with a cloud
        self.point_cloud_crop = None       # {"lo": (x, y, z), "hi": (x, y, z)}, the float32 values in use, with a cloud inside a crop box
        if point_cloud is not None:   # (behind look, wrist camera and planes; before or after the stack)
            try:
                if cloud_crop is None:
                    check(self.L.lcr_enable_point_cloud_sampled(self.handle, ctypes.byref(point_cloud), ctypes.byref(cloud_sampling)))   # (stride: lcr_enable_point_cloud)
                else:
                    check(self.L.lcr_enable_point_cloud_cropped(self.handle, ctypes.byref(point_cloud), ctypes.byref(cloud_sampling), ctypes.byref(cloud_crop)))
                cv = _capi.LcrPointCloudView()
                check(self.L.lcr_get_point_cloud(self.handle, ctypes.byref(cv)))
                check(self.L.lcr_get_point_cloud_sampling(self.handle, ctypes.byref(cloud_sampling)))
                crop_on, crop_got = ctypes.c_int32(0), _capi.PointCloudCrop()
                check(self.L.lcr_get_point_cloud_crop(self.handle, ctypes.byref(crop_on), ctypes.byref(crop_got)))
            except Exception:
                self.close()
                raise
            self.point_cloud_spec = cv.spec.as_dict()
            self.point_cloud_sampling = cloud_sampling.as_dict()
            self.point_cloud_crop = crop_got.as_dict() if crop_on.value else None
            P = int(cv.spec.points)
            self.point_cloud = DeviceArray(self, cv.points, (N, P, int(cv.channels)), np.float32)
            self.point_cloud_count = DeviceArray(self, cv.count, (N,), np.int32)
            self.point_cloud_source = DeviceArray(self, cv.source, (N, P), np.int32)
            self.point_cloud_pose = DeviceArray(self, cv.camera_pose, (int(cv.slots), 13, N), np.float32)
        # the voxel grid: (N, C, Dz, Dy, Dx) of its element type, the input of a Conv3d as it stands
        self.voxel_grid = self.voxel_grid_source = self.voxel_grid_count = self.voxel_grid_occupied = self.voxel_grid_pose = self.voxel_grid_spec = None
        if voxel_grid is not None:   # (behind look, wrist camera and planes; independent of the stack and the cloud)
            try:
                check(self.L.lcr_enable_voxel_grid(self.handle, ctypes.byref(voxel_grid)))
                vv = _capi.LcrVoxelGridView()
                check(self.L.lcr_get_voxel_grid(self.handle, ctypes.byref(vv)))
            except Exception:
                self.close()
                raise
            # (lo, hi and inv_cell: the float32 values in use -- inv_cell is what the kernel multiplies with, the authority for which cell a point falls in)
            self.voxel_grid_spec = dict(vv.spec.as_dict(), inv_cell=tuple(float(x) for x in vv.inv_cell))
            Dx, Dy, Dz = self.voxel_grid_spec["dims"]
            self.voxel_grid = DeviceArray(self, vv.voxels, (N, int(vv.channels), Dz, Dy, Dx), np.dtype(self.voxel_grid_spec["dtype"]))
            self.voxel_grid_source = DeviceArray(self, vv.source, (N, Dz, Dy, Dx), np.int32) if vv.source else None
            self.voxel_grid_count = DeviceArray(self, vv.count, (N,), np.int32)
            self.voxel_grid_occupied = DeviceArray(self, vv.occupied, (N,), np.int32)
            self.voxel_grid_pose = DeviceArray(self, vv.camera_pose, (int(vv.slots), 13, N), np.float32)
        # the heightmap: (N, C, Hy, Hx) float32, the input of a Conv2d as it stands
        self.heightmap = self.heightmap_source = self.heightmap_count = self.heightmap_filled = self.heightmap_pose = self.heightmap_spec = None
        if heightmap is not None:   # (behind look, wrist camera and planes; independent of the stack, the cloud and the grid)
            try:
                check(self.L.lcr_enable_heightmap(self.handle, ctypes.byref(heightmap)))
                hv = _capi.LcrHeightmapView()
                check(self.L.lcr_get_heightmap(self.handle, ctypes.byref(hv)))
            except Exception:
                self.close()
                raise
            # (lo, hi and inv_cell: the float32 values in use -- inv_cell is what the kernel multiplies with, the authority for which cell a point falls in)
            self.heightmap_spec = dict(hv.spec.as_dict(), inv_cell=tuple(float(x) for x in hv.inv_cell))
            Hx, Hy = self.heightmap_spec["dims"]
            self.heightmap = DeviceArray(self, hv.heightmap, (N, int(hv.channels), Hy, Hx), np.float32)
            self.heightmap_source = DeviceArray(self, hv.source, (N, Hy, Hx), np.int32) if hv.source else None
            self.heightmap_count = DeviceArray(self, hv.count, (N,), np.int32)
            self.heightmap_filled = DeviceArray(self, hv.filled, (N,), np.int32)
            self.heightmap_pose = DeviceArray(self, hv.camera_pose, (int(hv.slots), 13, N), np.float32)
        # the object boxes: (N, S, O, 8) int32, a record of _capi.BOXES_FIELDS per env, camera slot and object
        self.object_boxes = self.object_boxes_spec = None
        if object_boxes is not None:   # (behind look, wrist camera and planes; independent of the stack, the cloud, the grid and the map)
            try:
                check(self.L.lcr_enable_object_boxes(self.handle, ctypes.byref(object_boxes)))
                bv = _capi.LcrObjectBoxesView()
                check(self.L.lcr_get_object_boxes(self.handle, ctypes.byref(bv)))
            except Exception:
                self.close()
                raise
            self.object_boxes_spec = object_boxes.as_dict()
            self.object_boxes = DeviceArray(self, bv.boxes, (N, int(bv.slots), int(bv.spec.n_objects), 8), np.int32)
        # the surface normals: (N, H, W, 4) int8 per selected camera -- rint(127 n) and the face code --, the nine boxes and the camera poses the kernel used.  A handle
        # without them has none of these attributes
        if surface_normals is not None:   # (behind look, wrist camera and planes; independent of every other observation unit)
            try:
                check(self.L.lcr_enable_normals(self.handle, ctypes.byref(surface_normals)))
                nv = _capi.LcrNormalsView()
                check(self.L.lcr_get_normals(self.handle, ctypes.byref(nv)))
            except Exception:
                self.close()
                raise
            self.normals_spec = nv.spec.as_dict()
            for cam in self.normals_spec["cameras"]:
                setattr(self, "normals_" + cam, DeviceArray(self, getattr(nv, "normals_" + cam), (N, int(nv.image_height), int(nv.image_width), 4), np.int8))
            self.normals_boxes = DeviceArray(self, nv.boxes, (_capi.NORMALS_BOXES, _capi.NORMALS_BOX_FLOATS, N), np.float32)
            self.normals_pose = DeviceArray(self, nv.camera_pose, (int(nv.slots), 13, N), np.float32)
        # the motion vectors: (N, H, W, 2) float16 per selected camera -- current minus previous pixel position --, valid, and the boxes and camera poses the kernel used,
        # [0] now and [1] before.  A handle without them has none of these attributes
        if motion_vectors is not None:   # (behind look, wrist camera and planes; independent of every other observation unit; the last launch behind the frames)
            try:
                check(self.L.lcr_enable_motion_vectors(self.handle, ctypes.byref(motion_vectors)))
                mv = _capi.LcrMotionView()
                check(self.L.lcr_get_motion_vectors(self.handle, ctypes.byref(mv)))
            except Exception:
                self.close()
                raise
            self.flow_spec = mv.spec.as_dict()
            for cam in self.flow_spec["cameras"]:
                setattr(self, "flow_" + cam, DeviceArray(self, getattr(mv, "flow_" + cam), (N, int(mv.image_height), int(mv.image_width), 2), np.float16))
            self.flow_valid = DeviceArray(self, mv.valid, (N,), np.uint8)
            self.flow_boxes = DeviceArray(self, mv.boxes, (2, _capi.NORMALS_BOXES, _capi.NORMALS_BOX_FLOATS, N), np.float32)
            self.flow_pose = DeviceArray(self, mv.camera_pose, (2, int(mv.slots), 13, N), np.float32)
        self.reward = DeviceArray(self, out.reward, (N,), np.float32)
        self.terminated = DeviceArray(self, out.terminated, (N,), np.uint8)
        self.truncated = DeviceArray(self, out.truncated, (N,), np.uint8)
        self.is_success = DeviceArray(self, out.is_success, (N,), np.uint8)
        self.did_reset = DeviceArray(self, out.did_reset, (N,), np.uint8)
        self.terminal_obs = DeviceArray(self, out.terminal_obs, (18, N), np.float32)
        self.terminal_quat = DeviceArray(self, out.terminal_quat, (8, N), np.float32)
        self.timestamp = DeviceArray(self, out.timestamp, (N,), np.float64)
        self.current_goal = DeviceArray(self, out.current_goal, (N,), np.int32)
        self.active_mask = DeviceArray(self, out.active_mask, (N,), np.uint32) if out.active_mask else None
        self.active_count = DeviceArray(self, out.active_count, (N,), np.uint32) if out.active_count else None
        self.max_sweeps = DeviceArray(self, out.max_sweeps, (N,), np.uint32) if out.max_sweeps else None
        self.choice = DeviceArray(self, out.choice, (N,), np.uint32) if out.choice else None
        self.ctrl = DeviceArray(self, out.ctrl, (6, N), np.float32) if out.ctrl else None

    # ---- lifecycle ----
    def close(self):
        if getattr(self, "handle", None):
            if getattr(self, "_calib_dst", None) is not None:
                self.L.lcr_free(self.handle, self._calib_dst)
                self._calib_dst = None
            self.L.lcr_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        check(self.L.lcr_set_stream(self.handle, ctypes.c_void_p(int(stream_ptr) if stream_ptr else 0)))

    def sync(self):
        check(self.L.lcr_sync(self.handle))

    def wait_frames(self):
        """make the handle's stream wait -- an event wait on the device, the host goes on -- for whatever the last step is still drawing on the second stream (frames, planes,
        wrist frames, stack, point cloud, voxel grid, heightmap, object boxes, surface normals, motion vectors): what is enqueued on the handle's stream afterwards reads the observations of that step (lcr_get_obs, a joining call)"""
        check(self.L.lcr_get_obs(self.handle, ctypes.byref(LcrObsView())))

    # ---- reset / step ----
    def reset(self, seeds=None, mask=None):
        s = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if s is not None and s.shape != (self.n,):
            raise ValueError("seeds must have shape (n_envs,)")
        if m is not None and m.shape != (self.n,):
            raise ValueError("mask must have shape (n_envs,)")
        check(self.L.lcr_reset(self.handle, _vp(m), _vp(s)))

    def step_device(self, action_ptr):
        """action_ptr: device pointer to float32 [k][N] (e.g. tensor.data_ptr())."""
        check(self.L.lcr_step(self.handle, ctypes.c_void_p(int(action_ptr))))

    def step(self, action):
        """action: host array, shape (N, k) (env-major, as a VecEnv passes it) -> transposed to [k][N]."""
        a = np.asarray(action, np.float32)
        if a.shape != (self.n, self.action_dim):
            raise ValueError("Action dimension mismatch")  # reach_cube_env.py:231-232
        at = np.ascontiguousarray(a.T)
        check(self.L.lcr_step_host(self.handle, _vp(at)))

    # ---- device helpers ----
    def alloc_actions(self):
        p = ctypes.c_void_p()
        check(self.L.lcr_malloc(self.handle, 4 * self.action_dim * self.n, ctypes.byref(p)))
        return DeviceArray(self, p.value, (self.action_dim, self.n), np.float32, readonly=False)

    def free(self, arr):
        check(self.L.lcr_free(self.handle, ctypes.c_void_p(arr.ptr)))

    def fill_random_actions(self, arr, seed, step):
        check(self.L.lcr_fill_random_actions(self.handle, ctypes.c_void_p(arr.ptr), int(seed), int(step)))

    def render(self, env=0, camera="camera_vizu", width=640, height=640):
        """ray-cast one env: camera_front / camera_top / camera_vizu (camera_wrist on a sim that has one) -> (height, width, 3) uint8"""
        cam = CAMERAS[camera]
        out = np.empty((height, width, 3), np.uint8)
        check(self.L.lcr_render(self.handle, int(env), cam, int(width), int(height), _vp(out)))
        return out

    def render_state(self, qpos, target=None, camera="camera_front", width=320, height=240):
        """ray-cast an arbitrary pose (qpos of length nq as env.data.qpos; target_pos or None) without touching the sim state"""
        cam = CAMERAS[camera]
        q = np.ascontiguousarray(qpos, np.float64)
        if q.shape != (self.nq,):
            raise ValueError(f"qpos must have shape ({self.nq},)")
        t = None if target is None else np.ascontiguousarray(target, np.float32)
        out = np.empty((height, width, 3), np.uint8)
        check(self.L.lcr_render_state(self.handle, cam, int(width), int(height), _vp(q), _vp(t), _vp(out)))
        return out

    def _finished_ids(self, name, env_ids):
        """env_ids as the int32 array the render_terminal* call `name` hands to the library, checked against that call's precondition"""
        ids = np.ascontiguousarray(env_ids, np.int32)
        if ids.size and self.image_front is not None and ids.min() >= 0 and ids.max() < self.n and not self.did_reset.numpy()[ids].all():   # (lcr.h: the terminal poses belong to envs the LAST step reset; anything else is a stale frame)
            raise ValueError(f"{name}: every listed env must have finished an episode in the last step (did_reset)")
        return ids

    def render_terminal(self, env_ids):
        """last frames (camera_front, camera_top) of the episodes the last step ended in the listed envs, ray-cast as ONE batch from their
        terminal poses (the envs themselves have already been reset): two (len(env_ids), H, W, 3) uint8 arrays, (H, W) = self.image_size"""
        ids = self._finished_ids("render_terminal", env_ids)
        front = np.empty((ids.size,) + self.image_size + (3,), np.uint8)
        top = np.empty_like(front)
        check(self.L.lcr_render_terminal(self.handle, _vp(ids), int(ids.size), _vp(front), _vp(top)))
        return front, top

    def render_terminal_wrist(self, env_ids):
        """the last wrist frames of the episodes the last step ended in the listed envs, one batch (the sibling of render_terminal(), same precondition): a dict with the
        keys of observations() -- image_wrist (len(env_ids), H, W, 3) uint8 and, with image_planes, depth_wrist float32 / segmentation_wrist uint8 (len(env_ids), H, W)"""
        if self.wrist_camera is None:
            raise ValueError("render_terminal_wrist: no wrist_camera is enabled")
        ids = self._finished_ids("render_terminal_wrist", env_ids)
        shape = (ids.size,) + self.image_size
        rgb = np.empty(shape + (3,), np.uint8)
        d = np.empty(shape, np.float32) if self.depth_wrist is not None else None
        s = np.empty(shape, np.uint8) if self.seg_wrist is not None else None
        check(self.L.lcr_render_terminal_wrist(self.handle, _vp(ids), int(ids.size), _vp(rgb), _vp(d), _vp(s)))
        out = {"image_wrist": rgb}
        if d is not None:
            out["depth_wrist"] = d
        if s is not None:
            out["segmentation_wrist"] = s
        return out

    def obs_stack_terminal(self, env_ids):
        """the observation stacks of the episodes the last step ended in the listed envs (the sibling of render_terminal(), same precondition): (len(env_ids), K, C, H, W)
        of the stack's element type -- the K - 1 frames the env's stack held before the step refilled it, then the terminal frames.  Needs obs_stack=dict(..., terminal=True)"""
        if self.obs_stack is None:
            raise ValueError("obs_stack_terminal: no obs_stack is enabled")
        if not self.obs_stack_keeps_terminal:
            raise ValueError("obs_stack_terminal: the obs_stack was enabled without terminal=True, so the history of an episode that ends is not kept")
        ids = self._finished_ids("obs_stack_terminal", env_ids)
        out = np.empty((ids.size,) + self.obs_stack.shape[1:], self.obs_stack.dtype)
        check(self.L.lcr_obs_stack_terminal(self.handle, _vp(ids), int(ids.size), _vp(out)))
        return out

    def point_cloud_terminal(self, env_ids):
        """the point clouds of the last observations of the episodes the last step ended in the listed envs (the sibling of render_terminal(), same precondition), made by
        the sim's own cloud kernel from the terminal frames, planes, looks and poses: {"point_cloud": (len(env_ids), P, C) float32, "count": (len(env_ids),) int32,
        "source": (len(env_ids), P) int32, "pose": (slots, 13, len(env_ids)) float32}.  Works on any sim with a point_cloud"""
        if self.point_cloud is None:
            raise ValueError("point_cloud_terminal: no point_cloud is enabled")
        ids = self._finished_ids("point_cloud_terminal", env_ids)
        n = ids.size
        out = {"point_cloud": np.empty((n,) + self.point_cloud.shape[1:], np.float32), "count": np.empty(n, np.int32),
               "source": np.empty((n,) + self.point_cloud_source.shape[1:], np.int32), "pose": np.empty(self.point_cloud_pose.shape[:2] + (n,), np.float32)}
        check(self.L.lcr_point_cloud_terminal(self.handle, _vp(ids), int(n), _vp(out["point_cloud"]), _vp(out["count"]), _vp(out["source"]), _vp(out["pose"])))
        return out

    def look(self):
        """the looks of the envs (lcr_get_look): {"variants": the handle's list of LookVariant, "variant": (N,) int32, "rgb": (9, N) float32 -- cube, second cube, marker --,
        "episode": (N,) uint32 resets of each env so far}.  `set_look(variant=, rgb=)` of it restores the looks."""
        if self.look_variants is None:
            raise ValueError("look: no look is enabled (look_variants)")
        variant, rgb, episode = np.zeros(self.n, np.int32), np.zeros((9, self.n), np.float32), np.zeros(self.n, np.uint32)
        check(self.L.lcr_get_look(self.handle, _vp(variant), _vp(rgb), _vp(episode)))
        return {"variants": list(self.look_variants), "variant": variant, "rgb": rgb, "episode": episode}

    def set_look(self, variant=None, rgb=None, mask=None):
        """give the masked envs (None: all) a variant index and / or colours ((9, N): cube, second cube, marker rgb) and redraw the frames (lcr_set_look)"""
        v = None if variant is None else np.ascontiguousarray(variant, np.int32)
        c = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if v is not None and v.shape != (self.n,):
            raise ValueError("variant must have shape (n_envs,)")
        if c is not None and c.shape != (9, self.n):
            raise ValueError("rgb must have shape (9, n_envs)")
        if m is not None and m.shape != (self.n,):
            raise ValueError("mask must have shape (n_envs,)")
        check(self.L.lcr_set_look(self.handle, _vp(m), _vp(v), _vp(c)))

    def render_planes(self, env=0, camera="camera_front", width=320, height=240):
        """depth and segmentation of one env, one ray per pixel (the sibling of render()): ((height, width) float32 metres along the optical axis, clipped at
        depth_far; (height, width) uint8 ids, see include/lcr.h).  Works with or without image_planes."""
        depth, seg = np.empty((height, width), np.float32), np.empty((height, width), np.uint8)
        check(self.L.lcr_render_planes(self.handle, int(env), CAMERAS[camera], int(width), int(height), _vp(depth), _vp(seg)))
        return depth, seg

    def render_state_planes(self, qpos, target=None, camera="camera_front", width=320, height=240):
        """depth and segmentation of an arbitrary pose (the sibling of render_state()); the far clip is depth_far when image_planes are enabled, else 10 m"""
        q = np.ascontiguousarray(qpos, np.float64)
        if q.shape != (self.nq,):
            raise ValueError(f"qpos must have shape ({self.nq},)")
        t = None if target is None else np.ascontiguousarray(target, np.float32)
        depth, seg = np.empty((height, width), np.float32), np.empty((height, width), np.uint8)
        check(self.L.lcr_render_state_planes(self.handle, CAMERAS[camera], int(width), int(height), _vp(q), _vp(t), _vp(depth), _vp(seg)))
        return depth, seg

    def render_terminal_planes(self, env_ids):
        """the enabled planes of the last frames of the episodes the last step ended in the listed envs, one batch (the sibling of render_terminal(), same precondition):
        a dict with the keys of observations() -- depth_front, depth_top (len(env_ids), H, W) float32 / segmentation_front, segmentation_top uint8"""
        if not self.image_planes:
            raise ValueError("render_terminal_planes: no image_planes are enabled")
        ids = self._finished_ids("render_terminal_planes", env_ids)
        shape = (ids.size,) + self.image_size
        d = "depth" in self.image_planes
        s = "segmentation" in self.image_planes
        df, dtp = (np.empty(shape, np.float32), np.empty(shape, np.float32)) if d else (None, None)
        sf, stp = (np.empty(shape, np.uint8), np.empty(shape, np.uint8)) if s else (None, None)
        check(self.L.lcr_render_terminal_planes(self.handle, _vp(ids), int(ids.size), _vp(df), _vp(dtp), _vp(sf), _vp(stp)))
        out = {}
        if d:
            out["depth_front"], out["depth_top"] = df, dtp
        if s:
            out["segmentation_front"], out["segmentation_top"] = sf, stp
        return out

    def plane_arrays(self):
        """the enabled planes as {observation key: DeviceArray}, in the key order of observations()"""
        out = {}
        if self.depth_front is not None:
            out["depth_front"], out["depth_top"] = self.depth_front, self.depth_top
        if self.seg_front is not None:
            out["segmentation_front"], out["segmentation_top"] = self.seg_front, self.seg_top
        if self.depth_wrist is not None:   # (behind the four keys of the two scene cameras, which keep their places)
            out["depth_wrist"] = self.depth_wrist
        if self.seg_wrist is not None:
            out["segmentation_wrist"] = self.seg_wrist
        return out

    def read_rows(self, arr, rows):
        """host copies of selected leading-axis rows of a device array (e.g. the frames of a few recorded envs): one small
        device-to-host copy per row instead of the whole array"""
        rows = list(rows)
        row_shape = arr.shape[1:]
        nb = int(np.prod(row_shape)) * arr.dtype.itemsize
        out = np.empty((len(rows),) + row_shape, arr.dtype)
        for i, r in enumerate(rows):
            check(self.L.lcr_memcpy_d2h(self.handle, _vp(out[i:i + 1]), ctypes.c_void_p(arr.ptr + int(r) * nb), nb))   # (a slice: out[i] of an (N,) array is a scalar, not a view)
        return out

    def calibrate_copy(self, n_floats):
        """launch the known-byte-count copy kernel once (profiling calibration); returns bytes read == bytes written"""
        if getattr(self, "_calib_dst", None) is None or self._calib_n < n_floats:
            if getattr(self, "_calib_dst", None) is not None:
                check(self.L.lcr_free(self.handle, self._calib_dst))
                self._calib_dst = None
            p = ctypes.c_void_p()
            check(self.L.lcr_malloc(self.handle, 4 * n_floats, ctypes.byref(p)))
            self._calib_dst, self._calib_n = p, n_floats
        check(self.L.lcr_calibrate_copy(self.handle, self._calib_dst, n_floats))
        return 4 * n_floats

    def timer_begin(self):
        check(self.L.lcr_timer_begin(self.handle))

    def timer_end(self):
        ms = ctypes.c_float()
        check(self.L.lcr_timer_end(self.handle, ctypes.byref(ms)))
        return ms.value

    # ---- host-side views ----
    def observations(self):
        """dict of (N, .) float32 numpy arrays with the reference's keys (get_observation reach:281-295)."""
        obs = {"arm_qpos": self.arm_qpos.numpy().T.copy(), "arm_qvel": self.arm_qvel.numpy().T.copy()}
        # (insertion order of the reference's get_observation: target_pos, images, cube position(s) -- push_cube_env.py:293-306)
        if self.task_name in ("push", "pick_place"):
            obs["target_pos"] = self.aux_pos.numpy().T.copy()  # always present (push_cube_env.py:297)
        if self.image_front is not None:
            obs["image_front"] = self.image_front.numpy()
            obs["image_top"] = self.image_top.numpy()
            if self.image_wrist is not None:
                obs["image_wrist"] = self.image_wrist.numpy()
            for k, a in self.plane_arrays().items():
                obs[k] = a.numpy()
            if self.obs_stack is not None:
                obs["image_stack"] = self.obs_stack.numpy()
            if self.point_cloud is not None:
                obs["point_cloud"] = self.point_cloud.numpy()
            if self.voxel_grid is not None:
                obs["voxel_grid"] = self.voxel_grid.numpy()
            if self.heightmap is not None:
                obs["heightmap"] = self.heightmap.numpy()
            if self.object_boxes is not None:
                obs["object_boxes"] = self.object_boxes.numpy()
            for cam in getattr(self, "normals_spec", {"cameras": ()})["cameras"]:
                obs["normals_" + cam] = getattr(self, "normals_" + cam).numpy()
            for cam in getattr(self, "flow_spec", {"cameras": ()})["cameras"]:
                obs["flow_" + cam] = getattr(self, "flow_" + cam).numpy()
        if OBS_MODES["state"] == self.cfg.obs_mode or OBS_MODES["both"] == self.cfg.obs_mode:
            obs[self.cube_name] = self.cube_pos.numpy().T.copy()
            if self.task_name == "stack":
                obs["cube_blue_pos"] = self.aux_pos.numpy().T.copy()
        return obs

    def fetch_host(self):
        """State observations, rewards and flags of all envs after ONE device-to-host copy into pinned memory (lcr_fetch_host).
        Returns a dict of numpy VIEWS (no further copy) valid until the next call: observations as (N, .) float32 (strided),
        reward (N,) float32, terminated / truncated / is_success / did_reset (N,) bool, terminal_obs (N, 18) or None."""
        hv = LcrHostView()
        check(self.L.lcr_fetch_host(self.handle, ctypes.byref(hv)))
        N = self.n

        def view(ptr, rows, dt):
            if not ptr:
                return None
            cnt = rows * N
            buf = (ctypes.c_char * (cnt * np.dtype(dt).itemsize)).from_address(ptr)
            a = np.frombuffer(buf, dt, cnt)
            return a.reshape(rows, N).T if rows > 1 else a

        out = {
            "arm_qpos": view(hv.arm_qpos, 6, np.float32), "arm_qvel": view(hv.arm_qvel, 6, np.float32),
            "cube_pos": view(hv.cube_pos, 3, np.float32), "aux_pos": view(hv.aux_pos, 3, np.float32),
            "reward": view(hv.reward, 1, np.float32),
            "terminated": view(hv.terminated, 1, np.bool_), "truncated": view(hv.truncated, 1, np.bool_),
            "is_success": view(hv.is_success, 1, np.bool_), "did_reset": view(hv.did_reset, 1, np.bool_),
            "terminal_obs": view(hv.terminal_obs, 18, np.float32) if hv.any_reset else None,
        }
        return out

    def outputs(self):
        return {
            "reward": self.reward.numpy(),
            "terminated": self.terminated.numpy().astype(bool),
            "truncated": self.truncated.numpy().astype(bool),
            "is_success": self.is_success.numpy().astype(bool),
            "did_reset": self.did_reset.numpy().astype(bool),
        }

    def redo_flags(self):
        """Debug accessor: per 64-env wave, whether the LAST step repeated its control step in the second launch of the one-cube Newton kernels' pair
        (lcr_get_redo_flags); None for a handle whose step kernel keeps no such flags.  `redo_paired` says whether the pair runs (LCR_REDO_KERNEL=0: not)."""
        n_waves, paired = ctypes.c_int32(0), ctypes.c_int32(0)
        check(self.L.lcr_get_redo_flags(self.handle, None, 0, ctypes.byref(n_waves), ctypes.byref(paired)))
        self.redo_paired = bool(paired.value)
        if n_waves.value == 0:
            return None
        flags = np.zeros(n_waves.value, np.int32)
        check(self.L.lcr_get_redo_flags(self.handle, _vp(flags), n_waves.value, None, None))
        return flags.astype(bool)

    def get_state(self):
        N = self.n
        st = {
            "qpos": np.zeros((self.nq, N)), "qvel": np.zeros((self.nv, N)), "ee_lag": np.zeros((3, N)),
            "target": np.zeros((3, N), np.float32), "elapsed": np.zeros(N, np.int32), "rng": np.zeros((4, N), np.uint64),
            "current_goal": np.zeros(N, np.int32), "sim_time": np.zeros(N),
            "warm": np.zeros((_capi.NWARM, N), np.float32),   # carried constraint forces (mjData.qacc_warmstart of the reference's sim)
        }
        check(self.L.lcr_get_state(self.handle, _vp(st["qpos"]), _vp(st["qvel"]), _vp(st["ee_lag"]), _vp(st["target"]),
                                   _vp(st["elapsed"]), _vp(st["rng"]), _vp(st["current_goal"]), _vp(st["sim_time"]), _vp(st["warm"])))
        return st

    def set_state(self, qpos=None, qvel=None, ee_lag=None, target=None, elapsed=None, rng=None, current_goal=None, sim_time=None, warm=None):
        """Overwrite (parts of) the simulator state.  `set_state(**get_state())` is an exact checkpoint restore.  Setting qpos or qvel
        WITHOUT `warm` drops the carried constraint forces: the next step then starts from a cold solve."""
        N = self.n

        def prep(a, shape, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            if a.shape != shape:
                raise ValueError(f"bad state shape {a.shape}, want {shape}")
            return a

        qpos, qvel = prep(qpos, (self.nq, N), np.float64), prep(qvel, (self.nv, N), np.float64)
        ee_lag, target = prep(ee_lag, (3, N), np.float64), prep(target, (3, N), np.float32)
        elapsed, rng = prep(elapsed, (N,), np.int32), prep(rng, (4, N), np.uint64)
        current_goal, sim_time = prep(current_goal, (N,), np.int32), prep(sim_time, (N,), np.float64)
        warm = prep(warm, (_capi.NWARM, N), np.float32)
        check(self.L.lcr_set_state(self.handle, _vp(qpos), _vp(qvel), _vp(ee_lag), _vp(target), _vp(elapsed), _vp(rng),
                                   _vp(current_goal), _vp(sim_time), _vp(warm)))
