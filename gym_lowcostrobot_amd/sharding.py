"""Multi-GPU = independent env shards, one process per GPU, no data-path collective.

GPU/rank g of G owns the contiguous global env ids [g*n, (g+1)*n) (weak scaling: n per GPU is fixed).  RNG
streams and the synthetic policy are keyed on the GLOBAL env id, so any sharding yields the same trajectories.
The only communication is the timing protocol of the benchmark: a barrier on both sides of the timed region
and a MAX-reduction of the elapsed time (works on the "nccl"(=RCCL) backend with GPU tensors and on "gloo"
with CPU tensors, which is how the CPU tests cover it).
"""
import time


def shard_offset(envs_per_rank, rank):
    """global id of this rank's env 0"""
    return int(rank) * int(envs_per_rank)


def shard_range(envs_per_rank, rank):
    o = shard_offset(envs_per_rank, rank)
    return o, o + int(envs_per_rank)


def timed_region(run_steps, steps, *, dist=None, device_sync=None, tensor_device="cpu"):
    """Time exactly `steps` calls of run_steps(i) bracketed by barrier + device sync on both sides.
    Returns (max elapsed seconds over ranks, this rank's elapsed seconds)."""
    def sync_all():
        if dist is not None:
            dist.barrier()
        if device_sync is not None:
            device_sync()

    sync_all()
    t0 = time.perf_counter()
    for i in range(steps):
        run_steps(i)
    sync_all()
    local = time.perf_counter() - t0
    worst = local
    if dist is not None:
        import torch

        t = torch.tensor([local], dtype=torch.float64, device=tensor_device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        worst = float(t.item())
    return worst, local


def aggregate_throughput(envs_per_rank, world, steps, worst_seconds):
    """whole-job env-steps/s: units all ranks processed / max-over-ranks time"""
    return int(envs_per_rank) * int(world) * int(steps) / worst_seconds


class ShardedVecSim:
    """Single-process convenience over several GPUs: one VecSim (one C-ABI handle, one HIP stream) per device, contiguous
    global env-id ranges, launches enqueued on every device before anything is synchronised.  No collective is involved;
    results are identical to any other sharding of the same global batch."""

    def __init__(self, task, n_envs_total, devices, **kw):
        from .vecsim import VecSim

        devices = list(devices)
        if n_envs_total % len(devices):
            raise ValueError("n_envs_total must be divisible by the number of shards")
        self.per = n_envs_total // len(devices)
        self.n = n_envs_total
        # (look_variants / look_sampler too: the sampler is keyed by the global env id, so the shards draw the looks the whole job would)
        # (wrist_camera too: every shard mounts the same camera; shards[i].image_wrist ...)
        # (obs_stack too: every shard keeps the stack of its own envs, shards[i].obs_stack; an env's stack depends on that env alone)
        # (point_cloud too: every shard keeps the cloud of its own envs, shards[i].point_cloud; an env's cloud depends on that env alone.  Its crop box is in the world
        #  frame, which every env shares: every shard gets the same box, shards[i].point_cloud_crop)
        # (voxel_grid too: every shard keeps the grid of its own envs, shards[i].voxel_grid; its box is in the world frame, which every env shares: every shard gets the same spec)
        # (heightmap too: every shard keeps the map of its own envs, shards[i].heightmap; its box is in the world frame as well: every shard gets the same spec)
        # (object_boxes too: every shard keeps the records of its own envs, shards[i].object_boxes; an env's records depend on that env's planes alone: the same spec)
        # (surface_normals too: every shard keeps the planes of its own envs, shards[i].normals_front ...; an env's normals depend on that env alone: the same spec)
        # (motion_vectors too: every shard keeps the planes and the pose history of its own envs, shards[i].flow_front ...; an env's flow depends on that env alone: the same spec)
        # (terminal=True in obs_stack / point_cloud too: obs_stack_terminal() / point_cloud_terminal() below take GLOBAL env ids and ask the shard that owns each)
        # (planes=("depth",) in obs_stack too: the key goes to every shard with the dict, every shard stacks its own depth planes, and the terminal call is routed as before)
        # (image_planes / depth_far, like every other keyword, go to each shard's VecSim: the planes are per-shard device arrays, shards[i].depth_front ...)
        # every shard declares the whole job (lcr_config.global_envs): the same kernel family on every shard, and lcr_create checks that the cut is at wave boundaries
        kw.setdefault("global_envs", n_envs_total)
        self.shards = [VecSim(task, self.per, device=d, env_id_offset=shard_offset(self.per, i), **kw) for i, d in enumerate(devices)]
        self.action_dim = self.shards[0].action_dim
        self._act = [s.alloc_actions() for s in self.shards]

    def fill_random_actions(self, seed, step):
        for s, a in zip(self.shards, self._act):
            s.fill_random_actions(a, seed, step)

    def step_device(self):
        """step every shard on its own action buffer (asynchronous on every device)"""
        for s, a in zip(self.shards, self._act):
            s.step_device(a.ptr)

    def sync(self):
        for s in self.shards:
            s.sync()

    def get_state(self):
        import numpy as np

        sts = [s.get_state() for s in self.shards]
        return {k: np.concatenate([st[k] for st in sts], axis=-1) for k in sts[0]}

    def look(self):
        import numpy as np

        ls = [s.look() for s in self.shards]
        return {"variants": ls[0]["variants"], **{k: np.concatenate([l[k] for l in ls], axis=-1) for k in ("variant", "rgb", "episode")}}

    def _by_shard(self, env_ids):
        """global env ids -> per shard (positions in env_ids, local ids); an id outside the job goes to the nearest shard, whose library refuses it"""
        import numpy as np

        ids = np.ascontiguousarray(env_ids, np.int64).reshape(-1)
        owner = np.clip(ids // self.per, 0, len(self.shards) - 1)
        return ids, [(np.nonzero(owner == g)[0], (ids[owner == g] - g * self.per).astype(np.int32)) for g in range(len(self.shards))]

    def obs_stack_terminal(self, env_ids):
        """VecSim.obs_stack_terminal over the job's global env ids: every shard makes the terminal stacks of its own envs, in the order of env_ids"""
        import numpy as np

        ids, parts = self._by_shard(env_ids)
        s0 = self.shards[0]
        if s0.obs_stack is None:
            raise ValueError("obs_stack_terminal: no obs_stack is enabled")
        out = np.empty((ids.size,) + s0.obs_stack.shape[1:], s0.obs_stack.dtype)
        for s, (pos, local) in zip(self.shards, parts):
            if pos.size:
                out[pos] = s.obs_stack_terminal(local)
        return out

    def point_cloud_terminal(self, env_ids):
        """VecSim.point_cloud_terminal over the job's global env ids, in the order of env_ids (pose: (slots, 13, len(env_ids)))"""
        import numpy as np

        ids, parts = self._by_shard(env_ids)
        s0 = self.shards[0]
        if s0.point_cloud is None:
            raise ValueError("point_cloud_terminal: no point_cloud is enabled")
        n = ids.size
        out = {"point_cloud": np.empty((n,) + s0.point_cloud.shape[1:], np.float32), "count": np.empty(n, np.int32),
               "source": np.empty((n,) + s0.point_cloud_source.shape[1:], np.int32), "pose": np.empty(s0.point_cloud_pose.shape[:2] + (n,), np.float32)}
        for s, (pos, local) in zip(self.shards, parts):
            if pos.size:
                got = s.point_cloud_terminal(local)
                for k in ("point_cloud", "count", "source"):
                    out[k][pos] = got[k]
                out["pose"][:, :, pos] = got["pose"]
        return out

    def outputs(self):
        import numpy as np

        outs = [s.outputs() for s in self.shards]
        return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}

    def close(self):
        for s, a in zip(self.shards, self._act):
            s.free(a)
            s.close()
