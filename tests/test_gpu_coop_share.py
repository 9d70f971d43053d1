"""The one-cube Newton kernel's queue of cooperative solves (lcr_kernels.hip: CoopQueue): which wave of a workgroup solves a coupled env must not show in
the results.  Owner-only, shared (the default) and always-hand-off give the same bits on the four one-cube tasks over 64 control steps with auto-resets;
shards of multiples of 64 envs that are not multiples of 256 (so a workgroup holds 1-3 real waves) match the job run as one shard; two runs match."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASKS = [("reach", "joint"), ("push", "joint"), ("lift", "joint"), ("pick_place", "ee")]
STEPS = 64


def _run(task, mode, n, steps=STEPS, **kw):
    from gym_lowcostrobot_amd import VecSim
    sim = VecSim(task, n, observation_mode="state", action_mode=mode, base_seed=5, **kw)
    buf = sim.alloc_actions()
    for t in range(steps):
        sim.fill_random_actions(buf, 0, t)
        sim.step_device(buf.ptr)
    st = sim.get_state()
    out = {k: np.array(st[k]) for k in ("qpos", "qvel", "elapsed", "rng", "ee_lag", "warm") if k in st}
    out["reward"] = sim.reward.numpy().copy()
    sim.close()
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("task,mode", TASKS)
def test_share_modes_bit_identical(hip_lib, task, mode):
    n = 8192
    ref = _run(task, mode, n, coop_share="owner")
    assert np.isfinite(ref["qpos"]).all() and np.isfinite(ref["qvel"]).all()
    for share in ("shared", "handoff", None):
        got = _run(task, mode, n, coop_share=share)
        _same(ref, got, f"{task} owner-only vs {share}")
    assert (ref["elapsed"] < STEPS).any(), "no env was auto-reset within the run"


@pytest.mark.parametrize("task,mode", TASKS)
def test_shards_not_multiple_of_256(hip_lib, task, mode):
    from gym_lowcostrobot_amd import VecSim
    cuts = [0, 1088, 1088 + 2112, 1088 + 2112 + 960]   # 17, 33 and 15 waves: every shard ends with a workgroup of 1-3 real waves
    n = cuts[-1]
    kw = dict(observation_mode="state", action_mode=mode, base_seed=9)
    whole = VecSim(task, n, **kw)
    parts = [VecSim(task, b - a, env_id_offset=a, global_envs=n, **kw) for a, b in zip(cuts[:-1], cuts[1:])]
    bw = whole.alloc_actions()
    bp = [p.alloc_actions() for p in parts]
    for t in range(STEPS):
        whole.fill_random_actions(bw, 0, t)
        whole.step_device(bw.ptr)
        for p, b in zip(parts, bp):
            p.fill_random_actions(b, 0, t)
            p.step_device(b.ptr)
    sw = whole.get_state()
    sp = [p.get_state() for p in parts]
    for k in ("qpos", "qvel", "elapsed", "rng", "ee_lag"):
        np.testing.assert_array_equal(sw[k], np.concatenate([s[k] for s in sp], axis=-1), err_msg=k)
    np.testing.assert_array_equal(whole.reward.numpy(), np.concatenate([p.reward.numpy() for p in parts]))
    for s in [whole] + parts:
        s.close()


@pytest.mark.parametrize("task,mode", [("reach", "joint"), ("pick_place", "ee")])
def test_two_runs_identical(hip_lib, task, mode):
    a = _run(task, mode, 4160)
    b = _run(task, mode, 4160)
    _same(a, b, f"{task} run 1 vs run 2")
