"""The Newton solves' per-solve constants (csrc/lcr_newton.h: the joint-limit rows L^-1 (+-e_j) are computed once per solve, not in every pass of every iteration) at the
small shapes where those code paths can go wrong: 64 envs (one wave, three empty waves in its workgroup), 65 envs (a second wave with ONE real lane), 320 envs (two
workgroups, the second partly filled).  Every wave holds, in different lanes, the six kinds of KINDS below: both finger pads on the floor (arm slots 2 and 3), one
pad only, a link proxy on the floor (slot 4: four rows), one joint beyond its lower and another beyond its upper limit, a finger pair on the cube (a patient of the
cooperative solves: it sits out the arm solve) and lanes without any contact.

Checks: (1) qpos / qvel after each of five re-synchronised control steps with fixed seeded actions against the fp64 CPU oracle, preset faithful, with the tolerances and
shares tests/test_gpu_parity.py applies to the same kind of comparison; (2) two runs of the same rollout are bit-identical; (3) jobs cut into shards at wave
boundaries, one of them ending in a 65-env shard, give the bits of the job run as one, and the 65-env job gives the bits of the first 65 envs of the 320-env job
(DESIGN section 6).

The placements are selected on the CPU: a state is used only if the oracle's own fp32 build stays within a quarter of the kind's tolerance of the fp64 build over the
five steps -- the placement alone keeps the share of envs outside the tolerance at zero, the kernel's share is what the tests bound."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

KINDS = ("both_pads", "one_pad", "proxy", "limits", "finger_cube", "free")
STEPS = 5
# the kind of lane i is LANE_KIND[i % 12]: five or six lanes of a wave have their fingers on the cube -- no more than the eight coupled envs a wave of the one-cube kernels
# solves cooperatively (lcr_config.coop_max), beyond which the whole wave would take the coupled SIMT copy and no lane would sit out the arm solve
LANE_KIND = (0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 5, 5)
ACT_SCALE = 0.3          # tests/test_gpu_parity.py: test_link_proxy_contacts
N_POOL = 3072            # random arm states searched per task for the three floor-contact kinds
CASES = [("reach", "joint", 64), ("reach", "joint", 65), ("reach", "joint", 320), ("push", "joint", 64), ("push", "joint", 65), ("push", "joint", 320),
         ("pick_place", "ee", 64), ("pick_place", "ee", 65), ("pick_place", "ee", 320), ("stack", "joint", 64), ("push_loop", "joint", 64)]


def _tolerances(task, kind, n_kind):
    """(atol_q, atol_v, least share of the kind's envs within them) -- copied from tests/test_gpu_parity.py, preset faithful:
    floor contacts of the arm: test_link_proxy_contacts (4e-5, StackTwoCubes 6e-5; 4e-3; min(0.99, 1 - 1.5 / n), StackTwoCubes 0.975);
    joint limits and free flight: _cmp_step's defaults, as test_joint_limit_rows uses them (2e-5, 2e-3, 0.99);
    fingers on the cube: test_pinch_grasp_finger_cube_contacts (2e-5, 4e-3, 0.985)"""
    if kind in ("both_pads", "one_pad", "proxy"):
        return (6e-5 if task == "stack" else 4e-5), 4e-3, (0.975 if task == "stack" else min(0.99, 1.0 - 1.5 / n_kind))
    if kind == "finger_cube":
        return 2e-5, 4e-3, 0.985
    return 2e-5, 2e-3, 0.99


_PLACED = {}


def _placement(task, mode):
    """320 states, env i of kind KINDS[LANE_KIND[i % 12]], with the actions of the five steps: (qpos, qvel, actions[STEPS], kinds).  Computed once per task on the CPU."""
    if (task, mode) in _PLACED:
        return _PLACED[(task, mode)]
    from oracle import orc

    am = {"joint": 0, "ee": 1}[mode]
    rng = np.random.default_rng(808)
    per = 56
    o = orc.Oracle(task, N_POOL, preset="faithful", auto_reset=0, max_episode_steps=0, action_mode=am)
    o.reset(seeds=np.arange(N_POOL))
    kind = np.full(N_POOL, -1)
    # the three floor-contact kinds: random arm states, classified by the slots their first control step has active (oracle slot ids 12-13 finger<->cube,
    # 14-15 finger<->floor, 16 link proxies: tests/util.py)
    q, qd = util.random_arm_state(rng, N_POOL, scale_v=1.0)
    o.qpos[:, :6] = q; o.qvel[:, :6] = qd
    # ... two kinds are placed by hand in the last rows of the pool; the lanes without contact are random states again
    lim, pinch = (slice(N_POOL - (k + 1) * 4 * per, N_POOL - k * 4 * per) for k in range(2))
    m = lim.stop - lim.start                             # test_joint_limit_rows
    o.qpos[lim, :6] = rng.uniform(-0.3, 0.3, (m, 6)); o.qpos[lim, 1] = -0.8; o.qpos[lim, 2] = 0.3
    o.qvel[lim, :6] = rng.normal(0, 0.5, (m, 6))
    o.qpos[lim, 0] = -3.14 - rng.uniform(0, 0.01, m)     # beyond its lower limit
    o.qpos[lim, 5] = 0.032 + rng.uniform(0, 0.01, m)     # the gripper beyond its upper limit
    m = pinch.stop - pinch.start
    po = orc.Oracle(task, m, preset="faithful", auto_reset=0, max_episode_steps=0, action_mode=am)
    po.reset(seeds=np.arange(m))
    util.pinch_setup(po)                                 # test_pinch_grasp_finger_cube_contacts
    po.qpos[:, 6:9] += rng.normal(0, 3e-4, (m, 3)); po.qpos[:, 5] += rng.uniform(-0.02, 0.02, m); po.qvel[:, :6] = rng.normal(0, 0.1, (m, 6))
    o.qpos[pinch] = po.qpos; o.qvel[pinch] = po.qvel; o.ee_lag[pinch] = po.ee_lag
    util.sync_oracle_to_f32(o)
    q0, v0, lag0 = o.qpos.copy(), o.qvel.copy(), o.ee_lag.copy()
    # five re-synchronised steps of the fp64 build and of its fp32 twin from the same states: the slots of the first step classify, the twin's distance selects
    t = util._twin(o)
    acts = [(ACT_SCALE * rng.uniform(-1, 1, (N_POOL, o.action_dim))).astype(np.float32) for _ in range(STEPS)]
    rel = np.zeros(N_POOL)    # largest |fp32 - fp64| of the five steps, qpos in units of 1e-5, qvel in units of 1e-3
    first = None
    for a in acts:
        o.warm[:] = 0
        util.sync_oracle_to_f32(o)
        for k in ("qpos", "qvel", "ee_lag", "target", "elapsed", "rng", "goal", "sim_time"):
            getattr(t, k)[:] = getattr(o, k)
        t.warm[:] = 0
        o.step(a, threads=0); t.step(a, threads=0)
        dq = np.abs(t.qpos - o.qpos).max(axis=1); dv = np.abs(t.qvel - o.qvel).max(axis=1)
        rel = np.maximum(rel, np.maximum(dq / 1e-5, dv / 1e-3))
        rel[(t.active_count != o.active_count) | (t.choice != o.choice)] = np.inf     # a decision the two builds take differently: not a placement to test with
        if first is None:
            first = o.active_mask.copy()
    b = lambda k: ((first >> k) & 1).astype(bool)
    hand = np.zeros(N_POOL, bool)
    hand[lim.start:] = True
    on_cube = b(12) | b(13)
    kind[~hand & b(14) & b(15) & ~b(16) & ~on_cube] = 0
    kind[~hand & (b(14) ^ b(15)) & ~b(16) & ~on_cube] = 1
    kind[~hand & b(16) & ~on_cube] = 2
    kind[lim] = 3
    kind[pinch] = np.where(b(12) & b(13), 4, -1)[pinch]
    kind[~hand & ((first & 0x1F000) == 0)] = 5
    kind[rel > 0.5] = -1     # a quarter of the tightest tolerance (2e-5 rad, 2e-3 rad/s)
    picks = [list(np.nonzero(kind == k)[0]) for k in range(len(KINDS))]
    for k, p in enumerate(picks):
        assert len(p) >= 22, (task, KINDS[k], len(p))    # (two waves' worth of different states; the envs are independent, later waves may repeat them)
    kinds = np.array([LANE_KIND[i % 12] for i in range(320)])
    idx = np.array([picks[k][(i // 6) % len(picks[k])] for i, k in enumerate(kinds)])
    out = (q0[idx], v0[idx], lag0[idx], [a[idx] for a in acts], kinds)
    _PLACED[(task, mode)] = out
    return out


def _pair(task, mode, n):
    qpos, qvel, lag, acts, kinds = _placement(task, mode)
    sim, o = util.make_pair(task, n, preset="faithful", auto_reset=False, max_episode_steps=0, action_mode=mode)
    o.reset(seeds=np.arange(n)); sim.reset(seeds=np.arange(n))
    o.qpos[:] = qpos[:n]; o.qvel[:] = qvel[:n]; o.ee_lag[:] = lag[:n]
    return sim, o, [a[:n] for a in acts], kinds[:n]


@pytest.mark.parametrize("task,mode,n", CASES)
def test_mixed_waves_against_the_oracle(hip_lib, task, mode, n):
    sim, o, acts, kinds = _pair(task, mode, n)
    loose_q = 6e-5 if task == "stack" else 4e-5
    seen = np.zeros(len(KINDS), int)
    for t, a in enumerate(acts):
        # every env outside the loosest tolerance has to be explained inside parity_step (max_dq: test_link_proxy_contacts); the kinds' own tolerances follow
        dq, dv, ok, st = util.parity_step(sim, o, a, loose_q, 4e-3, max_dq=3e-2, where=("newton_consts", task, n, t), carry=False)
        if t == 0:
            m = o.active_mask
            for k, bits in enumerate(((14, 15), (), (16,), (), (12, 13), ())):
                seen[k] = sum(int((((m >> b) & 1) == 1)[kinds == k].sum()) for b in bits)
            one = (((m >> 14) & 1) ^ ((m >> 15) & 1))[kinds == 1]
            assert one.all() and seen[0] == 2 * (kinds == 0).sum() and seen[2] == (kinds == 2).sum() and seen[4] == 2 * (kinds == 4).sum(), (seen, one)
        if t in (0, STEPS - 1):
            for k, name in enumerate(KINDS):
                sel = kinds == k
                tq, tv, share = _tolerances(task, name, int(sel.sum()))
                within = (dq[sel] <= tq) & (dv[sel] <= tv)
                print(f"[newton_consts] {task} n={n} step {t + 1} {name}: {int(sel.sum())} envs, max |dq| {dq[sel].max():.2e} |dv| {dv[sel].max():.2e}, within {within.mean():.3f}")
                assert within.mean() >= share, (task, n, t, name, np.sort(dq[sel])[-3:], np.sort(dv[sel])[-3:])
    sim.close()


def _rollout(task, mode, n, **kw):
    from gym_lowcostrobot_amd import VecSim

    qpos, qvel, lag, acts, _ = _placement(task, mode)
    sim = VecSim(task, n, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, **kw)
    off = kw.get("env_id_offset", 0)
    sim.reset(seeds=np.arange(off, off + n, dtype=np.uint64))
    sl = slice(off, off + n)
    sim.set_state(qpos=np.ascontiguousarray(qpos[sl, : sim.nq].T), qvel=np.ascontiguousarray(qvel[sl, : sim.nv].T), ee_lag=np.ascontiguousarray(lag[sl].T))
    for a in acts:
        sim.step(a[sl])
    st = sim.get_state()
    out = {k: np.array(st[k]) for k in ("qpos", "qvel", "ee_lag", "warm")}
    sim.close()
    return out


@pytest.mark.parametrize("task,mode,n", CASES)
def test_two_runs_are_bit_identical(hip_lib, task, mode, n):
    a, b = _rollout(task, mode, n), _rollout(task, mode, n)
    assert np.isfinite(a["qpos"]).all() and np.isfinite(a["qvel"]).all()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("task,mode", [("reach", "joint"), ("push", "joint"), ("pick_place", "ee")])
def test_shards_and_the_65_env_job_match_the_320_env_job(hip_lib, task, mode):
    """the shard rule of DESIGN section 6 at these shapes.  A shard other than a job's last must hold a multiple of 64 envs (lcr_create refuses others), so a 65-env
    shard can only be the last one: envs [64, 129) of a 129-env job, beside [0, 64).  And the 65-env job against the first 65 envs of the 320-env job: env 64 is alone
    in its wave there and one of 64 here, the bits of an env do not depend on the other lanes of its wave"""
    whole = _rollout(task, mode, 320)
    lo, hi = _rollout(task, mode, 256, env_id_offset=0, global_envs=320), _rollout(task, mode, 64, env_id_offset=256, global_envs=320)
    for k in whole:
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]], axis=-1), err_msg=k)
    job = _rollout(task, mode, 129)
    lo, hi = _rollout(task, mode, 64, env_id_offset=0, global_envs=129), _rollout(task, mode, 65, env_id_offset=64, global_envs=129)
    for k in job:
        np.testing.assert_array_equal(job[k], np.concatenate([lo[k], hi[k]], axis=-1), err_msg=k)
        np.testing.assert_array_equal(job[k], whole[k][..., :129], err_msg=k)
    small = _rollout(task, mode, 65)
    for k in whole:
        np.testing.assert_array_equal(whole[k][..., :65], small[k], err_msg=k)
