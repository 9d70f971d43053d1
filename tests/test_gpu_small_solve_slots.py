"""What the small arm solve of the Newton kernels' fast substep visits (csrc/lcr_kernels.hip: slot_solve): only the arm slots that a lane which is NOT coupled has
active.  A coupled lane (a "patient": finger or gripper-body proxy on its cube) sits that solve out and gets every force from the cooperative solve, so neither its
own result nor that of any other lane may depend on which wave it shares with whom.

(1) Layout invariance, 128 envs, reach and push: the same 128 states in two lane orders.  Order A spreads the patients over both waves beside floor-contact lanes;
    order B puts all eight patients (lcr_config.coop_max) into wave 0 beside free lanes only -- its small arm solve has no slot at all -- and every floor-contact and
    joint-limit lane into wave 1, which has no patient.  After five control steps qpos, qvel and the carried forces of every env are equal (array_equal: a carried
    force of an inactive slot is a zero whose sign depends on whether its wave visited the slot -- the set-up reads it as `active ? f : 0`).
(2) coop_share owner-only / shared / hand-off on the order-B job: equal.
(3) Patients of the less common kinds against the fp64 oracle (util.parity_step), 64 and 65 envs, reach (joint) and pick_place (ee); StackTwoCubes and PushCubeLoop at
    64: one finger only on the cube (slot 0 alone, slot 1 alone), a finger on the cube with a pad on the floor (slot 0 or 1 with slot 2 or 3 in one lane), a pinched
    cube with joint 0 beyond its lower limit, a gripper-body proxy on the cube (slot 4 against a cube) -- each wave holds at most eight of them beside floor-contact,
    joint-limit and free lanes.  At 65 envs the only real lane of the second wave is a slot-0-alone patient: its 63 shadow lanes carry that contact uncoupled.

Tolerances and shares: tests/test_gpu_parity.py, as tests/test_gpu_newton_consts.py copies them (fingers on the cube: test_pinch_grasp_finger_cube_contacts 2e-5 / 4e-3 /
0.985; a lane that also has an arm contact with the floor, and the link proxies: test_link_proxy_contacts 4e-5, StackTwoCubes 6e-5 / 4e-3).  The placements are
selected on the CPU by the rule of tests/test_gpu_newton_consts.py: a state is used only if the oracle's fp32 twin stays within a quarter of the tightest tolerance
(2e-5 rad, 2e-3 rad/s) of the fp64 build over the five steps and takes the same decisions."""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_newton_consts import ACT_SCALE, STEPS, _placement as _common_placement

pytestmark = pytest.mark.gpu

RARE = ("finger0", "finger1", "finger_and_floor", "limit_patient", "proxy_on_cube")
COMMON = ("both_pads", "one_pad", "proxy", "limits", "finger_cube", "free")   # tests/test_gpu_newton_consts.py: KINDS
KINDS = RARE + COMMON
N_CAND = 768          # candidates per recipe
# kind of lane i of the oracle comparisons: LANE_KIND[i % 64] -- the five rare patients and two pinches per wave, seven of the eight coupled envs a wave solves
# cooperatively (lcr_config.coop_max: with more the wave would take the coupled SIMT copy, where nobody sits out); lane 0, and so env 64 of a 65-env job, is a
# slot-0-alone patient
_PATIENT_AT = {0: 0, 9: 1, 18: 2, 27: 3, 36: 4, 45: 9, 54: 9}
LANE_KIND = tuple(_PATIENT_AT.get(i, (5, 6, 7, 8, 10, 10)[i % 6]) for i in range(64))
ORACLE_CASES = [("reach", "joint", 64), ("reach", "joint", 65), ("pick_place", "ee", 64), ("pick_place", "ee", 65), ("stack", "joint", 64), ("push_loop", "joint", 64)]


def _tolerances(task, kind, n_kind):
    """(atol_q, atol_v, least share of the kind's envs within them), see the module docstring"""
    if kind in ("finger_and_floor", "proxy_on_cube", "both_pads", "one_pad", "proxy"):
        return (6e-5 if task == "stack" else 4e-5), 4e-3, (0.975 if task == "stack" else min(0.99, 1.0 - 1.5 / n_kind))
    if kind in ("finger0", "finger1", "limit_patient", "finger_cube"):
        return 2e-5, 4e-3, 0.985
    return 2e-5, 2e-3, 0.99


_PLACED = {}


def _pinch_at(q):
    """cube centre and yaw that put the cube between the finger spheres of arm pose q (joints 1-4 zero: the fingers' line is horizontal)"""
    from oracle import orc

    _, _, sph = orc.fk(q)
    d = sph[0] - sph[1]
    return 0.5 * (sph[0] + sph[1]), np.arctan2(d[1], d[0])


def _pools(task, mode):
    """per kind of KINDS: (qpos, qvel, ee_lag, [actions of the five steps]) of the states that qualify.  Computed once per task on the CPU."""
    if (task, mode) in _PLACED:
        return _PLACED[(task, mode)]
    from oracle import orc

    am = {"joint": 0, "ee": 1}[mode]
    rng = np.random.default_rng(909)
    n = 3 * N_CAND
    o = orc.Oracle(task, n, preset="faithful", auto_reset=0, max_episode_steps=0, action_mode=am)
    o.reset(seeds=np.arange(n))
    near_finger, near_body, turned = slice(0, N_CAND), slice(N_CAND, 2 * N_CAND), slice(2 * N_CAND, n)
    # random arm states with the cube dropped next to a finger pad (a finger on the cube, alone or with a pad on the floor) / next to the gripper body (tests/test_gpu_parity.py:
    # _states_with_slots)
    q, qd = util.random_arm_state(rng, 2 * N_CAND, scale_v=1.0)
    o.qpos[: 2 * N_CAND, :6] = q; o.qvel[: 2 * N_CAND, :6] = qd
    clear = np.zeros(n, bool)     # every link proxy at least 5 mm above the floor: an active proxy slot is then a proxy on the cube
    for e in range(2 * N_CAND):
        lp, _, sph = orc.fk(q[e])
        o.qpos[e, 6:9] = (sph[e & 1] if e < N_CAND else lp[4]) + rng.normal(0, 0.012, 3)
        o.qpos[e, 9:13] = [1, 0, 0, 0]
        c, r = orc.proxies(q[e])
        clear[e] = (c[:, 2] - r).min() > 0.005
    o.qpos[: 2 * N_CAND, 8] = np.maximum(o.qpos[: 2 * N_CAND, 8], 0.0149)
    # the pinch of util.pinch_setup turned with joint 0 past its lower limit
    po = orc.Oracle(task, 1, preset="faithful", auto_reset=0, max_episode_steps=0, action_mode=am)
    po.reset(seeds=np.arange(1))
    grip = util.pinch_setup(po)
    for e in range(turned.start, n):
        qe = np.zeros(6); qe[0] = -3.14 - rng.uniform(0, 0.01); qe[5] = grip + rng.uniform(-0.02, 0.02)
        c, yaw = _pinch_at(qe)
        o.qpos[e, :6] = qe; o.qpos[e, 6:9] = c + rng.normal(0, 3e-4, 3); o.qpos[e, 9:13] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        o.qvel[e, :] = 0; o.qvel[e, :6] = rng.normal(0, 0.1, 6)
        o.ee_lag[e] = orc.fk(qe)[1]    # (ee control: the lagged target where the gripper is -- the reset's lies half a turn of joint 0 away)
    util.sync_oracle_to_f32(o)
    q0, v0, lag0 = o.qpos.copy(), o.qvel.copy(), o.ee_lag.copy()
    t = util._twin(o)
    acts = [(ACT_SCALE * rng.uniform(-1, 1, (n, o.action_dim))).astype(np.float32) for _ in range(STEPS)]
    rel = np.zeros(n)    # largest |fp32 - fp64| of the five steps, qpos in units of 1e-5, qvel in units of 1e-3
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
        rel[(t.active_count != o.active_count) | (t.choice != o.choice)] = np.inf
        if first is None:
            first = o.active_mask.copy()
    b = lambda k: ((first >> k) & 1).astype(bool)
    pos = np.arange(n)
    where = lambda sl: (pos >= sl.start) & (pos < sl.stop)
    floor_pad = b(14) | b(15)
    kind = np.full(n, -1)    # (the random arm states lie inside the joint limits: util.random_arm_state)
    kind[where(near_finger) & b(12) & ~b(13) & ~floor_pad & ~b(16)] = 0
    kind[where(near_finger) & b(13) & ~b(12) & ~floor_pad & ~b(16)] = 1
    kind[where(near_finger) & (b(12) | b(13)) & floor_pad] = 2
    kind[where(turned) & b(12) & b(13)] = 3
    kind[where(near_body) & b(16) & ~b(12) & ~b(13) & ~floor_pad & clear] = 4
    kind[rel > 0.5] = -1
    pools = {}
    for k, name in enumerate(RARE):
        idx = np.nonzero(kind == k)[0]
        assert len(idx) >= 3, (task, name, len(idx))    # (a 65-env job takes two states of a kind, the 128-state job one)
        pools[name] = (q0[idx], v0[idx], lag0[idx], [a[idx] for a in acts])
    cq, cv, cl, ca, ck = _common_placement(task, mode)
    for k, name in enumerate(COMMON):
        idx = np.nonzero(ck == k)[0]
        pools[name] = (cq[idx], cv[idx], cl[idx], [a[idx] for a in ca])
    _PLACED[(task, mode)] = pools
    return pools


def _job(task, mode, kinds):
    """the states of a job whose env i is of kind KINDS[kinds[i]]: (qpos, qvel, ee_lag, actions[STEPS]); the j-th env of a kind takes the kind's j-th state (repeating)"""
    pools = _pools(task, mode)
    seen = {}
    pick = []
    for k in kinds:
        j = seen.get(k, 0); seen[k] = j + 1
        pick.append((KINDS[k], j % len(pools[KINDS[k]][0])))
    cat = lambda f: np.stack([f(pools[name], j) for name, j in pick])
    return cat(lambda p, j: p[0][j]), cat(lambda p, j: p[1][j]), cat(lambda p, j: p[2][j]), [cat(lambda p, j, s=s: p[3][s][j]) for s in range(STEPS)]


@pytest.mark.parametrize("task,mode,n", ORACLE_CASES)
def test_rare_patients_against_the_oracle(hip_lib, task, mode, n):
    kinds = np.array([LANE_KIND[i % 64] for i in range(n)])
    qpos, qvel, lag, acts = _job(task, mode, kinds)
    sim, o = util.make_pair(task, n, preset="faithful", auto_reset=False, max_episode_steps=0, action_mode=mode)
    o.reset(seeds=np.arange(n)); sim.reset(seeds=np.arange(n))
    o.qpos[:] = qpos; o.qvel[:] = qvel; o.ee_lag[:] = lag
    loose_q = 6e-5 if task == "stack" else 4e-5
    for t, a in enumerate(acts):
        dq, dv, ok, st = util.parity_step(sim, o, a, loose_q, 4e-3, max_dq=3e-2, where=("small_solve_slots", task, n, t), carry=False)
        if t == 0:   # the placement is what it says: the slots of the first step (oracle slot ids 12-13 finger<->cube, 14-15 finger<->floor, 16 link proxies)
            m = o.active_mask
            b = lambda k: ((m >> k) & 1).astype(bool)
            assert (b(12) & ~b(13))[kinds == 0].all() and (b(13) & ~b(12))[kinds == 1].all()
            assert ((b(12) | b(13)) & (b(14) | b(15)))[kinds == 2].all()
            assert (b(12) & b(13))[kinds == 3].all() and (qpos[kinds == 3, 0] < -3.14).all()    # (qpos: the state the step started from)
            assert (b(16) & ~b(12) & ~b(13))[kinds == 4].all()
            assert (sim.active_mask.numpy()[kinds < 5] == m[kinds < 5]).all()
        if t in (0, STEPS - 1):
            for k, name in enumerate(KINDS):
                sel = kinds == k
                if not sel.any():
                    continue
                tq, tv, share = _tolerances(task, name, int(sel.sum()))
                within = (dq[sel] <= tq) & (dv[sel] <= tv)
                print(f"[small_solve_slots] {task} n={n} step {t + 1} {name}: {int(sel.sum())} envs, max |dq| {dq[sel].max():.2e} |dv| {dv[sel].max():.2e}, within {within.mean():.3f}")
                assert within.mean() >= share, (task, n, t, name, np.sort(dq[sel])[-3:], np.sort(dv[sel])[-3:])
    sim.close()


# ---- the two lane orders of 128 states: eight patients (every rare kind, three pinches), 56 free lanes, 64 lanes with a floor contact or a joint beyond a limit ----
_PATIENTS = (0, 1, 2, 3, 4, 9, 9, 9)
_CONTACT = tuple((5, 6, 7, 8)[i % 4] for i in range(64))
ORDER_B = np.array(_PATIENTS + (10,) * 56 + _CONTACT)
# order A: wave w holds patients 4 w .. 4 w + 3, then alternately a free and a contact lane -- as positions of order B
ORDER_A_FROM_B = np.array([j for w in range(2) for j in ([4 * w + i for i in range(4)] + [x for i in range(28) for x in (8 + 28 * w + i, 64 + 32 * w + i)] + [64 + 32 * w + 28 + i for i in range(4)])])
assert sorted(ORDER_A_FROM_B) == list(range(128))


def _rollout(task, mode, order=None, **kw):
    """five control steps of the 128-state job, env i of the run being state order[i] of order B; returns the state in the order of B"""
    from gym_lowcostrobot_amd import VecSim

    qpos, qvel, lag, acts = _job(task, mode, ORDER_B)
    order = np.arange(128) if order is None else order
    sim = VecSim(task, 128, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, diagnostics=True, **kw)
    sim.reset(seeds=np.arange(128, dtype=np.uint64))
    sim.set_state(qpos=np.ascontiguousarray(qpos[order, : sim.nq].T), qvel=np.ascontiguousarray(qvel[order, : sim.nv].T), ee_lag=np.ascontiguousarray(lag[order].T))
    inv = np.argsort(order)
    first = None
    for a in acts:
        sim.step(a[order])
        if first is None:
            first = sim.active_mask.numpy()[inv].copy()    # the slots that were active in the first control step (ids as the oracle's: tests/util.py)
    st = sim.get_state()
    out = {k: np.array(st[k])[..., inv] for k in ("qpos", "qvel", "warm")}
    out["first_mask"] = first
    sim.close()
    return out


_ROLLED = {}


def _order_b(task, mode):
    if (task, mode) not in _ROLLED:
        _ROLLED[(task, mode)] = _rollout(task, mode)
    return _ROLLED[(task, mode)]


@pytest.mark.parametrize("task,mode", [("reach", "joint"), ("push", "joint")])
def test_lane_order_does_not_show(hip_lib, task, mode):
    b = _order_b(task, mode)
    a = _rollout(task, mode, ORDER_A_FROM_B)
    assert np.isfinite(b["qpos"]).all() and np.isfinite(b["qvel"]).all()
    m = b["first_mask"]    # the layout is what it says: patients (a finger or a proxy against the cube: slots 12, 13, 16), then lanes without any arm contact
    assert ((m[:8] & 0x13000) != 0).all() and ((m[8:64] & 0x1F000) == 0).all() and ((m[64:][np.arange(64) % 4 != 3] & 0x3000) == 0).all(), (m[:8], m[8:64], m[64:])    # (every fourth lane of wave 1 is a joint-limit lane, placed by hand)
    for k in b:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{task}: {k}, order A against order B")


@pytest.mark.parametrize("task,mode", [("reach", "joint"), ("push", "joint")])
def test_share_modes_agree_on_the_sorted_job(hip_lib, task, mode):
    b = _order_b(task, mode)
    for share in ("owner", "shared", "handoff"):
        got = _rollout(task, mode, coop_share=share)
        for k in b:
            np.testing.assert_array_equal(got[k], b[k], err_msg=f"{task}: {k}, coop_share {share}")
