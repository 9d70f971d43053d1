"""The one-cube Newton kernels step with a pair of launches (csrc/lcr_kernels.hip: STEP_FAST_ONLY): a kernel that holds only the fast substep copy,
and behind it the kernel with both copies, gated by one flag per 64-env wave.  A wave whose fast copy gives up (more than LCR_COOP_MAX coupled envs in a substep) stores
nothing in the first launch and repeats its control step in the second, which is the code LCR_REDO_KERNEL=0 runs alone.

What is bit-for-bit here and what is not.  The second launch against LCR_REDO_KERNEL=0: the same kernel from the same inputs -- equal bits, asserted.  A wave that never
bails, under two values of LCR_COOP_MAX: the same kernel from the same inputs -- equal bits, asserted.  The fast-copy-only kernel against the kernel with both copies is
another compilation of the source under -ffast-math: printed, not asserted.  So the comparisons with LCR_REDO_KERNEL=0 run in lockstep: before every control step the
legacy sim takes the pair sim's whole state (set_state(**get_state()): qpos, qvel, lagged kinematics, targets, step counts, rng words, carried forces), both step, and the
waves whose flag is up in THAT step are compared -- every array of get_state and every step output.

(1) Forced bail at substep 0, LCR_COOP_MAX=0: jobs of 64, 65 and 320 envs built from the states of tests/test_gpu_small_solve_slots.py, whole waves with patients (seven
    coupled envs beside floor-contact, joint-limit and free lanes) and whole waves without.  320 envs: waves 1, 3 and 4 hold patients -- flagged and unflagged waves in
    the first workgroup, and a second workgroup whose only real wave is flagged.  65 envs: wave 0 without, env 64 a patient alone among 63 shadow lanes.  The flags
    of the first step name exactly the waves with patients, a wave without patients is never flagged; flagged waves equal LCR_REDO_KERNEL=0, the others equal the same
    job at the default LCR_COOP_MAX (where no flag is up), and the pair agrees with the fp64 oracle at the tolerances and shares of tests/test_gpu_small_solve_slots.py
    (= tests/test_gpu_parity.py's).
(2) Bail in a later substep and across auto-resets, LCR_COOP_MAX=0: PushCube (joint) and PickPlaceCube (ee), 320 envs, max_episode_steps 3, 40 steps of seeded random
    actions.  Every fourth cube of waves 1 and 3 starts next to a finger pad: under ee control no env of 8192 brings a finger to its cube within three steps of a reset
    (fp64 oracle, 40 steps), so without the placement PickPlaceCube would never raise a flag.  Asserted: some step has a flagged wave, some step has a flagged wave in
    which an env is reset; in lockstep the flagged waves' outputs, terminal observations and state -- the rng words among them: the generator is advanced once, not
    twice -- equal LCR_REDO_KERNEL=0.
(3) Nothing flagged: ReachCube from its reset at the default LCR_COOP_MAX, ten steps, every flag zero, two runs equal.
(4) Shards: the 320-env job of (1) cut into 64 + 256 envs equals the whole job, flags included."""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_small_solve_slots import KINDS, LANE_KIND, _job, _tolerances

pytestmark = pytest.mark.gpu

PATIENT_WAVE = LANE_KIND                                              # seven coupled envs (every rare kind, two pinches) beside lanes of the common kinds
PLAIN_WAVE = tuple((5, 6, 7, 8, 10, 10)[i % 6] for i in range(64))   # both pads / one pad / a link proxy on the floor, joints beyond a limit, free lanes: nobody coupled
LAYOUT = {64: (True,), 65: (False, True), 320: (False, True, False, True, True)}   # which waves hold patients
CASES = [("reach", "joint", 64), ("reach", "joint", 65), ("reach", "joint", 320), ("pick_place", "ee", 65), ("pick_place", "ee", 320)]
STATE_KEYS = ("qpos", "qvel", "ee_lag", "target", "elapsed", "rng", "current_goal", "sim_time", "warm")
OUT_KEYS = ("arm_qpos", "arm_qvel", "cube_pos", "aux_pos", "reward", "terminated", "truncated", "is_success", "did_reset")


def _kinds(n):
    return np.array([(PATIENT_WAVE if LAYOUT[n][i // 64] else PLAIN_WAVE)[i % 64] for i in range(n)])


def _sim(monkeypatch, task, n, mode, coop_max, paired, **kw):
    """LCR_COOP_MAX and LCR_REDO_KERNEL are read at lcr_create"""
    from gym_lowcostrobot_amd import VecSim

    for name, val in (("LCR_COOP_MAX", coop_max), ("LCR_REDO_KERNEL", None if paired else "0")):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    kw.setdefault("auto_reset", False); kw.setdefault("max_episode_steps", 0)
    sim = VecSim(task, n, observation_mode="state", action_mode=mode, preset="faithful", diagnostics=True, **kw)
    monkeypatch.delenv("LCR_COOP_MAX", raising=False); monkeypatch.delenv("LCR_REDO_KERNEL", raising=False)
    return sim


def _place(sim, task, mode, n, off=0):
    qpos, qvel, lag, acts = _job(task, mode, _kinds(n))
    sl = slice(off, off + sim.n)
    sim.reset(seeds=np.arange(off, off + sim.n, dtype=np.uint64))
    sim.set_state(qpos=np.ascontiguousarray(qpos[sl, : sim.nq].T), qvel=np.ascontiguousarray(qvel[sl, : sim.nv].T), ee_lag=np.ascontiguousarray(lag[sl].T))
    return [a[sl] for a in acts]


def _snapshot(sim):
    """every array of get_state, every step output (observations, reward, flags; the terminal observation of the envs that were reset), the flags of the step"""
    out = {k: np.array(v) for k, v in sim.get_state().items()}
    h = sim.fetch_host()
    for k in OUT_KEYS:
        out[k] = None if h[k] is None else np.array(h[k]).T.copy() if h[k].ndim == 2 else np.array(h[k])
    out["terminal_obs"] = np.zeros((18, sim.n), np.float32)
    if h["terminal_obs"] is not None:
        out["terminal_obs"][:, out["did_reset"]] = np.array(h["terminal_obs"]).T[:, out["did_reset"]]
    out["flags"] = sim.redo_flags()
    return out


def _assert_equal(a, b, envs, what):
    """the columns `envs` (bool per env) of every array of two snapshots"""
    for k in a:
        if k == "flags" or a[k] is None:
            continue
        np.testing.assert_array_equal(a[k][..., envs], b[k][..., envs], err_msg=f"{what}: {k}")


def _lockstep(pair, legacy, acts):
    """steps both; before each step the legacy sim takes the pair sim's state.  Asserts the flagged waves equal; returns the pair sim's snapshots and how many envs of
    unflagged waves differ anywhere (the fast-copy-only kernel against the kernel with both copies: reported)"""
    shots, moved = [], 0
    assert pair.redo_flags() is not None and pair.redo_paired and legacy.redo_flags() is not None and not legacy.redo_paired
    for t, a in enumerate(acts):
        legacy.set_state(**pair.get_state())
        pair.step(a); legacy.step(a)
        p, g = _snapshot(pair), _snapshot(legacy)
        assert not g["flags"].any()   # (LCR_REDO_KERNEL=0 writes no flag)
        envs = np.repeat(p["flags"], 64)[: pair.n]
        _assert_equal(p, g, envs, f"step {t}, waves {np.nonzero(p['flags'])[0].tolist()} against LCR_REDO_KERNEL=0")
        if not envs.all():
            moved += int(np.any([(p[k][..., ~envs] != g[k][..., ~envs]).reshape(-1, (~envs).sum()).any(0) for k in STATE_KEYS], axis=0).sum())
        shots.append(p)
    return shots, moved


_RUNS = {}


def _forced(monkeypatch, task, mode, n):
    """the job of (1) under LCR_COOP_MAX=0, computed once per case: the pair's snapshots of the five steps (checked against LCR_REDO_KERNEL=0 on the way)"""
    if (task, mode, n) not in _RUNS:
        pair, legacy = _sim(monkeypatch, task, n, mode, 0, True), _sim(monkeypatch, task, n, mode, 0, False)
        acts = _place(pair, task, mode, n); _place(legacy, task, mode, n)
        shots, moved = _lockstep(pair, legacy, acts)
        print(f"[redo_kernel] {task} n={n}: envs of unflagged waves that differ from LCR_REDO_KERNEL=0 after a step (reported): {moved}")
        pair.close(); legacy.close()
        _RUNS[(task, mode, n)] = shots
    return _RUNS[(task, mode, n)]


@pytest.mark.parametrize("task,mode,n", CASES)
def test_forced_bail_goes_through_the_second_launch(hip_lib, monkeypatch, task, mode, n):
    shots = _forced(monkeypatch, task, mode, n)
    with_patients = np.array(LAYOUT[n])
    np.testing.assert_array_equal(shots[0]["flags"], with_patients)
    for s in shots:
        assert not s["flags"][~with_patients].any(), s["flags"]
        assert np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all()
    # the waves without patients: the same job at the default LCR_COOP_MAX, where every wave stays in the first launch
    plain = np.repeat(~with_patients, 64)[:n]
    base = _sim(monkeypatch, task, n, mode, None, True)
    acts = _place(base, task, mode, n)
    for t, a in enumerate(acts):
        base.step(a)
        b = _snapshot(base)
        assert not b["flags"].any(), (t, b["flags"])
        _assert_equal(shots[t], b, plain, f"step {t}, waves without patients against the default LCR_COOP_MAX")
    base.close()


@pytest.mark.parametrize("task,mode,n", CASES)
def test_forced_bail_against_the_oracle(hip_lib, monkeypatch, task, mode, n):
    kinds = _kinds(n)
    qpos, qvel, lag, acts = _job(task, mode, kinds)
    monkeypatch.setenv("LCR_COOP_MAX", "0")
    sim, o = util.make_pair(task, n, preset="faithful", auto_reset=False, max_episode_steps=0, action_mode=mode)
    monkeypatch.delenv("LCR_COOP_MAX", raising=False)
    o.reset(seeds=np.arange(n)); sim.reset(seeds=np.arange(n))
    o.qpos[:] = qpos; o.qvel[:] = qvel; o.ee_lag[:] = lag
    for t, a in enumerate(acts):
        dq, dv, ok, st = util.parity_step(sim, o, a, 4e-5, 4e-3, max_dq=3e-2, where=("redo_kernel", task, n, t), carry=False)
        if t == 0:
            np.testing.assert_array_equal(sim.redo_flags(), np.array(LAYOUT[n]))
        if t in (0, len(acts) - 1):
            for k, name in enumerate(KINDS):
                sel = kinds == k
                if not sel.any():
                    continue
                tq, tv, share = _tolerances(task, name, int(sel.sum()))
                within = (dq[sel] <= tq) & (dv[sel] <= tv)
                print(f"[redo_kernel] {task} n={n} step {t + 1} {name}: {int(sel.sum())} envs, max |dq| {dq[sel].max():.2e} |dv| {dv[sel].max():.2e}, within {within.mean():.3f}")
                assert within.mean() >= share, (task, n, t, name, np.sort(dq[sel])[-3:], np.sort(dv[sel])[-3:])
    sim.close()


@pytest.mark.parametrize("task,mode", [("push", "joint"), ("pick_place", "ee")])
def test_bail_in_a_later_substep_and_across_auto_resets(hip_lib, monkeypatch, task, mode):
    from oracle import orc

    n, steps = 320, 40
    rng = np.random.default_rng(5)   # (with this seed both tasks show what is asserted below; the fp64 oracle predicts flags in steps 1-3, PushCube's in most later steps too)
    pair, legacy = (_sim(monkeypatch, task, n, mode, 0, p, auto_reset=True, max_episode_steps=3) for p in (True, False))
    pair.reset(seeds=np.arange(n, dtype=np.uint64)); legacy.reset(seeds=np.arange(n, dtype=np.uint64))
    st = pair.get_state()
    for e in [e for w in (1, 3) for e in range(64 * w, 64 * w + 64, 4)]:   # a cube next to a finger pad (tests/test_gpu_parity.py: _states_with_slots)
        _, _, sph = orc.fk(st["qpos"][:6, e])
        st["qpos"][6:9, e] = sph[(e >> 2) & 1] + rng.normal(0, 0.012, 3)
    st["qpos"][8] = np.maximum(st["qpos"][8], 0.0149)
    pair.set_state(**st)
    acts = [rng.uniform(-1, 1, (n, pair.action_dim)).astype(np.float32) for _ in range(steps)]
    shots, moved = _lockstep(pair, legacy, acts)
    flagged = np.array([s["flags"] for s in shots])
    resets = np.array([np.add.reduceat(s["did_reset"].astype(int), np.arange(0, n, 64)) > 0 for s in shots])
    print(f"[redo_kernel] {task}: flagged waves per step {flagged.sum(1).tolist()}, of them with a reset {(flagged & resets).sum(1).tolist()}; "
          f"envs of unflagged waves that differ from LCR_REDO_KERNEL=0 after a step (reported): {moved}")
    assert (flagged.any(1) & ~flagged.all(1)).any()   # a step with waves in the second launch beside waves that are not
    assert (flagged & resets).any()                   # a wave of the second launch resets an env
    pair.close(); legacy.close()


def test_nothing_flagged(hip_lib, monkeypatch):
    runs = []
    for _ in range(2):
        sim = _sim(monkeypatch, "reach", 320, "joint", None, True, auto_reset=True, max_episode_steps=50)
        sim.reset(seeds=np.arange(320, dtype=np.uint64))
        rng = np.random.default_rng(3)
        shots = []
        for t in range(10):
            sim.step(rng.uniform(-1, 1, (320, sim.action_dim)).astype(np.float32))
            shots.append(_snapshot(sim))
            assert not shots[-1]["flags"].any(), (t, shots[-1]["flags"])
        sim.close()
        runs.append(shots)
    every = np.ones(320, bool)
    for t, (a, b) in enumerate(zip(*runs)):
        _assert_equal(a, b, every, f"step {t}, two runs")


@pytest.mark.parametrize("task,mode", [("reach", "joint"), ("pick_place", "ee")])
def test_shards_equal_the_whole_job(hip_lib, monkeypatch, task, mode):
    whole = _forced(monkeypatch, task, mode, 320)
    parts = []
    for off, m in ((0, 64), (64, 256)):
        sim = _sim(monkeypatch, task, m, mode, 0, True, env_id_offset=off, global_envs=320)
        acts = _place(sim, task, mode, 320, off)
        shots = []
        for a in acts:
            sim.step(a)
            shots.append(_snapshot(sim))
        sim.close()
        parts.append(shots)
    for t, w in enumerate(whole):
        lo, hi = parts[0][t], parts[1][t]
        np.testing.assert_array_equal(w["flags"], np.concatenate([lo["flags"], hi["flags"]]), err_msg=f"step {t}: flags")
        for k in w:
            if k != "flags" and w[k] is not None:
                np.testing.assert_array_equal(w[k], np.concatenate([lo[k], hi[k]], axis=-1), err_msg=f"step {t}: {k}")
