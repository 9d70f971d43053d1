"""coop_share = "ahead" of the one-cube Newton kernels (csrc/lcr_kernels.hip: CQ_AHEAD): a stepping wave that has no coupled env ("patient") in a
substep looks at the workgroup's queue once after its two small solves and makes one cooperative pass over posted patients whose owner is at an earlier substep.  Who
solves a patient is a race between the waves; what comes out is not: every comparison below is array_equal.

(1) Identity, 256 / 257 / 320 envs (one full workgroup; a second workgroup whose only wave has one real lane and 63 shadow lanes; a second workgroup with one real wave
    and three serving waves), reach and push, states of tests/test_gpu_small_solve_slots.py placed with set_state: wave 0 holds eight patients (lcr_config.coop_max)
    beside free lanes, every other wave floor-contact and joint-limit lanes and no patient -- waves 1-3 are still stepping while wave 0, two passes per substep, falls
    behind.  Ten control steps (the five actions of the states, twice) under "owner", "shared" and "ahead": every array of get_state, reward, flags and terminal
    observations are equal after every step.
(2) The path ran: summed over those ten steps the per-wave counter of patients solved through the new entry (diagnostics = 2, lane 3 of the wave's active_count words)
    is above zero in some wave of workgroup 0 under "ahead" and zero in every wave under "shared".  Over the run, not per step: which wave helps is the race.
(3) The "owner" job against the fp64 oracle, ten re-synchronised steps (util.parity_step: every env outside 4e-5 / 4e-3 has to be explained, in every step); per kind of
    lane the tolerances and shares of tests/test_gpu_small_solve_slots.py: _tolerances after steps 1 and 5 -- the window over which the states were selected (their fp32
    twin stays within a quarter of the tightest tolerance for the five steps of their five actions).
(4) Across auto-resets: PushCube (joint) and PickPlaceCube (ee), 320 envs, three-step episodes, 40 steps of seeded random actions, every fourth cube of waves 1 and 3
    next to a finger pad (tests/test_gpu_redo_kernel.py: without it ee control brings no finger to its cube within three steps): "ahead" equals "owner" in every
    output, terminal observation and array of get_state, the rng words among them.
(5) Shards of 64 + 256 envs equal the 320-env job of (1) under "ahead".
(6) Forced bails, LCR_COOP_MAX=0, 320 envs, five steps, waves 1, 3 and 4 with patients: the pair of launches under "ahead" against LCR_REDO_KERNEL=0 in lockstep (before
    every step the second sim takes the first one's whole state): equal in every env, and the flags name the waves with patients."""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_small_solve_slots import KINDS, LANE_KIND, _job, _tolerances

pytestmark = pytest.mark.gpu

_PATIENTS = (0, 1, 2, 3, 4, 9, 9, 9)                         # every rare kind of patient and three pinches: eight, what a wave solves cooperatively
_CONTACT = tuple((5, 6, 7, 8)[i % 4] for i in range(64))     # both pads / one pad / a link proxy on the floor, joints beyond a limit: nobody coupled
WAVE0 = _PATIENTS + (10,) * 56
SIZES = (256, 257, 320)
TASKS = [("reach", "joint"), ("push", "joint")]
MODES = ("owner", "shared", "ahead")
STATE_KEYS = ("qpos", "qvel", "ee_lag", "target", "elapsed", "rng", "current_goal", "sim_time", "warm")
OUT_KEYS = ("arm_qpos", "arm_qvel", "cube_pos", "aux_pos", "reward", "terminated", "truncated", "is_success", "did_reset")


def _kinds(n):
    return np.array([(WAVE0 if i < 64 else _CONTACT)[i % 64] for i in range(n)])


def _snapshot(sim):
    """every array of get_state, every step output (observations, reward, flags; the terminal observation of the envs that were reset)"""
    out = {k: np.array(v) for k, v in sim.get_state().items()}
    h = sim.fetch_host()
    for k in OUT_KEYS:
        out[k] = None if h[k] is None else np.array(h[k]).T.copy() if h[k].ndim == 2 else np.array(h[k])
    out["terminal_obs"] = np.zeros((18, sim.n), np.float32)
    if h["terminal_obs"] is not None:
        out["terminal_obs"][:, out["did_reset"]] = np.array(h["terminal_obs"]).T[:, out["did_reset"]]
    return out


def _assert_equal(a, b, what):
    assert set(STATE_KEYS) <= set(a)
    for k in a:
        if a[k] is not None:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _place(sim, task, mode, kinds, off=0):
    qpos, qvel, lag, acts = _job(task, mode, kinds)
    sl = slice(off, off + sim.n)
    sim.reset(seeds=np.arange(off, off + sim.n, dtype=np.uint64))
    sim.set_state(qpos=np.ascontiguousarray(qpos[sl, : sim.nq].T), qvel=np.ascontiguousarray(qvel[sl, : sim.nv].T), ee_lag=np.ascontiguousarray(lag[sl].T))
    return [a[sl] for a in acts] * 2


_RUNS = {}


def _run(task, mode, n, share):
    """the job of (1), once per case: the snapshots of the ten steps and, per wave, the patients solved through the new entry summed over the run"""
    key = (task, mode, n, share)
    if key not in _RUNS:
        from gym_lowcostrobot_amd import VecSim

        sim = VecSim(task, n, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, profile="wave_cycles", coop_share=share)
        shots, ahead = [], np.zeros((n + 63) // 64, np.int64)
        for a in _place(sim, task, mode, _kinds(n)):
            sim.step(a)
            shots.append(_snapshot(sim))
            ac = sim.active_count.numpy()
            ahead += np.array([ac[64 * w + 3] if 64 * w + 3 < n else 0 for w in range(len(ahead))], np.int64)   # (lane 3 of a wave; the one-lane wave of 257 envs has none)
        sim.close()
        _RUNS[key] = (shots, ahead)
    return _RUNS[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task,mode", TASKS)
def test_share_modes_are_equal_and_the_new_entry_ran(hip_lib, task, mode, n):
    ref, _ = _run(task, mode, n, "owner")
    for s in ref:
        assert np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all()
    counts = {}
    for share in ("shared", "ahead"):
        got, counts[share] = _run(task, mode, n, share)
        for t, (g, r) in enumerate(zip(got, ref)):
            _assert_equal(g, r, f"{task} n={n} step {t}, {share} against owner")
    print(f"[coop_ahead] {task} n={n}: patients solved through the new entry per wave over ten steps: ahead {counts['ahead'].tolist()}, shared {counts['shared'].tolist()}")
    assert counts["ahead"][:4].max() > 0, counts["ahead"]
    assert not counts["shared"].any(), counts["shared"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task,mode", TASKS)
def test_owner_run_against_the_oracle(hip_lib, task, mode, n):
    kinds = _kinds(n)
    qpos, qvel, lag, acts = _job(task, mode, kinds)
    sim, o = util.make_pair(task, n, preset="faithful", auto_reset=False, max_episode_steps=0, action_mode=mode, coop_share="owner")
    o.reset(seeds=np.arange(n)); sim.reset(seeds=np.arange(n))
    o.qpos[:] = qpos; o.qvel[:] = qvel; o.ee_lag[:] = lag
    for t, a in enumerate(acts * 2):
        dq, dv, ok, st = util.parity_step(sim, o, a, 4e-5, 4e-3, max_dq=3e-2, where=("coop_ahead", task, n, t), carry=False)
        if t == 0:   # the layout is what it says: wave 0's first eight lanes have a finger or a proxy on the cube (oracle slots 12, 13, 16 with the cube), nobody else has
            m = o.active_mask
            assert ((m[:8] & 0x3000) != 0).sum() >= 7 and ((m[8:] & 0x3000) == 0).all(), (m[:8], np.nonzero(m[8:] & 0x3000)[0])
        if t in (0, len(acts) - 1):
            for k, name in enumerate(KINDS):
                sel = kinds == k
                if not sel.any():
                    continue
                tq, tv, share = _tolerances(task, name, int(sel.sum()))
                within = (dq[sel] <= tq) & (dv[sel] <= tv)
                print(f"[coop_ahead] {task} n={n} step {t + 1} {name}: {int(sel.sum())} envs, max |dq| {dq[sel].max():.2e} |dv| {dv[sel].max():.2e}, within {within.mean():.3f}")
                assert within.mean() >= share, (task, n, t, name, np.sort(dq[sel])[-3:], np.sort(dv[sel])[-3:])
    sim.close()


@pytest.mark.parametrize("task,mode", [("push", "joint"), ("pick_place", "ee")])
def test_across_auto_resets(hip_lib, task, mode):
    from gym_lowcostrobot_amd import VecSim
    from oracle import orc

    n, steps = 320, 40
    runs = {}
    for share in ("owner", "ahead"):
        rng = np.random.default_rng(5)
        sim = VecSim(task, n, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=True, max_episode_steps=3, diagnostics=True, coop_share=share)
        sim.reset(seeds=np.arange(n, dtype=np.uint64))
        st = sim.get_state()
        for e in [e for w in (1, 3) for e in range(64 * w, 64 * w + 64, 4)]:   # a cube next to a finger pad (tests/test_gpu_parity.py: _states_with_slots)
            _, _, sph = orc.fk(st["qpos"][:6, e])
            st["qpos"][6:9, e] = sph[(e >> 2) & 1] + rng.normal(0, 0.012, 3)
        st["qpos"][8] = np.maximum(st["qpos"][8], 0.0149)
        sim.set_state(**st)
        shots = []
        for _ in range(steps):
            sim.step(rng.uniform(-1, 1, (n, sim.action_dim)).astype(np.float32))
            shots.append(_snapshot(sim))
        sim.close()
        runs[share] = shots
    assert any(s["did_reset"].any() for s in runs["owner"])
    for t, (g, r) in enumerate(zip(runs["ahead"], runs["owner"])):
        _assert_equal(g, r, f"{task} step {t}, ahead against owner")


@pytest.mark.parametrize("task,mode", TASKS)
def test_shards_equal_the_whole_job(hip_lib, task, mode):
    from gym_lowcostrobot_amd import VecSim

    whole, _ = _run(task, mode, 320, "ahead")
    parts = []
    for off, m in ((0, 64), (64, 256)):
        sim = VecSim(task, m, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, profile="wave_cycles", coop_share="ahead",
                     env_id_offset=off, global_envs=320)
        shots = []
        for a in _place(sim, task, mode, _kinds(320), off):
            sim.step(a)
            shots.append(_snapshot(sim))
        sim.close()
        parts.append(shots)
    for t, w in enumerate(whole):
        lo, hi = parts[0][t], parts[1][t]
        for k in w:
            if w[k] is not None:
                np.testing.assert_array_equal(w[k], np.concatenate([lo[k], hi[k]], axis=-1), err_msg=f"{task} step {t}: {k}")


def test_forced_bails_compose_with_the_redo_launch(hip_lib, monkeypatch):
    from gym_lowcostrobot_amd import VecSim

    task, mode, n = "reach", "joint", 320
    with_patients = np.array([False, True, False, True, True])
    plain = tuple((5, 6, 7, 8, 10, 10)[i % 6] for i in range(64))
    kinds = np.array([(LANE_KIND if with_patients[i // 64] else plain)[i % 64] for i in range(n)])
    sims = []
    for paired in (True, False):   # (LCR_COOP_MAX and LCR_REDO_KERNEL are read at lcr_create)
        monkeypatch.setenv("LCR_COOP_MAX", "0")
        if not paired:
            monkeypatch.setenv("LCR_REDO_KERNEL", "0")
        sims.append(VecSim(task, n, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, diagnostics=True, coop_share="ahead"))
        monkeypatch.delenv("LCR_COOP_MAX", raising=False); monkeypatch.delenv("LCR_REDO_KERNEL", raising=False)
    pair, legacy = sims
    acts = _place(pair, task, mode, kinds)[:5]; _place(legacy, task, mode, kinds)
    assert pair.redo_flags() is not None and pair.redo_paired and legacy.redo_flags() is not None and not legacy.redo_paired
    for t, a in enumerate(acts):
        legacy.set_state(**pair.get_state())
        pair.step(a); legacy.step(a)
        if t == 0:
            np.testing.assert_array_equal(pair.redo_flags(), with_patients)
        assert not pair.redo_flags()[~with_patients].any() and not legacy.redo_flags().any()
        _assert_equal(_snapshot(pair), _snapshot(legacy), f"step {t}, ahead with LCR_COOP_MAX=0 against LCR_REDO_KERNEL=0")
    pair.close(); legacy.close()
