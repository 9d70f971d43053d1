"""coop_share = "early" of the one-cube Newton kernels (csrc/lcr_kernels.hip: CQ_EARLY, cq_serve_call): every stepping wave, patients ("coupled
envs") of its own or not, looks at the workgroup's queue once BEFORE its two small solves, once between them and once when its own patients are back, and each time
makes one cooperative pass over posted patients whose owner is at an earlier substep; the "ahead" entry after the small solves stays.  Every pass, and the serving of a
wave that holds no env, has bailed out or has finished its step, goes through ONE out-of-line function per code object.  Who solves a patient is a race between the
waves; what comes out is not: every comparison below is array_equal.

Layouts (states of tests/test_gpu_small_solve_slots.py placed with set_state), 256 / 257 / 320 envs (one full workgroup; a second workgroup whose only wave has one real
lane and 63 shadow lanes and whose other three waves hold no env -- they go through the out-of-line serve at once; a second workgroup with one real wave):
  "wave0":  the layout of tests/test_gpu_coop_ahead.py: wave 0 holds eight patients (lcr_config.coop_max), every other wave contact lanes and no patient.
  "every":  PushCube only: wave 0 as above, every other wave two pinches and a finger-on-cube patient in its first three lanes beside contact lanes -- every wave owns a
            patient in every substep, so the "ahead" entry (open only to a wave without one) never opens, and waves 1-3, one pass per substep against wave 0's two,
            run ahead of wave 0.

(1) Identity: ten control steps (the five actions of the states, twice) under "owner", "shared", "ahead" and "early": every array of get_state, reward, flags and
    terminal observations are equal after every step.
(2) The path ran: summed over those ten steps the per-wave counter of patients solved at the new claim points (diagnostics = 2, lane 4 of the wave's active_count words) is
    above zero in each of the waves 1-3 under "early" on both layouts (two hundred substeps with eight patients of wave 0 posted in each: a wave that never wins a take is
    not a race lost, it is the entry not opening); the counter of the "ahead" entry (lane 3) is zero in every wave under "ahead" on the "every" layout.
(3) The "owner" job against the fp64 oracle on both layouts, ten re-synchronised steps, with the tolerances of tests/test_gpu_parity.py as
    tests/test_gpu_coop_ahead.py applies them (util.parity_step: 4e-5 / 4e-3, every env outside has to be explained; per kind of lane the shares of
    tests/test_gpu_small_solve_slots.py: _tolerances after steps 1 and 5).
(4) Across auto-resets: PushCube (joint) and PickPlaceCube (ee), 320 envs, three-step episodes, 40 steps: "early" equals "owner" in every output, terminal observation
    and array of get_state, the rng words among them.
(5) Shards of 64 + 256 envs equal the 320-env job under "early".
(6) Forced bails, LCR_COOP_MAX=0, 320 envs: the pair of launches under "early" against LCR_REDO_KERNEL=0 in lockstep -- the bailed waves leave through the out-of-line
    serve."""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_coop_ahead import _CONTACT, WAVE0, _assert_equal, _place, _snapshot
from tests.test_gpu_small_solve_slots import KINDS, LANE_KIND, _job, _tolerances

pytestmark = pytest.mark.gpu

SIZES = (256, 257, 320)
MODES = ("owner", "shared", "ahead", "early")
OWNING = (9, 9, 0) + _CONTACT[3:]     # a wave that owns patients in every substep and fewer than wave 0: two pinches and a finger on the cube
CASES = [("reach", "joint", "wave0"), ("push", "joint", "wave0"), ("push", "joint", "every")]


def _kinds(n, layout):
    other = _CONTACT if layout == "wave0" else OWNING
    return np.array([(WAVE0 if i < 64 else other)[i % 64] for i in range(n)])


_RUNS = {}


def _run(task, mode, layout, n, share):
    """the job of (1), once per case: the snapshots of the ten steps and, per wave, the patients solved through the "ahead" and the "early" entry summed over the run"""
    key = (task, mode, layout, n, share)
    if key not in _RUNS:
        from gym_lowcostrobot_amd import VecSim

        sim = VecSim(task, n, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, profile="wave_cycles", coop_share=share)
        waves = (n + 63) // 64
        shots, ahead, early = [], np.zeros(waves, np.int64), np.zeros(waves, np.int64)
        for a in _place(sim, task, mode, _kinds(n, layout)):
            sim.step(a)
            shots.append(_snapshot(sim))
            ac = sim.active_count.numpy()
            ahead += np.array([ac[64 * w + 3] if 64 * w + 3 < n else 0 for w in range(waves)], np.int64)   # (the one-lane wave of 257 envs has no lane 3 or 4)
            early += np.array([ac[64 * w + 4] if 64 * w + 4 < n else 0 for w in range(waves)], np.int64)
        sim.close()
        _RUNS[key] = (shots, ahead, early)
    return _RUNS[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task,mode,layout", CASES)
def test_share_modes_are_equal_and_the_early_entry_ran(hip_lib, task, mode, layout, n):
    ref = _run(task, mode, layout, n, "owner")[0]
    for s in ref:
        assert np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all()
    ahead, early = {}, {}
    for share in MODES[1:]:
        got, ahead[share], early[share] = _run(task, mode, layout, n, share)
        for t, (g, r) in enumerate(zip(got, ref)):
            _assert_equal(g, r, f"{task} {layout} n={n} step {t}, {share} against owner")
    print(f"[coop_early] {task} {layout} n={n}: patients solved per wave over ten steps, at the new claim points: early {early['early'].tolist()}, ahead {early['ahead'].tolist()};"
          f" after them by a wave without a patient: early {ahead['early'].tolist()}, ahead {ahead['ahead'].tolist()}")
    assert early["early"][1:4].min() > 0, early["early"]
    assert not early["ahead"].any() and not early["shared"].any(), (early["ahead"], early["shared"])
    if layout == "every":
        assert not ahead["ahead"].any(), ahead["ahead"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task,mode,layout", CASES)
def test_owner_run_against_the_oracle(hip_lib, task, mode, layout, n):
    kinds = _kinds(n, layout)
    qpos, qvel, lag, acts = _job(task, mode, kinds)
    sim, o = util.make_pair(task, n, preset="faithful", auto_reset=False, max_episode_steps=0, action_mode=mode, coop_share="owner")
    o.reset(seeds=np.arange(n)); sim.reset(seeds=np.arange(n))
    o.qpos[:] = qpos; o.qvel[:] = qvel; o.ee_lag[:] = lag
    for t, a in enumerate(acts * 2):
        dq, dv, ok, st = util.parity_step(sim, o, a, 4e-5, 4e-3, max_dq=3e-2, where=("coop_early", task, layout, n, t), carry=False)
        if t == 0 and layout == "every":   # the layout is what it says: every full wave has a finger or a proxy on the cube in its first lanes (oracle slots 12, 13, 16 with the cube)
            m = o.active_mask
            for w in range(n // 64):
                assert ((m[64 * w: 64 * w + 3] & 0x3000) != 0).sum() >= 2, (w, m[64 * w: 64 * w + 3])
        if t == 0 and layout == "wave0":   # wave 0's first eight lanes have a finger or a proxy on the cube, nobody else has
            m = o.active_mask
            assert ((m[:8] & 0x3000) != 0).sum() >= 7 and ((m[8:] & 0x3000) == 0).all(), (m[:8], np.nonzero(m[8:] & 0x3000)[0])
        if t in (0, len(acts) - 1):
            for k, name in enumerate(KINDS):
                sel = kinds == k
                if not sel.any():
                    continue
                tq, tv, share = _tolerances(task, name, int(sel.sum()))
                within = (dq[sel] <= tq) & (dv[sel] <= tv)
                print(f"[coop_early] {task} {layout} n={n} step {t + 1} {name}: {int(sel.sum())} envs, max |dq| {dq[sel].max():.2e} |dv| {dv[sel].max():.2e}, within {within.mean():.3f}")
                assert within.mean() >= share, (task, layout, n, t, name, np.sort(dq[sel])[-3:], np.sort(dv[sel])[-3:])
    sim.close()


@pytest.mark.parametrize("task,mode", [("push", "joint"), ("pick_place", "ee")])
def test_across_auto_resets(hip_lib, task, mode):
    from gym_lowcostrobot_amd import VecSim
    from oracle import orc

    n, steps = 320, 40
    runs = {}
    for share in ("owner", "early"):
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
    for t, (g, r) in enumerate(zip(runs["early"], runs["owner"])):
        _assert_equal(g, r, f"{task} step {t}, early against owner")


@pytest.mark.parametrize("task,mode,layout", CASES)
def test_shards_equal_the_whole_job(hip_lib, task, mode, layout):
    from gym_lowcostrobot_amd import VecSim

    whole = _run(task, mode, layout, 320, "early")[0]
    parts = []
    for off, m in ((0, 64), (64, 256)):
        sim = VecSim(task, m, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, profile="wave_cycles", coop_share="early",
                     env_id_offset=off, global_envs=320)
        shots = []
        for a in _place(sim, task, mode, _kinds(320, layout), off):
            sim.step(a)
            shots.append(_snapshot(sim))
        sim.close()
        parts.append(shots)
    for t, w in enumerate(whole):
        lo, hi = parts[0][t], parts[1][t]
        for k in w:
            if w[k] is not None:
                np.testing.assert_array_equal(w[k], np.concatenate([lo[k], hi[k]], axis=-1), err_msg=f"{task} {layout} step {t}: {k}")


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
        sims.append(VecSim(task, n, observation_mode="state", action_mode=mode, preset="faithful", auto_reset=False, max_episode_steps=0, diagnostics=True, coop_share="early"))
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
        _assert_equal(_snapshot(pair), _snapshot(legacy), f"step {t}, early with LCR_COOP_MAX=0 against LCR_REDO_KERNEL=0")
    pair.close(); legacy.close()
