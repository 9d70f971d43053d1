"""Where a wave of the Newton kernels spends its cycles (lcr_config.diagnostics = 2, VecSim profile="wave_cycles"; GPU box): per control step and wave -- total,
inside the Newton solves, inside COUPLED solves (envs with touching bodies solved cooperatively by the wave, or substeps in the coupled SIMT copy), how many of
each, Newton iterations executed; mean wave against the slowest wave of each step (the launch ends with the slowest).     python tools/newton_phases.py [task ...] [--n 65536]"""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

from gym_lowcostrobot_amd import VecSim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("tasks", nargs="*", default=["reach", "push", "lift", "pick_place_ee", "stack", "push_loop"])
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--coop-share", default=None, choices=["owner", "shared", "handoff", "ahead", "early"])   # (None: the library's default)
a = ap.parse_args()
for name in a.tasks:
    mode = "ee" if name.endswith("_ee") else "joint"
    task = name.replace("_ee", "")
    sim = VecSim(task, a.n, action_mode=mode, profile="wave_cycles", coop_share=a.coop_share)
    bufs = [sim.alloc_actions() for _ in range(16)]
    for i, b in enumerate(bufs):
        sim.fill_random_actions(b, 0, i)
    for i in range(60):
        sim.step_device(bufs[i % 16].ptr)
    rows = []
    for i in range(20):
        sim.step_device(bufs[i % 16].ptr)
        sim.sync()
        tot, solve, cpl, ch = (x.numpy()[::64].astype(np.float64) for x in (sim.max_sweeps, sim.active_mask, sim.active_count, sim.choice))
        # (one-cube Newton kernel, four-wave workgroups: lane 1 of active_count = cycles spent on other waves' patients, lane 2 = own patients other waves solved)
        ac = sim.active_count.numpy().astype(np.float64)
        rows.append((tot, solve, cpl, np.mod(np.floor(ch / 65536.0), 256.0), np.mod(ch, 65536.0), np.floor(ch / 16777216.0), ac[1::64], ac[2::64], ac[3::64], ac[4::64], ac[5::64]))
    tot, solve, cpl, ncpl, its, nslow, helpc, handed, ahead, early, wait = (np.stack([r[k] for r in rows]) for k in range(11))   # [step][wave]
    slow = tot.argmax(1)
    pick = lambda x: x[np.arange(len(slow)), slow].mean()
    print(f"{name:14s} n={a.n}: cycles per control step and wave, MEAN wave | SLOWEST wave of the step (mean over 20 steps)")
    print(f"   total            {tot.mean():10.0f} | {pick(tot):10.0f}     mean / slowest = {tot.mean() / pick(tot):.2f}")
    print(f"   Newton solves    {solve.mean():10.0f} | {pick(solve):10.0f}     ({100 * solve.mean() / tot.mean():.0f} % | {100 * pick(solve) / pick(tot):.0f} % of the wave's cycles; the rest: set-up, integration, reward)")
    print(f"   coupled solves   {cpl.mean():10.0f} | {pick(cpl):10.0f}     (cooperative solves + whole solves of substeps in the coupled SIMT copy); waves with any: {100 * (cpl > 0).mean():.0f} %")
    if True:   # envs solved cooperatively (summed over the substeps); substeps the wave spent in the coupled SIMT copy
        print(f"   substeps in the coupled SIMT copy: {nslow.mean():.2f} | {pick(nslow):.2f}; waves with any: {100 * (nslow > 0).mean():.1f} %; cooperative solves per wave and step: {ncpl.mean():.2f} | {pick(ncpl):.2f}, most {ncpl.max():.0f}")
        srt = np.sort(tot.max(0))[::-1]
        print(f"   slowest waves (max over the steps), cycles: {' '.join(f'{v:.0f}' for v in srt[:6])};  p99 {np.percentile(tot, 99):.0f}  p90 {np.percentile(tot, 90):.0f}  p50 {np.percentile(tot, 50):.0f}")
    if task != "stack" and task != "push_loop":
        print(f"   cooperative cycles left on the owner's path (coupled solves above); cycles helping other waves {helpc.mean():10.0f} | {pick(helpc):10.0f};"
              f" own patients handed off {handed.mean():.2f} | {pick(handed):.2f} of {ncpl.mean():.2f} | {pick(ncpl):.2f}")
        # what handing off can still win: the launch cannot end before the wave with the most cycles OUTSIDE its own-path cooperative passes
        at = lambda q: np.abs(tot - np.percentile(tot, q, axis=1, keepdims=True)).argmin(1)   # per step: the wave at that percentile of the totals
        w99, w90 = at(99), at(90)
        rest = (tot - cpl).max(1).mean()
        print(f"   own-path cooperative cycles of the slowest | p99 | p90 wave of a step: {pick(cpl):.0f} | {cpl[np.arange(len(w99)), w99].mean():.0f} | {cpl[np.arange(len(w90)), w90].mean():.0f}"
              f" (their totals {pick(tot):.0f} | {tot[np.arange(len(w99)), w99].mean():.0f} | {tot[np.arange(len(w90)), w90].mean():.0f});"
              f" largest total - own-path cooperative {rest:.0f}: ceiling {pick(tot) - rest:.0f} = {100 * (pick(tot) - rest) / pick(tot):.1f} % of the slowest wave")
        hs = helpc[np.arange(len(slow)), slow]
        print(f"   slowest wave of a step: helping cycles above its own-path cooperative cycles in {100 * (hs > cpl[np.arange(len(slow)), slow]).mean():.0f} % of the steps")
        # (lane 5) what an earlier claim by the helpers can remove: the slowest wave's own-path cooperative cycles after the last pass in which it solved a patient of its own
        print(f"   own-path cooperative cycles after the wave's last pass over patients of its own (waiting for the waves that hold the rest): {wait.mean():.0f} | {pick(wait):.0f}"
              f" = {100 * pick(wait) / max(pick(cpl), 1):.0f} % of the slowest wave's own-path cooperative cycles, {100 * pick(wait) / pick(tot):.1f} % of its total")
        if a.coop_share in (None, "early"):   # (lane 4 carries the counter under that mode only)
            print(f"   patients solved for waves at an earlier substep at the claim points before / between the small solves and after the wave's own patients: {early.mean():.2f} | {pick(early):.2f}, most {early.max():.0f}; waves with any: {100 * (early > 0).mean():.0f} %")
        if a.coop_share in (None, "ahead", "early"):   # (lane 3 carries the counter under these modes only)
            print(f"   patients solved for waves at an earlier substep while the wave had none of its own: {ahead.mean():.2f} | {pick(ahead):.2f}, most {ahead.max():.0f}; waves with any: {100 * (ahead > 0).mean():.0f} %")
    print(f"   Newton iterations executed by the wave: {its.mean():.1f} | {pick(its):.1f};  cycles per iteration (solves / iterations): {solve.sum() / max(its.sum(), 1):.0f}", flush=True)
    sim.close()
