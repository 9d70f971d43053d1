"""GPU: bench.py itself -- what a plain run measures and reports, and the outputs it dumps for comparing two builds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("obs", ["state", "both"])
def test_bench_plain_run_and_dumped_outputs(hip_lib, tmp_path, obs):
    """a plain bench.py run times exactly --steps steps and prints the headline alone; --dump-outputs writes what the last timed step returned,
    and the same arguments give the same arrays whatever the time-bounded clock prewarm did before the W + K steps"""
    got = []
    for r, prewarm in enumerate(("0", "30")):
        d = tmp_path / f"run{r}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--envs-per-gpu", "4096", "--obs", obs,
               "--prewarm-ms", prewarm, "--dump-outputs", str(d)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout
        j = json.loads(lines[0])
        assert j["metric"] == "env-steps/sec" and j["unit"] == "env-steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
        assert j["steps"] == 7 and j["warmup"] == 3 and j["value"] == pytest.approx(4096 * 7 / (j["ms_per_step"] * 7e-3), rel=1e-6)
        assert not {"cpu_baseline", "preset_fast", "baseline_sharded_configs", "repeats", "hdf5", "state_finite"} & set(j)
        files = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert sorted(files) == j["dump_outputs"]["arrays"]
        assert all(a.dtype in (np.float32, np.float64) for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64e6
        assert files["arm_qpos"].shape == (4096, 6) and files["reward"].shape == (4096,) and files["terminal_obs"].shape == (4096, 18)
        assert np.isfinite(files["arm_qpos"]).all() and np.isfinite(files["cube_pos"]).all()
        if obs == "both":
            assert files["image_front"].shape == (16, 240, 320, 3) and files["image_top"].std() > 5
        got.append(files)
    assert sorted(got[0]) == sorted(got[1])
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
