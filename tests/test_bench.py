"""bench.py's command line: the plain result line and --dump-outputs."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS, STEPS, WARMUP = 64, 3, 2


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--envs-per-gpu", str(N_ENVS), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run prints one line with the headline only (nothing of --full), times
    exactly --steps steps, and writes the last step's outputs as float32 arrays that a
    second run with the same arguments reproduces bit for bit."""
    from dexterity_amd import build

    build.build()
    a = _run(tmp_path / "a")
    b = _run(tmp_path / "b")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in a
    assert a["steps"] == STEPS and a["warmup"] == WARMUP
    assert a["health"]["env_substeps"] == N_ENVS * STEPS * a["config"]["substeps_per_env_step"]
    assert a["value"] == pytest.approx(N_ENVS * 1e3 / a["ms_per_step"], rel=1e-3)
    for key in ("roofline", "host_api", "cpu_baseline", "cpu_baseline_extra"):
        assert key not in a
    shapes = {"observation": (N_ENVS, 123), "reward": (N_ENVS,), "discount": (N_ENVS,), "step_type": (N_ENVS,),
              "qpos": (N_ENVS, 31), "qvel": (N_ENVS, 30)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in shapes)
    for name, shape in shapes.items():
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and x.shape == shape
        assert np.all(np.isfinite(x))
        assert np.array_equal(x, y), name
