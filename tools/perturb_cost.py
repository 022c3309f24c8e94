"""Cost of the per-env applied wrenches and of the random pushes: reorient
at 4096 envs, 1000 control steps of dx_env_step_random per case behind 30 warm-up steps, two
rounds in one process.  Prints one JSON line per case and round: ms per control step (wall
clock over the timed steps, one synchronisation at the end) and the step kernel's own time
(HIP events around every 10th launch).

    python tools/perturb_cost.py [--envs 4096] [--steps 1000] [--warmup 30] [--rounds 2]
"""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dexterity_amd import _lib, manipulation  # noqa: E402

PUSH = dict(bodies=("prop",), probability=0.25, force_range=(0.1, 0.6), torque_range=(0.0, 0.002), duration_steps=3)
CASES = (
    ("off (shared gravity compensation)", None),
    ("per-env rows equal to the shared array, no pushes", "rows"),
    ("pushes on the prop, probability 0", dict(PUSH, probability=0.0)),
    ("pushes on the prop, probability 0.25 x 3 steps", PUSH),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    L = _lib.load()
    for _ in range(a.rounds):
        for name, cfg in CASES:
            env = manipulation.load("reorient", "state_dense", seed=1, num_envs=a.envs)
            if cfg == "rows":
                rows = np.repeat(np.asarray(env.task.gravity_compensation, np.float32)[None], a.envs, axis=0)
                env.physics.set_xfrc(rows)
            elif cfg:
                env.configure_perturbations(**cfg)
            env.reset()
            for k in range(a.warmup):
                env.step_random(k)
            env.physics.sync()
            env.physics.health_clear()
            _lib.check(L.dx_timing_enable(env.physics.ptr, 10))
            t0 = time.perf_counter()
            for k in range(a.warmup, a.warmup + a.steps):
                env.step_random(k)
            env.physics.sync()
            dt = time.perf_counter() - t0
            ms, cnt = ctypes.c_double(), ctypes.c_int32()
            _lib.check(L.dx_timing_read(env.physics.ptr, ctypes.byref(ms), ctypes.byref(cnt)))
            _lib.check(L.dx_timing_enable(env.physics.ptr, 0))
            pushed = float(np.abs(env.applied_perturbations()).sum(axis=(1, 2)).astype(bool).mean()) if isinstance(cfg, dict) else 0.0
            print(json.dumps({
                "config": f"3 reorient {a.envs}, applied wrenches: {name}", "envs": a.envs,
                "ms_per_step": round(1e3 * dt / a.steps, 4), "env_steps_per_s": round(a.envs * a.steps / dt, 1),
                "step_kernel_ms_avg": round(ms.value / max(cnt.value, 1), 4), "step_kernel_launches_timed": cnt.value,
                "per_env_mode": env.physics.xfrc_ptr() is not None, "envs_pushed_at_the_end": round(pushed, 4),
                "contact_deferred": env.physics.health()["contact_deferred"]}), flush=True)
            env.close()


if __name__ == "__main__":
    main()
