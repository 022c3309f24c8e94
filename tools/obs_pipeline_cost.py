"""Cost of the observation pipeline: reorient at 4096 envs, 1000 control
steps of dx_env_step_random per case behind 30 warm-up steps, two rounds in one process.
Prints one JSON line per case and round: ms per control step (wall clock over the timed
steps, one synchronisation at the end) and the step kernel's own time (HIP events around
every 10th launch).

    python tools/obs_pipeline_cost.py [--envs 4096] [--steps 1000] [--warmup 30] [--rounds 2]
"""

import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dexterity_amd import _lib, manipulation  # noqa: E402

CASES = (
    ("off", None),
    ("(m, d, K) = (1, 0, 1): the launch alone", dict(update_interval=5, delay=0, buffer_size=1)),
    ("(1, 2, 4)", dict(update_interval=5, delay=10, buffer_size=4)),
    ("(1, 2, 4) with noise", dict(update_interval=5, delay=10, buffer_size=4, noise_std=0.01)),
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
            if cfg:
                env.configure_observations(**cfg)
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
            dims = (ctypes.c_int32 * 3)()
            _lib.check(L.dx_env_obs_pipe_dims(env.ptr, dims))
            W, K = dims[0], dims[1]
            print(json.dumps({
                "config": f"3 reorient {a.envs}, observation pipeline: {name}", "envs": a.envs,
                "ms_per_step": round(1e3 * dt / a.steps, 4), "env_steps_per_s": round(a.envs * a.steps / dt, 1),
                "step_kernel_ms_avg": round(ms.value / max(cnt.value, 1), 4), "step_kernel_launches_timed": cnt.value,
                "row_floats": W, "rows_delivered": K,
                # one sample in (source row read, ring row written) and K rows out (ring read, buffer written)
                "pipeline_bytes_per_env_step": (4 * W + 4 * ((W + 31) // 32 * 32) + K * 4 * ((W + 31) // 32 * 32)
                                                + K * 4 * W) if cfg else 0,
                "contact_deferred": env.physics.health()["contact_deferred"]}), flush=True)
            env.close()


if __name__ == "__main__":
    main()
