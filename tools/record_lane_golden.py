"""Records tests/golden/lane_parent.npz: reorient (Newton) at 256 envs x 12 control steps
with the device random agent, for tests/test_gpu_lane_golden.py to replay.  The goldens of
tools/record_guard_golden.py and tools/record_broadphase_golden.py hold 16 to 64 envs; this
one widens the set of states a scaffolding change of the step kernel is checked on, at
1 KB: per env one CRC32 of the final

  qpos | qvel | warm start | observation | reward | discount | step_type

bytes.  Run it on the GPU against the library of the revision whose results are the
yardstick:

  python tools/build_variant.py --rev=<parent> parent
  DX_LIB=variants/parent/libdx.so python tools/record_lane_golden.py

The recorder refuses to write unless, on the run it records (the parent's own), the
fraction of envs that hold a contact at the final state meets
record_broadphase_golden.MIN_CONTACT_FRACTION and at least one env ended an episode (step
type LAST, the auto-reset follows) before the final step.  It tries SEEDS in order and the
golden carries the seed it was recorded with."""
import importlib.util
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "lane_parent.npz")
NENV, STEPS = 256, 12
SEEDS = (97531, 97532, 97533, 97534)
LAST = 2  # StepType.LAST


def _broadphase_recorder():
    spec = importlib.util.spec_from_file_location(
        "record_broadphase_golden", os.path.join(ROOT, "tools", "record_broadphase_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BP = _broadphase_recorder()


def run_case(seed: int, nenv: int = NENV, steps: int = STEPS) -> dict:
    """Steps the case; per-env CRC32 of the final state and task outputs, the final contact
    counts, the step types after every control step and the health counters."""
    from dexterity_amd import _lib, manipulation

    env = manipulation.load("reorient", "state_dense", seed=seed, num_envs=nenv)
    env.reset()
    types = []
    for i in range(steps):
        env.step_random(i)
        types.append(np.asarray(env.timestep().step_type).astype(np.int32).reshape(nenv))
    ts = env.timestep()
    ph = env.physics
    parts = [ph.qpos, ph.qvel, ph.get(_lib.QACC_WARMSTART),
             np.concatenate([np.asarray(v).reshape(nenv, -1) for v in ts.observation.values()], axis=1),
             np.asarray(ts.reward), np.asarray(ts.discount), np.asarray(ts.step_type)]
    parts = [np.ascontiguousarray(np.asarray(p).reshape(nenv, -1)) for p in parts]
    crc = np.array([zlib.crc32(b"".join(p[k].tobytes() for p in parts)) for k in range(nenv)], dtype=np.uint32)
    ncon = ph.get(_lib.NCON)[:, 0].astype(np.int32)
    health = ph.health()
    env.close()
    return {"crc": crc, "ncon": ncon, "step_types": np.stack(types), "health": dict(health)}


def parent_run_ok(out: dict) -> tuple:
    frac = BP.contact_fraction(out["ncon"])
    resets = int((out["step_types"][:-1] == LAST).any(axis=0).sum())
    return frac >= BP.MIN_CONTACT_FRACTION and resets >= 1, frac, resets


def main():
    for seed in SEEDS:
        out = run_case(seed)
        ok, frac, resets = parent_run_ok(out)
        print(f"seed {seed}: envs with a contact {frac:.2f}, envs that auto-reset inside the window {resets}, "
              f"health {out['health']}")
        if ok:
            break
    else:
        sys.exit(f"refusing to write: no seed gives a contact fraction >= {BP.MIN_CONTACT_FRACTION} and an auto-reset")
    again = run_case(seed)
    assert again["crc"].tobytes() == out["crc"].tobytes(), "the run does not repeat itself"
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, crc=out["crc"], seed=np.int64(seed), contact_fraction=np.float32(frac), auto_resets=np.int32(resets))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
