"""Records tests/golden/broadphase_parent.npz: three scenes stepped with the device random
agent, for tests/test_gpu_broadphase.py to replay bit for bit.

Run it on the GPU against the library of the revision whose results are the yardstick:

  python tools/build_variant.py --rev=<parent> parent
  DX_LIB=variants/parent/libdx.so python tools/record_broadphase_golden.py

It refuses to write a golden without real contacts in it (MIN_CONTACT_FRACTION)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "broadphase_parent.npz")
SEED = 12345
# (key, domain, envs, control steps): reorient has the watch pass, auto-resets and 41
# cull items; bimanual 83 items (two item chunks), 36 pair chunks and a plane; Adroit
# reach 13 items and no plane
SCENES = (("reorient", "reorient", 32, 30), ("bimanual", "bimanual", 8, 20), ("adroit_reach", "reach", 16, 10))
MIN_CONTACT_FRACTION = 0.25  # of the reorient envs hold >= 1 contact at the final state


def run_scene(domain: str, nenv: int, steps: int) -> dict:
    """Steps `domain`.state_dense with the random agent and returns the final state, the
    task outputs and the final state's contact records (dx_forward on that state)."""
    from dexterity_amd import _lib, manipulation

    env = manipulation.load(domain, "state_dense", seed=SEED, num_envs=nenv)
    env.reset()
    for i in range(steps):
        env.step_random(i)
    ts = env.timestep()
    ph = env.physics
    out = {"qpos": ph.qpos, "qvel": ph.qvel, "reward": np.asarray(ts.reward), "discount": np.asarray(ts.discount),
           "step_type": np.asarray(ts.step_type)}
    ph.debug(True)
    ph.forward()
    ph.sync()
    ncon = ph.get(_lib.NCON)[:, 0].astype(np.int32)
    con = ph.debug_get("contact")
    keep = max(int(ncon.max()), 1)
    assert keep <= con.shape[1]
    con = con[:, :keep].copy()
    for e in range(nenv):  # records past an env's count are stale
        con[e, ncon[e]:] = 0
    out["ncon"] = ncon
    out["contact"] = con
    ph.debug(False)
    env.close()
    return out


def contact_fraction(ncon: np.ndarray) -> float:
    return float((ncon >= 1).mean())


def main():
    arrays = {}
    for key, domain, nenv, steps in SCENES:
        for name, a in run_scene(domain, nenv, steps).items():
            arrays[f"{key}/{name}"] = a
        n = arrays[f"{key}/ncon"]
        print(f"{key}: {nenv} envs x {steps} steps, contacts per env mean {n.mean():.2f} max {n.max()}, "
              f"envs with a contact {contact_fraction(n):.2f}")
    frac = contact_fraction(arrays["reorient/ncon"])
    if frac < MIN_CONTACT_FRACTION:
        sys.exit(f"refusing to write: only {frac:.2f} of the reorient envs hold a contact (need {MIN_CONTACT_FRACTION})")
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
