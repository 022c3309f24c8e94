"""Records tests/golden/guard_parent.npz: the kernels and paths that
tests/golden/broadphase_parent.npz does not reach, stepped with the device random agent,
for tests/test_gpu_guard_golden.py to replay bit for bit.

Run it on the GPU against the library of the revision whose results are the yardstick:

  python tools/build_variant.py --rev=<parent> parent
  DX_LIB=variants/parent/libdx.so python tools/record_guard_golden.py

Cases (CASES): reorient with the CG and the PGS specializations; the two reach scenes
(Shadow: contacts disabled; Adroit) with a time limit that ends the episode inside the
window, so that the auto-reset runs; reorient on the generic kernel; reorient with every
contact step forced to the mid tier, and through it to the overflow tier; reorient at 64
envs x 10 control steps.

The recorder refuses to write unless, on the run it records (the parent's own):
  * the forced-tier cases deferred steps (health counter contact_deferred; with
    DX_MID_DEFER_AT=0 the mid tier passes every step that has a contact on to the overflow
    tier);
  * each reach case saw an episode end (step type LAST) before the final step;
  * the 64-env case holds, among the env-substeps it can see, one with more than 64
    constraint rows, one with the fewest rows the scene can have and one with no contact.
    The scene's 24 dof friction-loss rows are always there (make_constraint, rows
    [0, nfric)), so "no constraint row" cannot occur on it: the census asks for an
    env-substep with those rows alone (no limit row, no contact row).  The library exports
    the row count of an env's last physics step only (dx_debug_get "efc_count", after a
    control step with the debug record on), so the census covers the last substep of every
    control step, taken in a second, identical run with the debug record on (the record
    adds stores only; the recorder checks that both runs end in the same state).  When 64
    envs do not hold such states the env count is doubled (CENSUS_ENVS) until they do; the
    golden carries the count it was recorded at.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "guard_parent.npz")
SEED = 4321
ENV_VARS = ("DX_GENERIC_KERNEL", "DX_DEFER_AT", "DX_MID_DEFER_AT", "DX_NO_MID")
REACH_LIMIT = 0.09  # s: the fifth 0.02 s control step reaches it, the sixth starts a new episode
# key: domain, envs, control steps, solver, environment variables, time limit
CASES = {
    "reorient_cg": dict(domain="reorient", nenv=16, steps=6, solver="CG"),
    "reorient_pgs": dict(domain="reorient", nenv=16, steps=6, solver="PGS"),
    "reach_shadow": dict(domain="reach_shadow", nenv=16, steps=8, time_limit=REACH_LIMIT),
    "reach_adroit": dict(domain="reach", nenv=16, steps=8, time_limit=REACH_LIMIT),
    "reorient_generic": dict(domain="reorient", nenv=16, steps=6, env={"DX_GENERIC_KERNEL": "1"}),
    "reorient_mid": dict(domain="reorient", nenv=16, steps=6, env={"DX_DEFER_AT": "0"}),
    "reorient_overflow": dict(domain="reorient", nenv=16, steps=6, env={"DX_DEFER_AT": "0", "DX_MID_DEFER_AT": "0"}),
    "reorient_64": dict(domain="reorient", nenv=64, steps=10),
}
CENSUS_ENVS = (64, 128, 256)
LAST = 2  # StepType.LAST
# the health counters that do not depend on timing (how many deferrals the mid tier took
# before its launch ended does)
HEALTH = ("contact_overflow", "row_overflow", "diverged", "contact_deferred")


def run_case(domain, nenv, steps, solver=None, env=None, time_limit=None, census=False) -> dict:
    """Steps the case and returns the final state, the task outputs, the step types after
    every control step, the health counters and the final state's contact records
    (dx_forward on that state).  `census`: the debug record on from the start, and the
    contact and constraint-row counts after every control step returned too."""
    from dexterity_amd import _lib, manipulation

    saved = {k: os.environ.pop(k, None) for k in ENV_VARS}
    os.environ.update(env or {})
    try:
        task = manipulation.SUITE[(domain, "state_dense")]()
        if solver:
            task.compiled = task.compiled.with_solver(solver)
        e = manipulation.GoalEnvironment(task, num_envs=nenv, seed=SEED, time_limit=time_limit)
    finally:
        for k in ENV_VARS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    ph = e.physics
    if census:
        ph.debug(True)
    e.reset()
    types, ncons, nefcs = [], [], []
    for i in range(steps):
        e.step_random(i)
        types.append(np.asarray(e.timestep().step_type).astype(np.int32))
        if census:
            ncons.append(ph.get(_lib.NCON)[:, 0].astype(np.int32))
            nefcs.append(ph.debug_get("efc_count")[:, 0].astype(np.int32))
    ts = e.timestep()
    h = ph.health()
    out = {"qpos": ph.qpos, "qvel": ph.qvel, "warmstart": ph.get(_lib.QACC_WARMSTART),
           "reward": np.asarray(ts.reward), "discount": np.asarray(ts.discount),
           "step_types": np.stack(types),
           "observation": np.concatenate([np.asarray(v).reshape(nenv, -1) for v in ts.observation.values()], axis=1),
           "health": np.array([h[k] for k in HEALTH], dtype=np.int64)}
    ph.debug(True)
    ph.forward()
    ph.sync()
    ncon = ph.get(_lib.NCON)[:, 0].astype(np.int32)
    keep = max(int(ncon.max()), 1)
    if ncon.max() > 0:
        con = ph.debug_get("contact")
        assert keep <= con.shape[1]
        con = con[:, :keep].copy()
    else:  # (a scene with contacts disabled has no record to read)
        con = np.zeros((nenv, 1, 16), dtype=np.float32)
    for k in range(nenv):  # records past an env's count are stale
        con[k, ncon[k]:] = 0
    out["ncon"] = ncon
    out["contact"] = con
    ph.debug(False)
    e.close()
    if census:
        out["census_ncon"], out["census_nefc"] = np.stack(ncons), np.stack(nefcs)
        out["nfric"] = int((np.asarray(task.compiled.arrays["dof_frictionloss"]).ravel() > 0).sum())
    return out


def check_parent_run(key: str, out: dict) -> None:
    """What the golden must hold, asserted on the recording run."""
    h = dict(zip(HEALTH, (int(v) for v in out["health"])))
    assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, (key, h)
    if key in ("reorient_mid", "reorient_overflow"):
        assert h["contact_deferred"] > 0, (key, h)
    if key.startswith("reach_"):
        assert (out["step_types"][:-1] == LAST).any(), f"{key}: no episode ended inside the window"
        assert (out["step_types"][-1] != LAST).all(), f"{key}: the window ends on an episode end"


def census_ok(nefc: np.ndarray, ncon: np.ndarray, nfric: int) -> bool:
    return bool((nefc > 64).any() and (nefc == nfric).any() and (ncon == 0).any())


def main():
    arrays = {}
    for key, case in CASES.items():
        if key == "reorient_64":
            continue
        out = run_case(**case)
        check_parent_run(key, out)
        n = out["ncon"]
        print(f"{key}: contacts per env mean {n.mean():.2f} max {n.max()}, health {out['health'].tolist()}, "
              f"step types seen {sorted(set(out['step_types'].ravel().tolist()))}")
        for name, a in out.items():
            arrays[f"{key}/{name}"] = a
    # the 64-env case and its census, on a second run of the same (parent) library
    for nenv in CENSUS_ENVS:
        case = dict(CASES["reorient_64"], nenv=nenv)
        out = run_case(**case)
        check_parent_run("reorient_64", out)
        c = run_case(census=True, **case)
        for name in ("qpos", "qvel", "warmstart", "reward", "contact"):
            assert c[name].tobytes() == out[name].tobytes(), f"the census run differs in {name}"
        nefc, ncon, nfric = c["census_nefc"], c["census_ncon"], c["nfric"]
        print(f"reorient_64 at {nenv} envs, census over {nefc.size} env-substeps (the last of each control step): "
              f"rows min {nefc.min()} max {nefc.max()}, > 64 rows {(nefc > 64).sum()}, the {nfric} friction rows alone "
              f"{(nefc == nfric).sum()}, no contact {(ncon == 0).sum()}, health {out['health'].tolist()}")
        if census_ok(nefc, ncon, nfric):
            break
    else:
        sys.exit("refusing to write: no env count holds an env-substep with > 64 rows, one with the friction rows "
                 "alone and one with no contact")
    for name, a in out.items():
        arrays[f"reorient_64/{name}"] = a
    arrays["reorient_64/census_nefc"], arrays["reorient_64/census_ncon"] = nefc, ncon
    arrays["reorient_64/nfric"] = np.int32(nfric)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
