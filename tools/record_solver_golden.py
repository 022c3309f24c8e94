"""Records tests/golden/solver_parent.npz: the constraint-solver paths that the other
bit-exact goldens (guard_parent.npz, lane_parent.npz, broadphase_parent.npz) do not reach,
on the scenes of tests/pgs_cases.py, for tests/test_gpu_solver_golden.py to replay bit for
bit.

Run it on the GPU against the library of the revision whose results are the yardstick:

  python tools/build_variant.py --rev=<parent> parent
  DX_LIB=variants/parent/libdx.so python tools/record_solver_golden.py

Cases (CASES): key -> the scene (boxes, planes, parts, hinges), the solver, the tier the
physics steps run in and the path of dx_step.hip they pin:
  cg-lds-146     solve_cg with nv <= 30 and more than 128 rows (up to 128, nv <= 30 runs
                 solve_cg_reg), generic step kernel
  cg-chol-nv36   solve_cg's Cholesky M^-1 (nv > 30)
  cg-mid-144     solve_cg as compiled into the mid tier
  pgs-rows-224   solve_pgs's register-row sweep (more than NB*64 + 64 rows), mid tier, NB 2
  pgs-rows-288   the same in the overflow tier, NB 3
  pgs-chol-nv36, pgs-chol-nv36-mid   solve_pgs's LDS sweep (nv > 30), step kernel and mid tier
  pgs-blocks-128 solve_pgs_ar without a tail
One env per case: three physics steps from pgs_cases.settled_state, the first from a zero
warm start in a launch of its own, the other two in one launch (an env run from a substep
to the end of its control step), each from the state and warm start the one before left.
Stored per launch: the bytes of qpos | qvel | warm start | qacc, and the solver's iteration
count, the constraint-row count and the contact count of its last physics step.

The recorder refuses to write unless the run it records (the parent's own) took the
intended path, by what the library reports (as tests/test_gpu_pgs_dispatch.py): the first
launch has the table's contact and row counts; every launch's last physics step has at
least one solver iteration, no overflow, no divergence, and counts that select the case's
path (path_ok); the tier shows in the health counters -- contact_deferred, and for the mid
tier deferred_behind_launch == 0 (one env per launch; a launch whose deferral the overflow
tier took behind it is done again, three times at the most).
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "solver_parent.npz")
SWITCHES = ("DX_NO_MID", "DX_DEFER_AT", "DX_MID_DEFER_AT", "DX_GENERIC_KERNEL", "DX_NO_QUEUE")
LAUNCHES = (1, 2)  # physics steps per launch
STEP_POOL, MID_POOL = 32, 64  # contacts the step kernel / the mid tier hold (tests/pgs_cases.py)
PGS_AR = 64  # rows per register block of solve_pgs_ar
# key: scene, solver, tier, NB (PGS register blocks of the tier), nv, contacts, rows, path
CASES = {
    "cg-lds-146": dict(spec=(2, 4, 0, 18), solver="CG", tier="step", NB=2, nv=30, ncon=32, nefc=146, path="cg-lds"),
    "cg-chol-nv36": dict(spec=(6, 1, 0, 0), solver="CG", tier="step", NB=2, nv=36, ncon=24, nefc=96, path="chol"),
    "cg-mid-144": dict(spec=(1, 9, 0, 0), solver="CG", tier="mid", NB=2, nv=6, ncon=36, nefc=144, path="cg-lds"),
    "pgs-rows-224": dict(spec=(2, 7, 0, 0), solver="PGS", tier="mid", NB=2, nv=12, ncon=56, nefc=224, path="rows"),
    "pgs-rows-288": dict(spec=(2, 9, 0, 0), solver="PGS", tier="hi", NB=3, nv=12, ncon=72, nefc=288, path="rows"),
    "pgs-chol-nv36": dict(spec=(6, 1, 0, 0), solver="PGS", tier="step", NB=2, nv=36, ncon=24, nefc=96, path="chol"),
    "pgs-chol-nv36-mid": dict(spec=(6, 2, 0, 0), solver="PGS", tier="mid", NB=2, nv=36, ncon=48, nefc=192, path="chol"),
    "pgs-blocks-128": dict(spec=(1, 8, 0, 0), solver="PGS", tier="step", NB=2, nv=6, ncon=32, nefc=128, path="blocks"),
}
FIELDS = ("state", "niter", "nefc", "ncon")


def path_ok(case: dict, nv: int, ncon: int, nefc: int) -> bool:
    """Whether a physics step with these counts runs in the case's tier and solver path."""
    tier = {"step": ncon <= STEP_POOL, "mid": STEP_POOL < ncon <= MID_POOL, "hi": ncon > MID_POOL}[case["tier"]]
    path = {"cg-lds": nv <= 30 and nefc > 2 * PGS_AR, "chol": nv > 30,
            "rows": nv <= 30 and nefc > case["NB"] * PGS_AR + PGS_AR,
            "blocks": nv <= 30 and nefc <= case["NB"] * PGS_AR}[case["path"]]
    return tier and path


def _launch(physics, cm, q, v, w, nsub):
    from dexterity_amd import _lib

    ph = physics.BatchedPhysics(physics.Model(cm), 1)
    ph.set(_lib.QPOS, q[None])
    ph.set(_lib.QVEL, v[None])
    ph.set(_lib.QACC_WARMSTART, w[None])
    ph.debug(True)
    ph.health_clear()
    ph.step(nsub)
    ph.sync()
    efc = ph.debug_get("efc_count")
    out = dict(qpos=ph.qpos[0].astype(np.float32), qvel=ph.qvel[0].astype(np.float32),
               warm=ph.get(_lib.QACC_WARMSTART)[0], qacc=ph.get(_lib.QACC)[0],
               niter=int(ph.get(_lib.NITER)[0, 0]), ncon=int(ph.get(_lib.NCON)[0, 0]),
               nefc=int(efc[0, 0]), row_overflow=int(efc[0, 1]), health=ph.health(),
               timeouts=int(ph.debug_get("queue_timeouts")[0]))
    ph.close()
    return out


def run_case(key: str) -> dict:
    """Runs the case's launches; returns per launch the state bytes (qpos | qvel | warm
    start | qacc, float32) and the counts, after asserting that this run took the case's
    path."""
    from dexterity_amd import physics
    from oracle import oracle
    from tests import pgs_cases as pc

    case = CASES[key]
    oracle.build()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            cm = pc.scene(*case["spec"], tmp_path=tmp).with_solver(case["solver"])
        assert int(cm.nv) == case["nv"], (key, cm.nv)
        q, v = pc.settled_state(oracle, cm)
        q, v, w = q.astype(np.float32), v.astype(np.float32), np.zeros(cm.nv, dtype=np.float32)
        out = {f: [] for f in FIELDS}
        for n, nsub in enumerate(LAUNCHES):
            for _ in range(3):
                o = _launch(physics, cm, q, v, w, nsub)
                if case["tier"] != "mid" or o["health"]["deferred_behind_launch"] == 0:
                    break
            h = o["health"]
            print(f"{key} launch {n} ({nsub} physics steps): contacts {o['ncon']} rows {o['nefc']} "
                  f"iterations {o['niter']} deferred {h['contact_deferred']} behind launch {h['deferred_behind_launch']}")
            assert o["timeouts"] == 0 and o["row_overflow"] == 0, (key, o)
            assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, (key, h)
            if n == 0:
                assert (o["ncon"], o["nefc"]) == (case["ncon"], case["nefc"]), (key, o["ncon"], o["nefc"])
            assert o["niter"] >= 1 and path_ok(case, int(cm.nv), o["ncon"], o["nefc"]), (key, o["niter"], o["ncon"], o["nefc"])
            # the tier: one deferral per launch (the env goes to the end of its control step
            # where it was taken), none from the step kernel's own pool
            assert h["contact_deferred"] == (0 if case["tier"] == "step" else 1), (key, h)
            if case["tier"] == "mid":
                assert h["deferred_behind_launch"] == 0 and h["mid_tier_gave_up"] == 0, (key, h)
            q, v, w = o["qpos"], o["qvel"], o["warm"]
            out["state"].append(np.concatenate([o["qpos"], o["qvel"], o["warm"], o["qacc"]]).astype(np.float32))
            for f in ("niter", "nefc", "ncon"):
                out[f].append(o[f])
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return {"state": np.stack(out["state"]).view(np.uint8),
            **{f: np.array(out[f], dtype=np.int32) for f in ("niter", "nefc", "ncon")}}


def main():
    arrays = {}
    for key in CASES:
        for name, a in run_case(key).items():
            arrays[f"{key}/{name}"] = a
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
