"""Records tests/golden/newton_parent.npz: the Newton solves that the other goldens do not
reach, for tests/test_gpu_newton_rows.py to replay bit for bit.  The change it was recorded
for is the exact line search's register slots (dx_step.hip line_search, Ctx::ls_slots: a
scene specialization keeps its own row bound, three slots in reorient).  Its cases were
chosen for a wider change of the Newton path (the rows' forces and Hessian weights stored
once per iterate), which was measured and not kept; they stay as the
yardstick for whoever changes solve, jac_t_force, build_hessian_inc or line_search next.
Not covered: no case runs a specialization's line search with more than 128 rows (the
reorient cases have at most 100; boxes_140 is a scene no specialization matches, so its
third slot is the generic kernel's, which keeps five).

Run it on the GPU against the library of the revision whose results are the yardstick:

  python tools/build_variant.py --rev=<parent> parent
  DX_LIB=variants/parent/libdx.so python tools/record_newton_golden.py

Cases:
  * reorient_64: 64 reorient envs x 6 control steps with the device random agent, the debug
    record on from the start (it adds stores only).  After every control step the census
    takes each env's contact count, row count and Newton iteration count of its last
    physics step.
  * fric_zones: the reorient hand at 0.1, 0.25, 0.4 and 0.5 of every limited joint's range,
    the cube away from it, random joint velocities up to 0.5 rad/s, gravity compensated: a
    forward pass and PHYS_SUBSTEPS substeps.  In an env without contact and without limit
    row the constraint force is the friction-loss rows' alone, M qacc - qfrc_smooth from the
    library's own record, so a dof whose force is +floss or -floss has its row in that
    linear zone.
  * limit_contact: the hand at 0.5 and 0.4 of the ranges, where it touches itself, with its
    first two limited joints (the wrist's) 5 mrad below their range in env 0 and above it in
    env 1: joints on their limits while contacts are active.
  * box_rest: a free cube with friction loss on its six dofs, no gravity, at rest in the
    air: the warm start is the solution, so the solve leaves at the gradient test with no
    iteration, on six rows.
  * boxes_140: two such cubes on four coincident planes (the scene of
    tools/record_rows_golden.py's boxes_72 with fewer planes): 32 contacts, the step
    kernel's whole pool, and 12 + 128 rows, on the generic kernel -- the line search's third
    register slot.

The recorder refuses to write unless, on the run it records (the parent's own):
  * reorient_64's census holds a solve of 1 iteration and one of >= 4, a solve with 65..128
    rows;
  * limit_contact's forward pass has an env with contacts and more rows than its friction
    rows and four per contact (nefc - nfric - 4 ncon > 0);
  * fric_zones has an env with no contact and the friction rows alone in which one dof's
    constraint force is +floss and another's -floss (to 1e-3 of floss);
  * box_rest ends every solve with 0 iterations on 6 rows;
  * boxes_140 has 129..176 rows with at most 32 contacts in its forward pass, deferred no
    step and overflowed nothing.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "newton_parent.npz")
ENV_CASE = dict(domain="reorient", nenv=64, steps=6)
PHYS_CASES = ("fric_zones", "limit_contact", "box_rest", "boxes_140")
PHYS_SUBSTEPS = 3
RANGE_FRACTIONS = (0.1, 0.25, 0.4, 0.5)
LIMIT_FRACTIONS = (0.5, 0.4)  # limit_contact: where fric_zones' hand touches itself
LIMIT_PAST = 0.005
BOX_FRICTIONLOSS = 0.02
POOL = 32  # the step kernel's contact pool (dx_internal.h DX_NCON_MAX)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GUARD = _tool("record_guard_golden")
HEALTH = GUARD.HEALTH


def contact_records(ph, nenv) -> dict:
    """A forward pass on the current state with the debug record on: contact counts and
    records (those past an env's count are stale: zeroed)."""
    from dexterity_amd import _lib

    ph.debug(True)
    ph.forward()
    ph.sync()
    ncon = ph.get(_lib.NCON)[:, 0].astype(np.int32)
    keep = max(int(ncon.max()), 1)
    if ncon.max() > 0:
        con = ph.debug_get("contact")
        assert keep <= con.shape[1]
        con = con[:, :keep].copy()
    else:
        con = np.zeros((nenv, 1, 16), dtype=np.float32)
    for k in range(nenv):
        con[k, ncon[k]:] = 0
    return {"ncon": ncon, "contact": con}


def run_env_case(domain, nenv, steps) -> dict:
    """The case stepped with the device random agent: final state, warm start, qacc, task
    outputs, step types, health counters, the census after every control step and the
    final state's contact records."""
    from dexterity_amd import _lib, manipulation

    saved = {k: os.environ.pop(k, None) for k in GUARD.ENV_VARS}
    try:
        task = manipulation.SUITE[(domain, "state_dense")]()
        e = manipulation.GoalEnvironment(task, num_envs=nenv, seed=GUARD.SEED)
    finally:
        for k in GUARD.ENV_VARS:
            if saved[k] is not None:
                os.environ[k] = saved[k]
    ph = e.physics
    ph.debug(True)
    e.reset()
    types, ncons, nefcs, niters = [], [], [], []
    for i in range(steps):
        e.step_random(i)
        types.append(np.asarray(e.timestep().step_type).astype(np.int32))
        ncons.append(ph.get(_lib.NCON)[:, 0].astype(np.int32))
        nefcs.append(ph.debug_get("efc_count")[:, 0].astype(np.int32))
        niters.append(ph.get(_lib.NITER)[:, 0].astype(np.int32))
    ts = e.timestep()
    h = ph.health()
    out = {"qpos": ph.qpos, "qvel": ph.qvel, "warmstart": ph.get(_lib.QACC_WARMSTART), "qacc": ph.qacc,
           "reward": np.asarray(ts.reward), "discount": np.asarray(ts.discount), "step_types": np.stack(types),
           "observation": np.concatenate([np.asarray(v).reshape(nenv, -1) for v in ts.observation.values()], axis=1),
           "health": np.array([h[k] for k in HEALTH], dtype=np.int64),
           "census_ncon": np.stack(ncons), "census_nefc": np.stack(nefcs), "census_niter": np.stack(niters),
           "nfric": np.int32((np.asarray(task.compiled.arrays["dof_frictionloss"]).ravel() > 0).sum())}
    out.update(contact_records(ph, nenv))
    ph.debug(False)
    e.close()
    return out


def boxes_scene(n_boxes: int, n_planes: int, gravity=(0.0, 0.0, -9.81)):
    """`n_boxes` free cubes (half size 2 cm) with friction loss on their dofs, in a row on
    `n_planes` coincident ground planes."""
    from dexterity_amd.mjcf.compiler import Scene

    s = Scene(gravity=gravity)
    for k in range(n_planes):
        s.add_world_geom(f"ground{k}", "plane", (1, 1, 0.1))
    for i in range(n_boxes):
        s.add_free_box(f"box{i}", 0.02, [0.2 * (i - 0.5 * (n_boxes - 1)), 0.0, 0.0199])
        s.bodies[-1].joints[0]["frictionloss"] = BOX_FRICTIONLOSS
    return s.compile()


def phys_setup(key: str):
    """(compiled model, qpos [n, nq], qvel [n, nv], xfrc or None) of a physics case."""
    from dexterity_amd import physics
    from dexterity_amd.mjcf.compiler import CompiledModel

    if key == "box_rest":
        cm = boxes_scene(1, 1, gravity=(0.0, 0.0, 0.0))
        qpos = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (2, 1))
        qpos[:, 2] = (0.5, 0.8)
        return cm, qpos, np.zeros((2, int(cm.nv))), None
    if key == "boxes_140":
        cm = boxes_scene(2, 4)
        qpos = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (2, 1))
        qpos[1, 2], qpos[1, 9] = 0.0197, 0.0195  # (env 1: deeper, the two cubes differently)
        qvel = np.zeros((2, int(cm.nv)))
        qvel[:, 0], qvel[:, 7] = 0.05, -0.03
        return cm, qpos, qvel, None
    assert key in ("fric_zones", "limit_contact")
    cm = CompiledModel.load(os.path.join(ROOT, "assets", "shadow_reorient.npz"))
    fractions = RANGE_FRACTIONS if key == "fric_zones" else LIMIT_FRACTIONS
    n = len(fractions)
    qpos = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (n, 1))
    limited = 0
    for j in range(int(cm.njnt)):
        if cm.jnt_type[j] != 3 or not cm.jnt_limited[j]:
            continue
        lo, hi = cm.jnt_range[j]
        for k, t in enumerate(fractions):
            qpos[k, int(cm.jnt_qposadr[j])] = lo + t * (hi - lo)
        if key == "limit_contact" and limited < 2:
            qpos[0, int(cm.jnt_qposadr[j])] = lo - LIMIT_PAST
            qpos[1, int(cm.jnt_qposadr[j])] = hi + LIMIT_PAST
        limited += 1
    qpos[:, 24:27] = [0.3, 0.3, 0.5]  # the cube away from the hand
    qvel = np.random.RandomState(17).uniform(-0.5, 0.5, size=(n, int(cm.nv)))
    qvel[:, 24:] = 0.0
    return cm, qpos, qvel, physics.gravity_compensation(cm, "shadow_hand_e/")


def run_phys_case(key: str) -> dict:
    """The case's forward pass (qacc, counts, the dense M and qfrc_smooth of the debug
    record, contact records), then PHYS_SUBSTEPS substeps one at a time (counts after each;
    state, warm start and qacc at the end)."""
    from dexterity_amd import _lib, physics

    cm, qpos, qvel, xfrc = phys_setup(key)
    n = qpos.shape[0]
    ph = physics.BatchedPhysics(physics.Model(cm), n, device=0)
    if xfrc is not None:
        ph.set_xfrc(xfrc)
    ph.set(_lib.QPOS, qpos)
    ph.set(_lib.QVEL, qvel)
    rec = contact_records(ph, n)
    out = {"qacc0": ph.qacc, "ncon0": rec["ncon"], "contact0": rec["contact"],
           "nefc0": ph.debug_get("efc_count")[:, 0].astype(np.int32),
           "niter0": ph.get(_lib.NITER)[:, 0].astype(np.int32),
           "M0": ph.debug_get("M"), "qfrc_smooth0": ph.debug_get("qfrc_smooth")}
    ncons, nefcs, niters = [], [], []
    for _ in range(PHYS_SUBSTEPS):
        ph.step(1)
        ph.sync()
        ncons.append(ph.get(_lib.NCON)[:, 0].astype(np.int32))
        nefcs.append(ph.debug_get("efc_count")[:, 0].astype(np.int32))
        niters.append(ph.get(_lib.NITER)[:, 0].astype(np.int32))
    out.update({"qpos": ph.qpos, "qvel": ph.qvel, "warmstart": ph.get(_lib.QACC_WARMSTART), "qacc": ph.qacc,
                "ncon": np.stack(ncons), "nefc": np.stack(nefcs), "niter": np.stack(niters)})
    h = ph.health()
    out["health"] = np.array([h[k] for k in HEALTH], dtype=np.int64)
    ph.close()
    return out


def friction_zone_envs(out: dict) -> list:
    """fric_zones: the envs without contact and without limit row in which one dof's
    constraint force (M qacc - qfrc_smooth of the forward pass) is +floss and another's
    -floss."""
    from dexterity_amd.mjcf.compiler import CompiledModel

    cm = CompiledModel.load(os.path.join(ROOT, "assets", "shadow_reorient.npz"))
    floss = np.asarray(cm.arrays["dof_frictionloss"], dtype=np.float64).ravel()
    dofs = np.nonzero(floss > 0)[0]
    nv = floss.size
    envs = []
    for k in range(out["qacc0"].shape[0]):
        if out["ncon0"][k] != 0 or out["nefc0"][k] != dofs.size:
            continue
        M = np.asarray(out["M0"][k], dtype=np.float64).reshape(nv, nv)
        f = M @ np.asarray(out["qacc0"][k], dtype=np.float64) - np.asarray(out["qfrc_smooth0"][k], dtype=np.float64)
        ratio = f[dofs] / floss[dofs]
        if (np.abs(ratio - 1.0) < 1e-3).any() and (np.abs(ratio + 1.0) < 1e-3).any():
            envs.append(k)
    return envs


def check_phys_run(key: str, out: dict) -> None:
    """What the golden must hold of a physics case, asserted on the recording run."""
    h = dict(zip(HEALTH, (int(v) for v in out["health"])))
    for name in ("qacc0", "qacc", "qpos", "qvel", "warmstart"):
        assert np.isfinite(out[name]).all(), (key, name)
    assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, (key, h)
    if key == "fric_zones":
        assert friction_zone_envs(out), (key, out["ncon0"], out["nefc0"])
    elif key == "limit_contact":
        nfric = int((np.asarray(phys_setup(key)[0].arrays["dof_frictionloss"]).ravel() > 0).sum())
        assert ((out["ncon0"] > 0) & (out["nefc0"] - nfric - 4 * out["ncon0"] > 0)).any(), \
            (key, out["ncon0"], out["nefc0"], nfric)
    elif key == "box_rest":
        assert (out["nefc0"] == 6).all() and (out["nefc"] == 6).all(), (key, out["nefc0"], out["nefc"])
        assert (out["niter0"] == 0).all() and (out["niter"] == 0).all(), (key, out["niter0"], out["niter"])
    else:
        assert ((out["nefc0"] >= 129) & (out["nefc0"] <= 176)).all() and (out["ncon0"] <= POOL).all(), \
            (key, out["nefc0"], out["ncon0"])
        assert h["contact_deferred"] == 0, (key, h)


def check_env_run(out: dict) -> None:
    """What the golden must hold of the 64-env run, asserted on the recording run."""
    h = dict(zip(HEALTH, (int(v) for v in out["health"])))
    assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, h
    ncon, nefc, niter = out["census_ncon"], out["census_nefc"], out["census_niter"]
    solved = nefc > 0
    assert (solved & (niter == 1)).any(), "no solve of one iteration"
    assert (solved & (niter >= 4)).any(), "no solve of four iterations or more"
    assert ((nefc >= 65) & (nefc <= 128)).any(), "no solve with 65..128 rows"


def main():
    arrays = {}
    for key in PHYS_CASES:
        out = run_phys_case(key)
        print(f"{key}: forward contacts {out['ncon0'].tolist()} rows {out['nefc0'].tolist()} iterations "
              f"{out['niter0'].tolist()}; substeps: rows {out['nefc'].tolist()} iterations {out['niter'].tolist()}, "
              f"health {out['health'].tolist()}" + (f", friction zones in envs {friction_zone_envs(out)}" if key == "fric_zones" else ""),
              flush=True)
        check_phys_run(key, out)
        for name, a in out.items():
            arrays[f"{key}/{name}"] = a
    out = run_env_case(**ENV_CASE)
    ncon, nefc, niter = out["census_ncon"], out["census_nefc"], out["census_niter"]
    print(f"reorient_64: census over {nefc.size} env-substeps: rows min {nefc.min()} max {nefc.max()}, 65..128 rows "
          f"{((nefc >= 65) & (nefc <= 128)).sum()}, iterations {np.bincount(niter.ravel()).tolist()}, health {out['health'].tolist()}", flush=True)
    check_env_run(out)
    for name, a in out.items():
        arrays[f"reorient_64/{name}"] = a
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
