"""Records tests/golden/rows_parent.npz: the broadphase, mid-phase and constraint-row paths
that the box cull without identity products, the row parameters computed once per contact and
the power-2 impedance touch, for tests/test_gpu_rows_golden.py to replay bit for bit.  (The
mid-phase itself is the parent's single-stage loop: a version compacted on its sphere test was
measured and not kept, DESIGN.md section 9.  Its pair-count census stays in the golden for
whoever takes that up again.)

Run it on the GPU against the library of the revision whose results are the yardstick:

  python tools/build_variant.py --rev=<parent> parent
  DX_LIB=variants/parent/libdx.so python tools/record_rows_golden.py

Environment cases (ENV_CASES, stepped with the device random agent as
tools/record_guard_golden.py steps its own; 16 envs x 6 control steps unless noted): reorient
at 64 envs x 10 steps; reorient with every contact step forced to the mid tier and through it
to the overflow tier (the tier kernels' copies of the changed code; these runs have at most
19 contacts in an env, so they do not reach make_constraint's chunks past the first -- the
boxes_72 case below does); Adroit reach (tendon-limit rows); the bimanual handover at 8 envs
(its own kernel and contact records).

Physics cases (PHYS_CASES, states set through the batch API, a forward pass and then
PHYS_SUBSTEPS substeps): a frictionless (condim 1) cube on a plane (the one-row contact); the
reorient hand with every limited joint below its range, above it, alternating, and inside it
(limit rows on both sides); the cube on the plane with solimp power 3 (the impedance's
general-power path), at penetrations on both segments of the impedance curve and on its
plateau; two cubes on nine coincident planes (boxes_72: 72 contacts and 288 rows in an env,
more than the mid tier's 64, so the overflow tier runs make_constraint's second chunk of 64
contacts, `ch > 0`: its tables reloaded, row_coef once and row_store per edge).

The recorder refuses to write unless, on the run it records (the parent's own):
  * the forced-tier cases deferred steps (health counter contact_deferred);
  * the Adroit case ends in a state with an active tendon-limit row in some env;
  * the condim-1 case has contacts and exactly one row per contact; the joint-limit case has
    at least one row per limited joint on top of the friction rows, in the env below and in
    the env above the ranges (exactly: friction rows + active limit rows + four rows per
    contact); the power-3 case has contacts in every env; the boxes_72 case has more than 64
    contacts in every env's forward pass, four rows per contact, deferred steps and no
    overflow;
  * the 64-env case's mid-phase census holds.  The census comes from the stage counters
    (dx_stage_read: mid_pairs, the geom pairs the mid-phase walked; mid_keep, the pairs it
    kept), in a second, identical run with the stage record on (it adds stores only; the
    recorder checks that both runs end in the same state).  The counters add up over an
    env's collision passes, so the census reads their growth over one control step -- five
    substeps and at most one observation pass, NPASS passes -- and asks for an env and a
    control step with: more than 64 * NPASS pairs (some pass walked more than one chunk);
    between 1 and 64 pairs in all (some pass walked part of a chunk); no pair (every pass
    found the list empty); pairs but none kept (the box test's list ended empty; the counters
    do not tell a pair the sphere test dropped from one the box test dropped).  When 64 envs
    do not hold such steps the env count is doubled (CENSUS_ENVS); the golden carries the
    count it was recorded at.
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "rows_parent.npz")
NPASS = 6  # collision passes of one control step: five substeps and the observation pass
CENSUS_ENVS = (64, 128, 256)
ENV_CASES = {
    "reorient_64": dict(domain="reorient", nenv=64, steps=10),
    "reorient_mid": dict(domain="reorient", nenv=16, steps=6, env={"DX_DEFER_AT": "0"}),
    "reorient_overflow": dict(domain="reorient", nenv=16, steps=6, env={"DX_DEFER_AT": "0", "DX_MID_DEFER_AT": "0"}),
    "reach_adroit": dict(domain="reach", nenv=16, steps=6),
    "bimanual": dict(domain="bimanual", nenv=8, steps=6),
}
PHYS_CASES = ("box_condim1", "joint_limits", "box_power3", "boxes_72")
POWER3_SOLIMP = "0.9 0.95 0.001 0.5 3"
# the cube's height over the plane (half size 0.02): penetrations of 0.1, 0.3 (the impedance's
# lower segment, x <= mid), 0.7 (its upper segment) and 1.5 (its plateau) of solimp's width
BOX_Z = (0.0199, 0.0197, 0.0193, 0.0185)
PHYS_SUBSTEPS = 3


def _guard():
    spec = importlib.util.spec_from_file_location("record_guard_golden", os.path.join(ROOT, "tools", "record_guard_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GUARD = _guard()
HEALTH = GUARD.HEALTH


def box_scene(condim: int, solimp: str = None):
    """A free cube (half size 2 cm) over a level plane, both geoms with the given condim
    (and solimp)."""
    from dexterity_amd.mjcf.compiler import Scene

    s = Scene(timestep=0.002, gravity=(0.0, 0.0, -9.81))
    kw = dict(condim=condim, friction="1.0 0.005 0.0001")
    if solimp:
        kw["solimp"] = solimp
    s.add_world_geom("ground", "plane", (1, 1, 0.1), **kw)
    s.add_free_box("box", 0.02, [0.0, 0.0, 0.0199], **kw)
    return s.compile()


def boxes_scene(n_boxes: int, n_planes: int):
    """`n_boxes` free cubes in a row on `n_planes` coincident ground planes: four contacts per
    cube and plane (the scene of tests/pgs_cases.py, with the default Newton solver)."""
    from dexterity_amd.mjcf.compiler import Scene

    s = Scene()
    for k in range(n_planes):
        s.add_world_geom(f"ground{k}", "plane", (1, 1, 0.1))
    for i in range(n_boxes):
        s.add_free_box(f"box{i}", 0.02, [0.2 * (i - 0.5 * (n_boxes - 1)), 0.0, 0.0199])
    return s.compile()


def phys_setup(key: str):
    """(compiled model, qpos [n, nq], qvel [n, nv], xfrc or None) of a physics case."""
    from dexterity_amd import physics
    from dexterity_amd.mjcf.compiler import CompiledModel

    if key in ("box_condim1", "box_power3"):
        cm = box_scene(1) if key == "box_condim1" else box_scene(3, POWER3_SOLIMP)
        qpos = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (len(BOX_Z), 1))
        qpos[:, 2] = BOX_Z
        qvel = np.zeros((len(BOX_Z), int(cm.nv)))
        qvel[:, 0] = 0.05  # sliding: the pyramid's edges see a tangential velocity
        return cm, qpos, qvel, None
    if key == "boxes_72":
        cm = boxes_scene(2, 9)
        qpos = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (2, 1))
        qpos[1, 2], qpos[1, 9] = 0.0197, 0.0195  # (env 1: deeper, the two cubes differently)
        qvel = np.zeros((2, int(cm.nv)))
        qvel[:, 0], qvel[:, 7] = 0.05, -0.03
        return cm, qpos, qvel, None
    assert key == "joint_limits"
    cm = CompiledModel.load(os.path.join(ROOT, "assets", "shadow_reorient.npz"))
    qpos = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (4, 1))
    rng = np.random.RandomState(11)
    k = 0
    for j in range(int(cm.njnt)):
        if cm.jnt_type[j] != 3 or not cm.jnt_limited[j]:
            continue
        lo, hi = cm.jnt_range[j]
        a = int(cm.jnt_qposadr[j])
        qpos[0, a] = lo - 0.02
        qpos[1, a] = hi + 0.02
        qpos[2, a] = lo - 0.01 if k % 2 == 0 else hi + 0.01
        qpos[3, a] = rng.uniform(lo, hi)
        k += 1
    qpos[:, 24:27] = [0.3, 0.3, 0.5]  # the cube away from the hand
    qvel = rng.uniform(-0.5, 0.5, size=(4, int(cm.nv)))
    return cm, qpos, qvel, physics.gravity_compensation(cm, "shadow_hand_e/")


def joint_limit_rows(cm, q) -> int:
    """Active joint-limit rows at qpos q: a limited hinge within its margin of either end of
    its range."""
    n = 0
    for j in range(int(cm.njnt)):
        if cm.jnt_type[j] != 3 or not cm.jnt_limited[j]:
            continue
        lo, hi = cm.jnt_range[j]
        x, m = float(np.float32(q[int(cm.jnt_qposadr[j])])), float(cm.jnt_margin[j])
        n += int(x - np.float32(lo) < m) + int(np.float32(hi) - x < m)
    return n


def run_phys_case(key: str) -> dict:
    """The case's forward pass (qacc, contact and row counts), then PHYS_SUBSTEPS substeps
    (state, warm start, counts)."""
    from dexterity_amd import _lib, physics

    cm, qpos, qvel, xfrc = phys_setup(key)
    model = physics.Model(cm)
    ph = physics.BatchedPhysics(model, qpos.shape[0], device=0)
    if xfrc is not None:
        ph.set_xfrc(xfrc)
    ph.set(_lib.QPOS, qpos)
    ph.set(_lib.QVEL, qvel)
    ph.debug(True)
    ph.forward()
    ph.sync()
    out = {"qacc0": ph.qacc, "ncon0": ph.get(_lib.NCON)[:, 0].astype(np.int32),
           "nefc0": ph.debug_get("efc_count")[:, 0].astype(np.int32),
           "qacc_smooth0": ph.debug_get("qacc_smooth")}
    ph.step(PHYS_SUBSTEPS)
    ph.sync()
    out.update({"qpos": ph.qpos, "qvel": ph.qvel, "warmstart": ph.get(_lib.QACC_WARMSTART),
                "ncon": ph.get(_lib.NCON)[:, 0].astype(np.int32),
                "nefc": ph.debug_get("efc_count")[:, 0].astype(np.int32)})
    h = ph.health()
    out["health"] = np.array([h[k] for k in HEALTH], dtype=np.int64)
    ph.close()
    return out


def check_phys_run(key: str, out: dict) -> None:
    from dexterity_amd.mjcf.compiler import CompiledModel

    for name in ("qacc0", "qpos", "qvel", "warmstart"):
        assert np.isfinite(out[name]).all(), (key, name)
    if key == "box_condim1":
        assert (out["ncon0"] > 0).all() and (out["nefc0"] == out["ncon0"]).all(), (key, out["ncon0"], out["nefc0"])
    elif key == "box_power3":
        assert (out["ncon0"] > 0).all() and (out["nefc0"] == 4 * out["ncon0"]).all(), (key, out["ncon0"], out["nefc0"])
    elif key == "boxes_72":
        h = dict(zip(HEALTH, (int(v) for v in out["health"])))
        assert (out["ncon0"] > 64).all() and (out["nefc0"] == 4 * out["ncon0"]).all(), (key, out["ncon0"], out["nefc0"])
        assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, (key, h)
        assert h["contact_deferred"] > 0, (key, h)
    else:
        cm, qpos, _, _ = phys_setup(key)
        nfric = int((np.asarray(cm.arrays["dof_frictionloss"]).ravel() > 0).sum())
        limits = np.array([joint_limit_rows(cm, q) for q in qpos])
        nlim = int(sum(1 for j in range(int(cm.njnt)) if cm.jnt_type[j] == 3 and cm.jnt_limited[j]))
        assert (limits[:3] == nlim).all() and limits[3] == 0, (key, limits, nlim)
        # (the hand's contacts with itself are condim 3: four rows each)
        assert (out["nefc0"] == nfric + limits + 4 * out["ncon0"]).all(), (key, out["nefc0"], out["ncon0"], nfric, limits)


def tendon_limit_rows(cm, q) -> int:
    """Active tendon-limit rows at qpos q: a limited fixed tendon whose length is within its
    margin of either end of its range."""
    n = 0
    for t in range(int(cm.ntendon)):
        if not cm.tendon_limited[t]:
            continue
        a, k = int(cm.tendon_adr[t]), int(cm.tendon_num[t])
        length = sum(float(cm.wrap_coef[w]) * q[int(cm.jnt_qposadr[int(cm.dof_jntid[int(cm.wrap_dof[w])])])]
                     for w in range(a, a + k))
        lo, hi = cm.tendon_range[t]
        m = float(cm.tendon_margin[t])
        n += int(length - lo < m) + int(hi - length < m)
    return n


def check_env_run(key: str, out: dict) -> None:
    h = dict(zip(HEALTH, (int(v) for v in out["health"])))
    assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, (key, h)
    if key in ("reorient_mid", "reorient_overflow"):
        assert h["contact_deferred"] > 0, (key, h)
    if key == "reach_adroit":
        from dexterity_amd.mjcf.compiler import CompiledModel

        cm = CompiledModel.load(os.path.join(ROOT, "assets", "adroit_reach.npz"))
        rows = [tendon_limit_rows(cm, q) for q in np.asarray(out["qpos"], dtype=np.float64)]
        assert max(rows) > 0, f"{key}: no env ends with an active tendon-limit row"


def env_case(case: dict) -> dict:
    """record_guard_golden's run_case with the debug record on from the start (it adds stores
    only): the final state, the task outputs, the step types, the health counters, the final
    state's contact records, and the contact and constraint-row counts after every control
    step (census_ncon, census_nefc)."""
    out = GUARD.run_case(census=True, **case)
    return {k: np.asarray(v) for k, v in out.items()}


def mid_census(domain, nenv, steps, env=None) -> dict:
    """The 64-env case once more with the stage record on: the growth of mid_pairs and
    mid_keep per env over every control step, and the final state."""
    from dexterity_amd import _lib, manipulation

    saved = {k: os.environ.pop(k, None) for k in GUARD.ENV_VARS}
    os.environ.update(env or {})
    try:
        e = manipulation.GoalEnvironment(manipulation.SUITE[(domain, "state_dense")](), num_envs=nenv, seed=GUARD.SEED)
    finally:
        for k in GUARD.ENV_VARS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    L = _lib.load()
    ph = e.physics
    names = {v: k for k, v in _lib.COUNTERS.items()}
    buf = (ctypes.c_uint64 * (_lib.NSTAGE * nenv))()

    def read():
        ph.sync()
        _lib.check(L.dx_stage_read(ph.ptr, buf, _lib.NSTAGE * nenv))
        a = np.frombuffer(buf, dtype=np.uint64).reshape(nenv, _lib.NSTAGE).astype(np.int64)
        return a[:, names["mid_pairs"]].copy(), a[:, names["mid_keep"]].copy()

    _lib.check(L.dx_stage_timing(ph.ptr, 1))
    e.reset()
    read()  # (dx_stage_read hands out the counts since the last read: the reset's are dropped)
    pairs, keep = [], []
    for i in range(steps):
        e.step_random(i)
        p1, k1 = read()
        pairs.append(p1)
        keep.append(k1)
    out = {"qpos": ph.qpos, "qvel": ph.qvel, "warmstart": ph.get(_lib.QACC_WARMSTART),
           "census_pairs": np.stack(pairs), "census_keep": np.stack(keep)}
    e.close()
    return out


def census_ok(pairs: np.ndarray, keep: np.ndarray) -> bool:
    return bool((pairs > 64 * NPASS).any() and ((pairs >= 1) & (pairs <= 64)).any() and (pairs == 0).any()
                and ((pairs > 0) & (keep == 0)).any())


def main():
    arrays = {}
    for key, case in ENV_CASES.items():
        if key == "reorient_64":
            continue
        out = env_case(case)
        check_env_run(key, out)
        n = out["ncon"]
        print(f"{key}: contacts per env mean {n.mean():.2f} max {n.max()}, health {out['health'].tolist()}")
        for name, a in out.items():
            arrays[f"{key}/{name}"] = a
    for key in PHYS_CASES:
        out = run_phys_case(key)
        check_phys_run(key, out)
        print(f"{key}: forward contacts {out['ncon0'].tolist()} rows {out['nefc0'].tolist()}; after {PHYS_SUBSTEPS} substeps "
              f"contacts {out['ncon'].tolist()} rows {out['nefc'].tolist()}")
        for name, a in out.items():
            arrays[f"{key}/{name}"] = a
    for nenv in CENSUS_ENVS:
        case = dict(ENV_CASES["reorient_64"], nenv=nenv)
        out = env_case(case)
        check_env_run("reorient_64", out)
        c = mid_census(**case)
        for name in ("qpos", "qvel", "warmstart"):
            assert c[name].tobytes() == out[name].tobytes(), f"the census run differs in {name}"
        pairs, keep = c["census_pairs"], c["census_keep"]
        print(f"reorient_64 at {nenv} envs, census over {pairs.size} env-steps of {NPASS} collision passes: pairs min "
              f"{pairs.min()} max {pairs.max()}; > {64 * NPASS} pairs {(pairs > 64 * NPASS).sum()}, 1..64 pairs "
              f"{((pairs >= 1) & (pairs <= 64)).sum()}, no pair {(pairs == 0).sum()}, pairs but none kept "
              f"{((pairs > 0) & (keep == 0)).sum()}, health {out['health'].tolist()}")
        if census_ok(pairs, keep):
            break
    else:
        sys.exit("refusing to write: no env count holds the mid-phase census")
    for name, a in out.items():
        arrays[f"reorient_64/{name}"] = a
    arrays["reorient_64/census_pairs"], arrays["reorient_64/census_keep"] = pairs, keep
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
