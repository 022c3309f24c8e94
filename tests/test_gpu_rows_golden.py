"""The box cull without its identity products, the row parameters computed once per contact
and the impedance without its ladder on the power remove work, not arithmetic: every result
stays what the parent revision computed.  tests/golden/rows_parent.npz
(tools/record_rows_golden.py, run with the parent revision's library) holds the paths they
touch that the older goldens do not pin: 64 reorient envs; the mid and the overflow tier with
the row counts after every control step; Adroit reach with tendon-limit rows; the bimanual
handover; a frictionless contact (one row per contact); the hand's joints beyond both ends of
their ranges; a scene whose solimp power is 3, which runs the impedance's general-power path;
and two cubes on nine coincident planes, 72 contacts in an env, which run make_constraint's
second chunk of 64 contacts in the overflow tier.  Each case is replayed on this tree's
library and compared byte for byte; the power-3 scene is also held to the fp64 oracle.

The mid-phase is the parent's single-stage loop (a version compacted on its sphere test was
measured and not kept).  The 64-env run still carries the census of its
pair counts per control step: more than one chunk, part of one, none, and pairs of which none
was kept -- by the box test: the stage counters do not tell a pair the sphere test dropped
from one the box test dropped."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_rows_golden", os.path.join(ROOT, "tools", "record_rows_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def rows_golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "rows_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def _case(golden, key):
    return {k[len(key) + 1:]: v for k, v in golden.items() if k.startswith(key + "/")}


def test_golden_reaches_the_paths(rows_golden):
    """The recorded runs (the parent's own) took the paths: the mid-phase census of the
    64-env run, deferred steps in the forced-tier runs, a tendon-limit row in the Adroit run,
    one row per frictionless contact, limit rows on both sides (the row count exact), contacts
    in the power-3 run, more than 64 contacts in every env of the boxes_72 run."""
    c = _case(rows_golden, "reorient_64")
    assert REC.census_ok(c["census_pairs"], c["census_keep"])
    assert c["census_pairs"].shape == (REC.ENV_CASES["reorient_64"]["steps"], c["ncon"].shape[0])
    for key in REC.ENV_CASES:
        REC.check_env_run(key, _case(rows_golden, key))
    for key in REC.PHYS_CASES:
        REC.check_phys_run(key, _case(rows_golden, key))
    assert _case(rows_golden, "boxes_72")["ncon0"].min() > 64


def _same(got, want, skip=()):
    for name, a in got.items():
        if name in skip:
            continue
        w = want[name]
        assert a.shape == w.shape and a.dtype == w.dtype, name
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(w).tobytes(), name


@pytest.mark.parametrize("key", list(REC.ENV_CASES))
def test_env_results_are_the_parents(rows_golden, key):
    """The same calls on this tree's library: state, warm start, task outputs, step types,
    health counters, the contact and row counts after every control step and the final
    state's contact records equal the parent revision's, bit for bit."""
    want = _case(rows_golden, key)
    case = dict(REC.ENV_CASES[key], nenv=int(want["ncon"].shape[0]))  # (reorient_64: the recorded env count)
    _same(REC.env_case(case), want)


@pytest.mark.parametrize("key", list(REC.PHYS_CASES))
def test_physics_results_are_the_parents(rows_golden, key):
    """Forward pass and substeps of the set states: qacc, state, warm start, contact and row
    counts equal the parent revision's, bit for bit."""
    _same(REC.run_phys_case(key), _case(rows_golden, key))


def test_power3_scene_matches_the_oracle(oracle_mod):
    """The general-power impedance against the fp64 oracle: constrained qacc of the forward
    pass within 5e-4 of max(1, |qacc_smooth|), the bound of tests/test_gpu_parity.py."""
    from dexterity_amd import blob

    cm, qpos, qvel, _ = REC.phys_setup("box_power3")
    assert (np.asarray(cm.arrays["gpair_solimp"]).reshape(-1, 5)[:, 4] == 3).all()
    got = REC.run_phys_case("box_power3")
    om = oracle_mod.OracleModel(blob.pack(cm.arrays))
    for e in range(qpos.shape[0]):
        d = oracle_mod.OracleData(om)
        d.qpos[:] = qpos[e].astype(np.float32)
        d.qvel[:] = qvel[e].astype(np.float32)
        d.forward()
        assert got["nefc0"][e] == d.nefc
        scale = max(1.0, np.abs(d.qacc_smooth).max())
        err = np.abs(got["qacc0"][e] - d.qacc).max()
        print(f"power-3 env {e}: |qacc| err {err:.3e}, scale {scale:.3e}")
        assert err <= 5e-4 * scale, e
