"""The step kernel's lane guards are scaffolding, not arithmetic: rewriting them must leave
every result as it was.  tests/golden/guard_parent.npz (tools/record_guard_golden.py, run
with the parent revision's library) holds the kernels and paths that
tests/golden/broadphase_parent.npz does not reach -- the CG and PGS specializations, both
reach scenes across an auto-reset, the generic kernel, the mid and the overflow tier, and
64 reorient envs whose states span the constraint-row counts (more than one wave of rows,
the friction rows alone, no contact).  Each case is replayed on this tree's library and
compared byte for byte."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_guard_golden", os.path.join(ROOT, "tools", "record_guard_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def guard_golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "guard_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_golden_spans_the_row_counts(guard_golden):
    """The recorded 64-env run (the parent's own) holds an env-substep with more than 64
    constraint rows, one with the scene's friction rows alone and one with no contact; the
    forced-tier runs deferred steps; both reach runs ended an episode inside the window."""
    nefc, ncon = guard_golden["reorient_64/census_nefc"], guard_golden["reorient_64/census_ncon"]
    assert REC.census_ok(nefc, ncon, int(guard_golden["reorient_64/nfric"]))
    assert nefc.shape == ncon.shape == (REC.CASES["reorient_64"]["steps"], guard_golden["reorient_64/ncon"].shape[0])
    for key in REC.CASES:
        REC.check_parent_run(key, {k: guard_golden[f"{key}/{k}"] for k in ("health", "step_types")})


@pytest.mark.parametrize("key", list(REC.CASES))
def test_results_are_the_parents(guard_golden, key):
    """The same calls on this tree's library: state, warm start, task outputs, step types,
    health counters and the final state's contact records equal the parent revision's, bit
    for bit."""
    case = dict(REC.CASES[key], nenv=int(guard_golden[f"{key}/ncon"].shape[0]))  # (reorient_64: the recorded env count)
    got = REC.run_case(**case)
    for name, a in got.items():
        want = guard_golden[f"{key}/{name}"]
        assert a.shape == want.shape and a.dtype == want.dtype, name
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(want).tobytes(), name
