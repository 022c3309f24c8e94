"""Factoring the constraint solvers' shared pieces, and the drivers that run an env to the
end of its control step, must leave every result as it was.  tests/golden/solver_parent.npz
(tools/record_solver_golden.py, run with the parent revision's library) holds the solver
paths that the other bit-exact goldens do not reach, on the scenes of tests/pgs_cases.py:
solve_cg in LDS (nv <= 30 with more than 128 rows, in the generic step kernel and in the
mid tier; nv > 30 with its Cholesky M^-1), solve_pgs's register-row sweep in the mid and the
overflow tier, its LDS sweep (nv > 30) and solve_pgs_ar without a tail.  Each case is
replayed on this tree's library -- one env, three physics steps in two launches -- and
compared byte for byte, after the run itself has shown, by the library's own counts, that
it took the intended path (the recorder's assertions)."""

import importlib.util
import os

import numpy as np
import pytest

from tests.test_gpu_parity import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_solver_golden", os.path.join(ROOT, "tools", "record_solver_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def solver_golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "solver_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_golden_took_the_paths(solver_golden):
    """The recorded run (the parent's own): the first launch of every case has the table's
    contact and row counts, and every launch's last physics step iterated and has counts that
    select the case's tier and solver path."""
    for key, case in REC.CASES.items():
        ncon, nefc, niter = (solver_golden[f"{key}/{f}"] for f in ("ncon", "nefc", "niter"))
        assert ncon.shape == nefc.shape == niter.shape == (len(REC.LAUNCHES),)
        assert (int(ncon[0]), int(nefc[0])) == (case["ncon"], case["nefc"]), key
        for n in range(len(REC.LAUNCHES)):
            assert niter[n] >= 1 and REC.path_ok(case, case["nv"], int(ncon[n]), int(nefc[n])), (key, n)
        nq = case["nv"] + case["spec"][0]  # (a free cube: 7 coordinates, 6 dofs)
        assert solver_golden[f"{key}/state"].shape == (len(REC.LAUNCHES), 4 * (nq + 3 * case["nv"])), key


@pytest.mark.parametrize("key", list(REC.CASES))
def test_results_are_the_parents(gpu, oracle_mod, solver_golden, key):  # noqa: F811
    """The same launches on this tree's library (run_case asserts the path on this run):
    qpos, qvel, warm start and qacc after each launch equal the parent revision's bit for
    bit, and so do the iteration, row and contact counts."""
    got = REC.run_case(key)
    for name in REC.FIELDS:
        a, want = got[name], solver_golden[f"{key}/{name}"]
        assert a.shape == want.shape and a.dtype == want.dtype, name
        assert a.tobytes() == want.tobytes(), (name, a, want)
