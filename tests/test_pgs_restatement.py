"""The oracle's PGS (oracle/dx_oracle.c solve_pgs) against an independent numpy restatement
(tests/pgs_cases.py solve_pgs), and the sensitivity of the PGS dispatch cases
(test_gpu_pgs_dispatch.py) to the defect they were built to catch: a solver that leaves the
tail rows' starting forces out of qacc.  CPU only."""

import numpy as np
import pytest

from dexterity_amd import blob
from tests import pgs_cases as pc
from tests.test_gpu_parity import PGS_TAIL_MAX

_cache = {}


def _setup(oracle_mod, tmp_path_factory, spec):
    """Per scene: the model, the settled state, and per eps the warm start, the oracle's
    PGS pass and the dual problem it solved."""
    if spec in _cache:
        return _cache[spec]
    cm = pc.scene(*spec, tmp_path=tmp_path_factory.mktemp("rack"))
    om = oracle_mod.OracleModel(blob.pack(cm.arrays))
    om_nt = oracle_mod.OracleModel(blob.pack(cm.with_solver("Newton").arrays))
    q, v = pc.settled_state(oracle_mod, cm)
    dn = pc.oracle_at(oracle_mod, om_nt, q, v)
    w, a0 = dn.qacc.copy(), dn.qacc_smooth.copy()
    runs = []
    for eps in pc.EPS:
        warm = pc.f32(pc.warm_start(w, a0, eps))
        d = pc.oracle_at(oracle_mod, om, q, v, warm=warm)
        runs.append((eps, warm, d, pc.Problem(d, cm)))
    _cache[spec] = (cm, dn, max(1.0, np.abs(a0).max()), runs)
    return _cache[spec]


@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_numpy_pgs_matches_oracle(oracle_mod, tmp_path_factory, case):
    """The restatement and the oracle agree on qacc within 1e-10 of the scale (measured:
    4e-15) and on the sweep count, with the warm start kept (dual cost below -1) for eps up
    to 1e-3 and, where the case is a tail case, dropped at 1e-2; and the scene has the
    dofs, contacts and rows its place in the dispatch matrix needs."""
    name, spec, tier, NB, nv, ncon, nefc, path = case
    cm, dn, scale, runs = _setup(oracle_mod, tmp_path_factory, spec)
    assert (cm.nv, dn.ncon, dn.nefc) == (nv, ncon, nefc)
    for eps, warm, d, p in runs:
        assert d.nefc == nefc
        qacc, sweeps, keep, f0 = pc.solve_pgs(p, warm)
        dc = p.dual_cost(p.warm_forces(warm))
        err = np.abs(qacc - d.qacc).max() / scale
        print(f"{name} eps {eps:g}: dual cost {dc:.3g}, sweeps {sweeps} (oracle {d.niter}), |qacc| err / scale {err:.1e}")
        assert err <= 1e-10 and sweeps == d.niter
        if eps <= 1e-3:
            assert dc < -1 and keep
            assert np.all(f0[p.nfric:] > 0)  # every contact row shares the load
        elif path != "chol":
            assert dc > 0 and not keep
    if spec[3]:
        # friction-loss rows inside their box and at its bounds
        p = runs[0][3]
        f = np.abs(runs[0][2].efc_force[: p.nfric])
        assert p.nfric == spec[3] and (f >= p.floss[: p.nfric]).sum() >= 3 and (f < p.floss[: p.nfric]).sum() >= 3


@pytest.mark.parametrize("case", [c for c in pc.CASES if c[7] == "tail"], ids=[c[0] for c in pc.CASES if c[7] == "tail"])
def test_tail_cases_see_a_forgotten_tail(oracle_mod, tmp_path_factory, case):
    """A statement about the numpy model, not about the kernel: with the tail rows' starting
    forces left out of qacc (solve_pgs tail_from), every tail case with a kept warm start
    ends more than 5 x PGS_TAIL_MAX of the scale from the oracle -- so the GPU test's bound
    cannot hold for a kernel that forgets them."""
    name, spec, tier, NB, nv, ncon, nefc, path = case
    cm, dn, scale, runs = _setup(oracle_mod, tmp_path_factory, spec)
    tail = NB * pc.PGS_AR
    assert tail < nefc <= tail + pc.PGS_AR
    for eps, warm, d, p in runs:
        if eps > 1e-3:
            continue
        qacc, sweeps, keep, f0 = pc.solve_pgs(p, warm, tail_from=tail)
        err = np.abs(qacc - d.qacc).max() / scale
        print(f"{name} eps {eps:g}: {nefc - tail} tail rows, {np.count_nonzero(f0[tail:])} start nonzero, "
              f"forgotten: |qacc| err / scale {err:.1e}")
        assert keep and np.count_nonzero(f0[tail:]) > 0
        assert err > 5 * PGS_TAIL_MAX
