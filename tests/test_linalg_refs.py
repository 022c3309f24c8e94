"""The fp32 restatements that tests/test_gpu_linalg.py measures the device against, held to
that test's own yardstick on its own systems (tests/linalg_harness.py): against the fp64
truth every restatement's error stays within 4 kappa eps (kappa the 2-norm condition number
of the fp32 matrix, eps = 2^-24), for every n the GPU test covers and every system kind --
X X' + 0.1 I, mass-like matrices, Newton Hessians up to kappa ~ 1e7 -- with and without a
diagonal add.  No GPU: this pins the references, so a device failure is the device's.

tests/test_sweep_solve.py's rule err_s < max(1e-4, 10 err_chol) is not reused: at other n
than its own 30 the fp32 restatement itself breaks it (9.5 x over at worst, n = 1..30 on
the mass-like and Hessian-like kinds); an error is compared with kappa eps here instead.
"""
import numpy as np
import pytest

from tests import linalg_harness as lh


def _worst(errs):
    return max(errs, key=lambda t: t[0])


def _check(errs, what):
    w = _worst(errs)
    print(f"{what}: worst e / (kappa eps) = {w[0]:.3g} at {w[1:]} over {len(errs)} systems")
    bad = [t for t in errs if not t[0] <= 4.0]
    assert not bad, f"{what}: {len(bad)} systems above 4 kappa eps, worst {w}"


def test_sweep_restatement_within_4_kappa_eps():
    errs = [(s.err(lh.sweep_solve(s.Aeff, s.b)) / s.keps, n, s.kind)
            for n in range(1, 31) for s in lh.systems("sweep", n)]
    assert len(errs) == 30 * 6
    _check(errs, "sweep_solve")


@pytest.mark.parametrize("routine,lo,hi", [("chol32", 1, 32), ("chol64", 33, 64)])
def test_fp32_cholesky_within_4_kappa_eps(routine, lo, hi):
    errs = [(s.err(lh.chol_solve_f32(s.Aeff, s.b)) / s.keps, n, s.kind)
            for n in range(lo, hi + 1) for s in lh.systems(routine, n)]
    assert len(errs) == 32 * 6
    _check(errs, f"chol_solve_f32 ({routine})")


def test_sweep_inverse_restatement_within_4_kappa_eps():
    """max |Ainv - A^-1| / max |A^-1| against kappa eps; the restatement's result is
    symmetric to rounding."""
    errs = []
    for n in range(1, 31):
        for s in lh.systems("inverse", n):
            A64 = s.A.astype(np.float64)
            ref = np.linalg.inv(A64)
            keps = np.linalg.cond(A64, 2) * lh.EPS
            R = lh.sweep_inverse(s.A).astype(np.float64)
            errs.append((np.abs(R - ref).max() / np.abs(ref).max() / keps, n, s.kind))
            assert np.abs(R - R.T).max() <= 4 * keps * np.abs(ref).max()
    assert len(errs) == 30 * 6
    _check(errs, "sweep_inverse")


def test_fp32_cholesky_factor_within_4_n_eps():
    """||G G' - A||2 <= 4 n eps ||A||2 for numpy's fp32 factor (backward stable: the bound
    does not carry kappa)."""
    errs = []
    for n in range(1, 31):
        for s in lh.systems("factor", n):
            A64 = s.A.astype(np.float64)
            G = np.linalg.cholesky(s.A).astype(np.float64)
            errs.append((np.linalg.norm(G @ G.T - A64, 2) / np.linalg.norm(A64, 2) / (n * lh.EPS), n, s.kind))
    assert len(errs) == 30 * 6
    _check(errs, "cholesky factor (n eps)")


def test_tree_restatement_within_4_kappa_eps():
    """tests/test_tree_ldl.py's tree_solve on float32 arrays, on every tree the GPU test
    uses; at least two of the synthetic trees fit the kernel's item table."""
    trees = {**lh.asset_trees(), **lh.synthetic_trees()}
    assert lh.asset_trees(), "no shipped scene has nv > 30"
    fit = [k for k, par in lh.synthetic_trees().items() if lh.ldl_table(par)[0] <= lh.DX_LDL_SLOTS]
    assert len(fit) >= 2, fit
    errs = []
    for name, par in trees.items():
        slots, _ = lh.ldl_slots(par)
        for s in lh.tree_systems(name, par):
            x = lh.tree_solve(s.Aeff, slots, s.b)
            assert x.dtype == np.float32
            errs.append((s.err(x) / s.keps, name, len(par)))
    _check(errs, "tree_solve")


def test_inputs_are_what_the_tests_say():
    """Six systems per n, every second one with a diagonal add, all kinds present, fp32
    throughout, and the seeds are per (routine, n): the same call gives the same bits."""
    a, b = lh.systems("sweep", 7), lh.systems("sweep", 7)
    assert [s.kind for s in a] == list(lh.KINDS) and len(a) == 6
    assert all(np.array_equal(p.A, q.A) and np.array_equal(p.b, q.b) and np.array_equal(p.d, q.d) for p, q in zip(a, b))
    assert [bool(s.d.any()) for s in a] == [False, True] * 3
    assert all(s.A.dtype == np.float32 and s.b.dtype == np.float32 and np.array_equal(s.A, s.A.T) for s in a)
    assert not np.array_equal(a[0].A, lh.systems("chol32", 7)[0].A)
    assert max(s.cond for n in (24, 30) for s in lh.systems("sweep", n)) > 1e5  # the Hessians are ill-conditioned
    # packed triangles round-trip
    A = a[0].A
    assert np.array_equal(lh.unpack(lh.pack(A, lh.TRI32), 7, sym=True), A)


def test_harness_builds_and_rejects_sizes_it_could_not_index():
    """Both libraries build without a GPU and carry their lane-range mask; an n outside a
    routine's range, or a tree item outside the n x n triangle, is refused on the host
    (DXH_EINVAL = -1) before anything is allocated or launched."""
    import ctypes

    paths = lh.build()
    assert sorted(paths) == ["plain", "ranged"]
    for name, path in paths.items():
        L = ctypes.CDLL(path)
        assert L.dxh_lane_range_mask() == int(lh.BUILDS[name], 0) and L.dxh_ldl_slots() == lh.DX_LDL_SLOTS
        L.dxh_build_key.restype = ctypes.c_char_p
        assert L.dxh_build_key().decode() == lh.source_key(lh.BUILDS[name])
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
        buf = np.zeros(2 * lh.TRI64 + lh.VEC, np.float32)
        f = buf.ctypes.data_as(fp)
        for fn, bad in (("dxh_sweep_solve30", (0, 31)), ("dxh_chol_solve32", (0, 33)), ("dxh_chol_solve64", (32, 65))):
            for n in bad:
                nn = np.array([n], np.int32)
                args = [1, nn.ctypes.data_as(ip), f, f, f] + ([0] if "chol" in fn else [])
                assert getattr(L, fn)(*args, ctypes.c_uint(0), f) == -1, (fn, n)
        for fn in ("dxh_sweep_inverse30", "dxh_chol_factor30"):
            nn = np.array([31], np.int32)
            assert getattr(L, fn)(1, nn.ctypes.data_as(ip), f, ctypes.c_uint(0), f) == -1
        nn, ns, sy = np.array([8], np.int32), np.array([1], np.int32), np.array([1], np.uint32)
        tab = np.full(lh.DX_LDL_SLOTS * lh.WAVE, -1, np.int32)
        tab[3] = 9 | (2 << 8) | (1 << 16)  # dof 9 of an 8-dof tree
        assert L.dxh_tree_solve(1, nn.ctypes.data_as(ip), ns.ctypes.data_as(ip), sy.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                tab.ctypes.data_as(ip), f, f, f, ctypes.c_uint(0), f) == -1
