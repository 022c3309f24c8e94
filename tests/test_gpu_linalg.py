"""Device-level tests of dx_device.h's wave linear algebra and reductions, run through
tests/csrc/dx_linalg_harness.hip (one kernel per routine, one wave per case, every case of
a routine in one launch) in both builds of the lane id: DX_LANE_RANGE_MASK 0 (dx_ik,
dx_dls) and 0x3b (dx_step.hip).

Solves are held to the fp64 truth by e_dev <= 4 max(e_ref, kappa eps): e = ||x - x*||2 /
||x*||2, e_ref the error of the fp32 numpy restatement of the same algorithm on the same
system (tests/test_linalg_refs.py keeps those within 4 kappa eps), eps = 2^-24.  The factor
4 is for what separates the device from the restatement -- 1-ulp v_rcp / v_rsq, FMA
contraction, the MFMA's accumulation order -- all rounding-level; a wrong lane, a lost
diagonal add or a missed pivot gives errors of order 1.  Around that: exact contracts (the
diagonal add, T aliasing A, poison against zero padding, repeatability, everything outside
the n-row triangle untouched), exact integer / max reductions, and summation-order bounds
for the float sums and the Gram matrix.  NaN inputs are outside the routines' documented
domain and are fed only where a routine documents them (mfma_chol_pivots32).

Every LDS image a kernel works in is filled with a NaN pattern before A and x are staged,
so a read past ti(n), past x[n-1] or of an unwritten word of T that reached a result
would show as NaN, and a store outside the routine's own words as a changed poison word.
"""
import functools

import numpy as np
import pytest

from tests import linalg_harness as lh

pytestmark = pytest.mark.gpu

TRI32, TRI64, VEC, EPS = lh.TRI32, lh.TRI64, lh.VEC, lh.EPS
POISON = np.uint32(lh.POISON)


@pytest.fixture(scope="module", params=list(lh.BUILDS))
def H(request):
    return lh.Harness(request.param)


# ------------------------------------------------------------------------ #
# cases and references: computed once, shared by both builds, never modified
# ------------------------------------------------------------------------ #
@functools.lru_cache(maxsize=None)
def solve_cases(routine):
    lo, hi, ref = {"sweep": (1, 30, lh.sweep_solve), "chol32": (1, 32, lh.chol_solve_f32),
                   "chol64": (33, 64, lh.chol_solve_f32)}[routine]
    sys_ = [s for n in range(lo, hi + 1) for s in lh.systems(routine, n)]
    assert len(sys_) == 6 * (hi - lo + 1)
    return sys_, [s.err(ref(s.Aeff, s.b)) for s in sys_]


@functools.lru_cache(maxsize=None)
def tree_cases():
    trees = {**lh.asset_trees(), **lh.synthetic_trees()}
    sys_, tabs, eref, names = [], [], [], []
    for name, par in trees.items():
        tab = lh.ldl_table(par)
        if tab[0] > lh.DX_LDL_SLOTS:
            continue  # the model would keep the dense solver (dx_model.hip)
        names.append(name)
        slots, _ = lh.ldl_slots(par)
        for s in lh.tree_systems(name, par):
            sys_.append(s)
            tabs.append(tab)
            eref.append(s.err(lh.tree_solve(s.Aeff, slots, s.b)))
    return sys_, tabs, eref, names


def _poison_words(a):
    return lh.bits(a) == POISON


def _check_solve(name, build, run, tri, sys_, eref, has_T):
    """run(cases, **kw) -> images A | x | (T).  The bound against fp64, the untouched
    words, then the exact contracts, each one more launch of all cases."""
    n = np.array([s.n for s in sys_])
    cases = [(s.A, s.d, s.b) for s in sys_]
    img = run(cases)
    # --- against fp64
    worst_dev = worst_ref = 0.0
    bad = []
    for q, s in enumerate(sys_):
        x = img[q, tri:tri + s.n]
        e = s.err(x) if np.all(np.isfinite(x)) else np.inf
        worst_dev, worst_ref = max(worst_dev, e / s.keps), max(worst_ref, eref[q] / s.keps)
        if not e <= 4 * max(eref[q], s.keps):
            bad.append((s.n, s.kind, q % 6, e, eref[q], s.keps))
    print(f"LINALG {name} {build}: worst e_dev / (kappa eps) = {worst_dev:.3g}, restatement {worst_ref:.3g}, "
          f"{len(sys_)} systems")
    assert not bad, f"{name}: e_dev > 4 max(e_ref, kappa eps) for (n, kind, index, e_dev, e_ref, kappa eps): {bad[:8]}"
    # --- untouched: A as staged and poison past ti(n); x past n; T past ti(n)
    for q, s in enumerate(sys_):
        t = lh.ti(s.n)
        assert np.array_equal(lh.bits(img[q, :t]), lh.bits(lh.pack(s.A, tri)[:t])), (name, "A changed", s.n)
        assert _poison_words(img[q, t:tri]).all(), (name, "A's padding written", s.n)
        assert _poison_words(img[q, tri + s.n:tri + VEC]).all(), (name, "x past n written", s.n)
        assert not _poison_words(img[q, tri:tri + s.n]).any()
        if has_T:
            assert _poison_words(img[q, tri + VEC + t:]).all(), (name, "T past ti(n) written", s.n)
    xs = [lh.bits(img[q, tri:tri + s.n]) for q, s in enumerate(sys_)]

    def same_x(other, what):
        diff = [sys_[q].n for q in range(len(sys_)) if not np.array_equal(lh.bits(other[q, tri:tri + n[q]]), xs[q])]
        assert not diff, f"{name}: {what}: x differs in bits at n = {sorted(set(diff))}"

    # --- the diagonal add: (A, d) == (A with d added in fp32 on the host, 0)
    assert sum(bool(s.d.any()) for s in sys_) == len(sys_) // 2
    same_x(run([(s.Aeff, 0 * s.d, s.b) for s in sys_]), "diagonal add on the host")
    # --- poison against zero padding
    z = run(cases, fill=0)
    same_x(z, "zero-filled padding")
    for q, s in enumerate(sys_):
        assert not z[q, tri + s.n:tri + VEC].any()
    # --- repeatability: the whole image
    assert np.array_equal(lh.bits(run(cases)), lh.bits(img)), f"{name}: two runs differ"
    return img, same_x


def test_sweep_solve30(H):
    sys_, eref = solve_cases("sweep")
    _check_solve("mfma_sweep_solve30", H.name, H.sweep_solve30, TRI32, sys_, eref, has_T=False)


def _check_alias(name, run, tri, sys_, same_x):
    """T aliasing A (the Newton path's chol_solve(H, nv, dir, H)): the same bits, the
    separate T words never touched, nothing past ti(n) of A written."""
    al = run([(s.A, s.d, s.b) for s in sys_], alias=True)
    same_x(al, "T aliasing A")
    for q, s in enumerate(sys_):
        assert _poison_words(al[q, lh.ti(s.n):tri]).all(), (name, "alias: A past ti(n) written", s.n)
        assert _poison_words(al[q, tri + s.n:]).all(), (name, "alias: x past n or the unused T written", s.n)


def test_chol_solve32(H):
    sys_, eref = solve_cases("chol32")
    _, same_x = _check_solve("mfma_chol_solve32", H.name, H.chol_solve32, TRI32, sys_, eref, has_T=True)
    _check_alias("mfma_chol_solve32", H.chol_solve32, TRI32, sys_, same_x)


def test_chol_solve64(H):
    sys_, eref = solve_cases("chol64")
    for s in sys_[1::2]:  # d1 (columns < 32) and d2 (columns >= 32): nonzero and distinct
        assert s.d[:32].all() and s.d[32:].all() and len(set(s.d.tolist())) == s.n
    _, same_x = _check_solve("mfma_chol_solve64", H.name, H.chol_solve64, TRI64, sys_, eref, has_T=True)
    _check_alias("mfma_chol_solve64", H.chol_solve64, TRI64, sys_, same_x)


def test_tree_solve(H):
    sys_, tabs, eref, names = tree_cases()
    assert H.ldl_slots == lh.DX_LDL_SLOTS
    assert any(k in names for k in lh.asset_trees()) and len([k for k in names if k in lh.synthetic_trees()]) >= 2, names
    run = lambda cases, **kw: H.tree_solve(cases, tabs, **kw)  # noqa: E731
    _check_solve("tree_solve", H.name, run, TRI64, sys_, eref, has_T=True)


# ------------------------------------------------------------------------ #
# inverse and factor
# ------------------------------------------------------------------------ #
@functools.lru_cache(maxsize=None)
def matrix_cases(routine):
    return [s for n in range(1, 31) for s in lh.systems(routine, n)]


def test_sweep_inverse30(H):
    sys_ = matrix_cases("inverse")
    mats = [s.A for s in sys_]
    img = H.sweep_inverse30(mats)
    worst_dev = worst_ref = 0.0
    for q, s in enumerate(sys_):
        t = lh.ti(s.n)
        A64 = s.A.astype(np.float64)
        ref = np.linalg.inv(A64)
        keps = np.linalg.cond(A64, 2) * EPS
        R = lh.sweep_inverse(s.A).astype(np.float64)
        scale = np.abs(ref).max()
        e_ref = np.abs(R - ref).max() / scale
        assert not _poison_words(img[q, TRI32:TRI32 + t]).any(), ("an entry of the triangle not written", s.n)
        D = lh.unpack(img[q, TRI32:], s.n).astype(np.float64)  # lower triangle
        lo = np.tril_indices(s.n)
        e_dev = np.abs(D - ref)[lo].max() / scale
        worst_dev, worst_ref = max(worst_dev, e_dev / keps), max(worst_ref, e_ref / keps)
        bound = 4 * max(e_ref, keps)
        assert e_dev <= bound, (s.n, s.kind, e_dev, e_ref, keps)
        # the written triangle against the restatement's entries on either side of the
        # diagonal (the restatement keeps both): each within the device's bound plus the
        # restatement's own error of the same truth
        assert np.abs(D - R)[lo].max() <= (bound + e_ref) * scale and np.abs(D - R.T)[lo].max() <= (bound + e_ref) * scale
        # untouched: A, and Ainv past ti(n)
        assert np.array_equal(lh.bits(img[q, :t]), lh.bits(lh.pack(s.A, TRI32)[:t]))
        assert _poison_words(img[q, t:TRI32]).all() and _poison_words(img[q, TRI32 + t:]).all(), s.n
    print(f"LINALG mfma_sweep_inverse30 {H.name}: worst max|Ainv - A^-1| / (kappa eps max|A^-1|) = {worst_dev:.3g}, "
          f"restatement {worst_ref:.3g}, {len(sys_)} matrices")
    z = H.sweep_inverse30(mats, fill=0)
    for q, s in enumerate(sys_):
        t = lh.ti(s.n)
        assert np.array_equal(lh.bits(z[q, TRI32:TRI32 + t]), lh.bits(img[q, TRI32:TRI32 + t])), ("zero padding", s.n)
        assert not z[q, TRI32 + t:].any()
    assert np.array_equal(lh.bits(H.sweep_inverse30(mats)), lh.bits(img))


def test_chol_factor30(H):
    sys_ = matrix_cases("factor")
    mats = [s.A for s in sys_]
    img = H.chol_factor30(mats)
    worst_dev = worst_ref = 0.0
    for q, s in enumerate(sys_):
        t = lh.ti(s.n)
        A64 = s.A.astype(np.float64)
        na = np.linalg.norm(A64, 2)
        Gn = np.linalg.cholesky(s.A).astype(np.float64)
        e_ref = np.linalg.norm(Gn @ Gn.T - A64, 2) / na
        assert not _poison_words(img[q, :t]).any(), ("an entry of the factor not written", s.n)
        G = lh.unpack(img[q], s.n).astype(np.float64)
        e_dev = np.linalg.norm(G @ G.T - A64, 2) / na
        worst_dev, worst_ref = max(worst_dev, e_dev / (s.n * EPS)), max(worst_ref, e_ref / (s.n * EPS))
        assert e_dev <= 4 * max(e_ref, s.n * EPS), (s.n, s.kind, e_dev, e_ref)
        assert (np.diag(G) > 0).all()
        assert _poison_words(img[q, t:]).all(), ("written past ti(n)", s.n)  # in place: the poison past ti(n)
    print(f"LINALG mfma_chol_factor30 {H.name}: worst ||G G' - A|| / (n eps ||A||) = {worst_dev:.3g}, "
          f"numpy fp32 {worst_ref:.3g}, {len(sys_)} matrices")
    z = H.chol_factor30(mats, fill=0)
    for q, s in enumerate(sys_):
        t = lh.ti(s.n)
        assert np.array_equal(lh.bits(z[q, :t]), lh.bits(img[q, :t])), ("zero padding", s.n)
        assert not z[q, t:].any()
    assert np.array_equal(lh.bits(H.chol_factor30(mats)), lh.bits(img))


# ------------------------------------------------------------------------ #
# mfma_chol_pivots32
# ------------------------------------------------------------------------ #
def test_chol_pivots32(H):
    rng = np.random.default_rng(lh.ROUTINES["pivots"])
    nv, eps32 = 24, np.float32(1.1920929e-07)
    mats, thr, want, what = [], [], [], []
    for n in (3, 6, 15, 30):
        J = rng.standard_normal((n, nv))
        A = (J @ J.T + 1e-2 * np.eye(n)).astype(np.float32)  # n = 30 > nv: the pivots past nv are reg's
        piv = np.diag(np.linalg.cholesky(A.astype(np.float64))) ** 2
        # an fp32 pivot is off by a few n eps max(diag): far inside the factors 0.5 and 2
        assert 8 * n * EPS * np.diag(A).max() < 0.25 * piv.min()
        for f, ok in ((0.5, 1), (2.0, 0)):
            mats.append(A); thr.append(f * piv.min()); want.append(ok); what.append(f"n {n} thr {f} x smallest pivot")
        for (i, j) in ((0, 0), (n - 1, 0), (n - 1, n - 1), (n // 2, 1)):  # a NaN entry: never above thr
            B = A.copy()
            B[i, j] = B[j, i] = np.nan
            mats.append(B); thr.append(0.5 * piv.min()); want.append(0); what.append(f"n {n} NaN at ({i}, {j})")
    # rank-deficient, reg = 0, at dx_dls.hip's threshold eps_fp32 max(n3, nv) max_i H_ii
    for n3, rank in ((15, 12), (30, 24), (6, 5)):
        J = rng.standard_normal((n3, nv))
        J[rank:] = J[:n3 - rank]  # the rows past the rank repeat the first ones
        A = (J.astype(np.float32).astype(np.float64) @ J.astype(np.float32).astype(np.float64).T).astype(np.float32)
        mats.append(A); thr.append(eps32 * np.float32(max(n3, nv)) * np.diag(A).max()); want.append(0)
        what.append(f"n3 {n3} rank {rank} at the DLS threshold")
        F = rng.standard_normal((n3, nv))  # full rank at the same threshold: true
        if n3 <= nv:
            A = (F @ F.T).astype(np.float32)
            mats.append(A); thr.append(eps32 * np.float32(max(n3, nv)) * np.diag(A).max()); want.append(1)
            what.append(f"n3 {n3} full rank at the DLS threshold")
    ok = H.chol_pivots32(mats, thr)
    assert (ok == ok[:, :1]).all(), "the result is not wave-uniform"
    wrong = [w for w, got, exp in zip(what, ok[:, 0], want) if got != exp]
    assert not wrong, wrong
    assert np.array_equal(H.chol_pivots32(mats, thr, fill=0), ok) and np.array_equal(H.chol_pivots32(mats, thr), ok)


# ------------------------------------------------------------------------ #
# reductions and scans
# ------------------------------------------------------------------------ #
def _int_cases():
    rng = np.random.default_rng(11)
    lanes = np.arange(64)
    small = [rng.integers(-1000, 1001, 64) for _ in range(8)]
    small += [np.where(lanes == k, 7, 0) for k in range(64)]    # one-hot at every lane: each DPP stage's source
    small += [np.where(lanes == k, -7, 0) for k in range(64)]   # (negative: the minimum's turn)
    small += [np.ones(64, int), -np.ones(64, int)]
    small += [np.array(c)[lanes // 16] for c in ((1, 2, 3, 4), (4, 3, 2, 1), (0, 5, 0, 0), (-3, 0, 9, -8), (0, 0, 0, 6))]
    small += [np.array(c)[(lanes // 4) % 4] for c in ((1, 20, 300, 4000), (-5, 6, -7, 8))]  # per-quad constants
    wide = [rng.integers(-2**31, 2**31, 64) for _ in range(8)]  # max / min only: the sums would overflow
    wide += [np.where(lanes == k, -2**31, 2**31 - 1) for k in (0, 15, 16, 31, 32, 47, 48, 63)]
    return np.array(small, np.int32), np.array(wide).astype(np.int32)


def test_integer_reductions_and_scans(H):
    small, wide = _int_cases()
    iv = np.concatenate([small, wide])
    z = np.zeros_like(iv)
    out = H.wave_ops(iv, z.astype(np.float32), z)
    for k in range(3):
        assert (out[:, k] == out[:, k, :1]).all(), "a reduction's result is not uniform over the wave"
    ns = len(small)
    assert np.array_equal(out[:ns, 0, 0], small.sum(1, dtype=np.int32)), "wave_sum_i"
    assert np.array_equal(out[:, 1, 0], iv.max(1)), "wave_max_i"
    assert np.array_equal(out[:, 2, 0], iv.min(1)), "wave_min_i"
    inc = np.cumsum(small, 1, dtype=np.int32)
    bad = np.argwhere(out[:ns, 3] != inc)
    assert not len(bad), f"wave_incl_scan: first (case, lane) {bad[0]}"
    assert np.array_equal(out[:ns, 4], inc - small), "wave_excl_scan"


def _max_bits(f):
    m = np.float32(f.max())
    return np.float32(0.0).view(np.uint32) if m == 0 else m.view(np.uint32)  # -0 / +0: +0


def test_wave_max_f_and_argmax_first(H):
    rng = np.random.default_rng(12)
    lanes = np.arange(64)
    inf, nz = np.float32(np.inf), np.float32(-0.0)
    fv = [rng.standard_normal(64) * 10 ** rng.uniform(-20, 20) for _ in range(8)]
    fv += [-np.abs(rng.standard_normal(64)) - 0.5 for _ in range(4)]                  # all negative
    fv += [np.full(64, nz), np.where(lanes == 37, 0.0, nz), np.where(lanes == 5, nz, -1.0),
           np.where(lanes % 2 == 0, nz, 0.0)]                                        # -0 / +0: +0
    fv += [np.where(lanes == k, inf, rng.standard_normal(64)) for k in (0, 31, 32, 63)]
    fv += [np.full(64, -inf), np.where(lanes == 40, -1e30, -inf), np.where(lanes == 9, -inf, inf)]
    fv += [np.where(lanes == k, 1.5, 0.0) for k in range(64)]                        # one-hot at every lane
    fv += [np.where(lanes == k, -1.5, -3.0) for k in range(0, 64, 7)]
    # ties across rows and halves: the maximum at several lanes
    ties = [(5, 21, 37, 53), (15, 16), (31, 32), (47, 48, 63), (0, 63), (63,), (33, 2), tuple(range(64)), (20, 52), (12, 28)]
    fv += [np.where(np.isin(lanes, t), 2.0, rng.uniform(-1, 1, 64)) for t in ties]
    fv = np.array(fv, np.float32)
    nc = len(fv)
    for bi in (np.tile(lanes, (nc, 1)), np.tile(63 - lanes, (nc, 1)), np.tile(1000 + (lanes * 37) % 64, (nc, 1))):
        out = H.wave_ops(np.zeros_like(bi), fv, bi)
        assert (out[:, 6] == out[:, 6, :1]).all() and (out[:, 7] == out[:, 7, :1]).all()
        got = out[:, 6, 0].view(np.uint32)
        want = np.array([_max_bits(f) for f in fv])
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"wave_max_f: cases {bad[:8]}: {got[bad[:8]]} != {want[bad[:8]]}"
        first = np.array([bi[q][fv[q] == fv[q].max()].min() for q in range(nc)])
        bad = np.flatnonzero(out[:, 7, 0] != first)
        assert not len(bad), f"wave_argmax_first: cases {bad[:8]}: {out[bad[:8], 7, 0]} != {first[bad[:8]]}"


def test_wave_sum(H):
    """|err| <= 63 eps sum |v| (64 terms in any order); exact where every partial sum is."""
    rng = np.random.default_rng(13)
    lanes = np.arange(64)
    fv = [rng.standard_normal(64) * 10 ** rng.uniform(-3, 3, 64) for _ in range(16)]
    fv += [np.where(lanes == k, 1.5, 0.0) for k in range(64)]
    fv += [np.ones(64), np.array((1.0, 2.0, 3.0, 4.0))[lanes // 16], lanes.astype(float)]
    fv = np.array(fv, np.float32)
    out = H.wave_ops(np.zeros(fv.shape, np.int32), fv, np.zeros(fv.shape, np.int32))
    assert (out[:, 5] == out[:, 5, :1]).all()
    got = out[:, 5, 0].view(np.float32).astype(np.float64)
    f64 = fv.astype(np.float64)
    assert (np.abs(got - f64.sum(1)) <= 63 * EPS * np.abs(f64).sum(1)).all()
    assert np.array_equal(got[16:], f64[16:].sum(1)), "a sum of small integers / one-hots is exact in any order"


def test_wave_reduce_scatter32(H):
    rng = np.random.default_rng(14)
    t = [rng.standard_normal((64, 32)) * 10 ** rng.uniform(-2, 2, (64, 32)) for _ in range(8)]
    t = np.array(t, np.float32)
    # one-hot (lane, component) sweep: 64 x 32 cases, the value names its source
    hot = np.zeros((64 * 32, 64, 32), np.float32)
    L, C = np.divmod(np.arange(64 * 32), 32)
    val = (1.0 + L + C / 32.0).astype(np.float32)
    hot[np.arange(64 * 32), L, C] = val
    out = H.reduce_scatter32(np.concatenate([t, hot]))
    assert np.array_equal(lh.bits(out[:, 0::2]), lh.bits(out[:, 1::2])), "lanes 2c and 2c + 1 differ"
    t64 = t.astype(np.float64)
    err = np.abs(out[:8, 0::2].astype(np.float64) - t64.sum(1))
    assert (err <= 63 * EPS * np.abs(t64).sum(1)).all(), err.max()
    want = np.zeros((64 * 32, 32), np.float32)
    want[np.arange(64 * 32), C] = val
    bad = np.argwhere(out[8:, 0::2] != want)
    assert not len(bad), f"one-hot: first (case = 32 lane + component, component read) {bad[0]}"
    assert np.array_equal(lh.bits(H.reduce_scatter32(t)), lh.bits(out[:8]))


def test_pgs_gram64(H):
    """Entry (r, c) (lane c, out[r]) within 31 eps (sum_k |P_rk P_ck| + |diag|) of fp64: 30
    products and the diagonal, in any order.  !full: the doc comment says "tile (0, 0)
    alone"; solve_pgs_ar then visits only the row groups below 32 and its lanes >= 32 hold
    padding rows (AR_kk replaced by 1, a zero box), so rows >= 32 of every lane and all of
    lanes >= 32 are left out of the assertion -- whatever rows 32-63 of P and diag hold."""
    rng = np.random.default_rng(15)
    P, diag, full = [], [], []
    for nv in (30, 29, 24, 7, 1):
        for f in (1, 0, 0):
            p = np.zeros((64, 30))
            p[:, :nv] = rng.standard_normal((64, nv)) * 10 ** rng.uniform(-1, 1, (64, 1))  # zero tails past nv
            d = rng.uniform(0.1, 10.0, 64)
            if not f and len(full) % 3 == 1:  # as the caller has them: no rows past 32
                p[32:], d[32:] = 0.0, 0.0
            P.append(p); diag.append(d); full.append(f)
    P, diag, full = np.array(P, np.float32), np.array(diag, np.float32), np.array(full, np.int32)
    out = H.pgs_gram64(P, diag, full)  # [case][lane c][row r]
    P64 = P.astype(np.float64)
    for q in range(len(P)):
        ref = P64[q] @ P64[q].T + np.diag(diag[q].astype(np.float64))
        tol = 31 * EPS * (np.abs(P64[q]) @ np.abs(P64[q]).T + np.diag(np.abs(diag[q].astype(np.float64))))
        m = 64 if full[q] else 32
        err = np.abs(out[q].T.astype(np.float64) - ref)[:m, :m]
        bad = np.argwhere(err > tol[:m, :m])
        assert not len(bad), f"case {q} full {full[q]}: first (row, lane) {bad[0]}: {err[tuple(bad[0])]}"
        assert np.isfinite(out[q]).all()
    assert np.array_equal(lh.bits(H.pgs_gram64(P, diag, full)), lh.bits(out))
