"""Builder, loader, inputs and fp32 references for the device-level tests of dx_device.h's
wave linear algebra and reductions (tests/csrc/dx_linalg_harness.hip).

build() compiles the harness twice with dexterity_amd/build.py's own FLAGS, once with
-DDX_LANE_RANGE_MASK=0 (the lane id as dx_ik / dx_dls see it) and once with 0x3b (as
dx_step.hip sees it), into tests/_build/libdx_linalg_harness_{plain,ranged}.so.  The
harness is not in build.py's csrc directory: libdx.so and its build key do not depend on it.

The references are the fp32 restatements of the same algorithms (tests/test_sweep_solve.py,
tests/test_tree_ldl.py, an fp32 Cholesky with two substitutions); fp64 numpy is the truth.
tests/test_linalg_refs.py holds the references to the bound the GPU test then applies to
the device, on the same systems.
"""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_sweep_solve import hessian_like, sweep_inverse, sweep_solve  # noqa: E402,F401
from tests.test_tree_ldl import ldl_slots, tree_solve  # noqa: E402,F401

SRC = os.path.join(HERE, "csrc", "dx_linalg_harness.hip")
OUTDIR = os.path.join(HERE, "_build")
BUILDS = {"plain": "0", "ranged": "0x3b"}  # DX_LANE_RANGE_MASK
EPS = 2.0 ** -24
WAVE = 64
TRI32, TRI64, VEC = 528, 2080, 64
POISON = 0x7FC0DEAD  # a quiet NaN with a payload: no arithmetic produces it
DX_LDL_SLOTS = 16  # dx_internal.h (the library reports its own: Harness.ldl_slots)


def lib_path(name: str) -> str:
    return os.path.join(OUTDIR, f"libdx_linalg_harness_{name}.so")


def source_key(mask: str) -> str:
    """Hash of everything one harness library is built from: the harness, the headers it
    includes, build.py's flags and the lane-range mask.  The library carries it
    (dxh_build_key), as libdx.so carries dx_build_key."""
    import hashlib

    from dexterity_amd import build as dx_build

    h = hashlib.sha1()
    for path in [SRC] + [os.path.join(dx_build.CSRC, f) for f in sorted(dx_build.HEADERS)]:
        h.update(os.path.basename(path).encode() + open(path, "rb").read())
    h.update((" ".join(dx_build.FLAGS) + " " + mask).encode())
    return h.hexdigest()[:16]


def _built_from(path: str, key: str) -> bool:
    return os.path.exists(path) and f"DXH_KEY:{key}".encode() in open(path, "rb").read()


def build(force: bool = False, verbose: bool = False) -> dict:
    """Both harness libraries.  A library that carries the key of the present sources is
    used as it is -- file times play no part, so a tree copied with its libraries (as
    libdx.so travels, dexterity_amd.build.build) is not compiled again."""
    from dexterity_amd import build as dx_build

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = {}
    for name, mask in BUILDS.items():
        path = out[name] = lib_path(name)
        key = source_key(mask)
        if not force and _built_from(path, key):
            continue
        os.makedirs(OUTDIR, exist_ok=True)
        tmp = f"{path}.{os.getpid()}.tmp"
        cmd = [hipcc, *dx_build.FLAGS, f"-DDX_LANE_RANGE_MASK={mask}", f'-DDXH_BUILD_KEY="{key}"', "-I", dx_build.CSRC,
               "-shared", SRC, "-o", tmp]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(tmp, path)
    return out


# ------------------------------------------------------------------------ #
# packed triangles
# ------------------------------------------------------------------------ #
def ti(i: int) -> int:
    return i * (i + 1) // 2


def pack(A: np.ndarray, words: int) -> np.ndarray:
    """Lower triangle of A, row-major, in a zero-padded buffer of `words` float32."""
    n = len(A)
    out = np.zeros(words, np.float32)
    out[:ti(n)] = A[np.tril_indices(n)]
    return out


def unpack(buf: np.ndarray, n: int, sym: bool = False) -> np.ndarray:
    """n x n lower-triangular (or symmetric) matrix of the first ti(n) words."""
    M = np.zeros((n, n), buf.dtype)
    M[np.tril_indices(n)] = buf[:ti(n)]
    return M + np.tril(M, -1).T if sym else M


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------ #
# inputs, shared by the CPU and the GPU tests
# ------------------------------------------------------------------------ #
KINDS = ("a", "b", "c12", "c40", "c70", "c40")  # six systems per (routine, n)
ROUTINES = {"sweep": 1, "chol32": 2, "chol64": 3, "inverse": 4, "factor": 5, "tree": 6, "pivots": 7}


class System:
    """One SPD system in fp32: A, the diagonal add d (zeros for every other system), the
    right-hand side b; Aeff = A with d added in fp32 is the matrix every solve sees, and
    the fp64 truth is taken of Aeff and b as rounded -- input rounding is not error."""

    def __init__(self, kind, A, d, b):
        self.kind, self.n = kind, len(b)
        self.A = np.ascontiguousarray(A, np.float32)
        self.d = np.ascontiguousarray(d, np.float32)
        self.b = np.ascontiguousarray(b, np.float32)
        self.Aeff = self.A.copy()
        self.Aeff[np.diag_indices(self.n)] = np.diag(self.A) + self.d  # fp32 add
        A64 = self.Aeff.astype(np.float64)
        self.cond = float(np.linalg.cond(A64, 2))
        self.xstar = np.linalg.solve(A64, self.b.astype(np.float64))

    def err(self, x) -> float:
        """||x - x*||2 / ||x*||2"""
        return float(np.linalg.norm(np.asarray(x, np.float64) - self.xstar) / np.linalg.norm(self.xstar))

    @property
    def keps(self) -> float:
        return self.cond * EPS


def spd(rng, kind: str, n: int) -> np.ndarray:
    if kind == "a":
        X = rng.standard_normal((n, n + 3))
        return X @ X.T + 0.1 * np.eye(n)
    if kind == "b":
        return hessian_like(rng, n, 0, 0.0)
    return hessian_like(rng, n, int(kind[1:]), 4.0)


def systems(routine: str, n: int, kinds=KINDS) -> list:
    """The systems of (routine, n): one per kind, every second one with d ~ U(0, 0.5)."""
    rng = np.random.default_rng([ROUTINES[routine], n])
    out = []
    for q, kind in enumerate(kinds):
        A = spd(rng, kind, n)
        A = 0.5 * (A + A.T)
        d = rng.uniform(0.0, 0.5, n) if q % 2 else np.zeros(n)
        out.append(System(kind, A, d, rng.standard_normal(n)))
    return out


def chol_solve_f32(A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp32 Cholesky (LAPACK spotrf) and the two substitutions in fp32."""
    f = np.float32
    L = np.linalg.cholesky(A.astype(f))
    n = len(b)
    y = np.zeros(n, f)
    for i in range(n):
        y[i] = (f(b[i]) - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, f)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


# ------------------------------------------------------------------------ #
# dof trees (parent arrays, parents before children) and tree-sparse systems
# ------------------------------------------------------------------------ #
def chain(n):
    return [k - 1 for k in range(n)]


def star(n):
    return [-1] + [0] * (n - 1)


def two_hands():
    """A 6-dof root chain carrying two hands of five 4-dof fingers: 46 dofs."""
    par = chain(6)
    for _ in range(2 * 5):
        par += [5, len(par), len(par) + 1, len(par) + 2]
    return par


def random_forest(n, seed=64):
    rng = np.random.default_rng(seed)
    return [int(rng.integers(-1, k)) for k in range(n)]


def synthetic_trees() -> dict:
    return {"chain16": chain(16), "star40": star(40), "two_hands46": two_hands(), "forest64": random_forest(64)}


def asset_trees(min_nv: int = 31) -> dict:
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "assets", "*.npz"))):
        par = [int(p) for p in np.load(path, allow_pickle=False)["dof_parentid"]]
        if len(par) >= min_nv:
            out[os.path.splitext(os.path.basename(path))[0]] = par
    return out


def ldl_table(par):
    """(nslot, sync, tab[DX_LDL_SLOTS * 64]) as dx_model.hip builds them, from ldl_slots."""
    slots, ends = ldl_slots(par)
    tab = np.full(DX_LDL_SLOTS * WAVE, -1, np.int32)
    sync = 0
    for e in ends:
        if e < 32:
            sync |= 1 << e
    if len(slots) <= DX_LDL_SLOTS:
        for s, sl in enumerate(slots):
            for q, (k, i, j) in enumerate(sl):
                tab[s * WAVE + q] = k | (i << 8) | (j << 16)
    return len(slots), sync, tab


def tree_systems(name: str, par, count: int = 6) -> list:
    """SPD matrices with the tree's sparsity (tests/test_tree_ldl.py's construction)."""
    nv = len(par)
    rng = np.random.default_rng([ROUTINES["tree"], nv, sum(name.encode())])
    out = []
    for q in range(count):
        L = np.eye(nv)
        for k in range(nv):
            i = par[k]
            while i >= 0:
                L[k, i] = rng.normal(scale=0.5)
                i = par[i]
        M = L.T @ np.diag(rng.uniform(0.2, 3.0, nv)) @ L
        d = rng.uniform(0.0, 0.5, nv) if q % 2 else np.zeros(nv)
        out.append(System("tree", 0.5 * (M + M.T), d, rng.standard_normal(nv)))
    return out


# ------------------------------------------------------------------------ #
# the ctypes loader
# ------------------------------------------------------------------------ #
def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


class Harness:
    """One of the two harness libraries.  Every call is one launch with all its cases and
    raises on a HIP error code; solves return the whole LDS image of every case."""

    def __init__(self, name: str):
        build()
        self.name = name
        self.L = ctypes.CDLL(lib_path(name))
        assert self.L.dxh_lane_range_mask() == int(BUILDS[name], 0)
        self.L.dxh_build_key.restype = ctypes.c_char_p
        assert self.L.dxh_build_key().decode() == source_key(BUILDS[name]), "the harness library is of other sources"
        self.ldl_slots = self.L.dxh_ldl_slots()

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: the harness returned {rc}")

    @staticmethod
    def _stage(cases, tri, with_x=True):
        """cases: (A, d, x) per case -> n, packed A, d and x buffers."""
        nc = len(cases)
        n = np.array([len(c[0]) for c in cases], np.int32)
        A = np.stack([pack(c[0], tri) for c in cases])
        d = np.zeros((nc, VEC), np.float32)
        x = np.zeros((nc, VEC), np.float32)
        if with_x:
            for q, c in enumerate(cases):
                d[q, :n[q]] = c[1]
                x[q, :n[q]] = c[2]
        return n, A, d, x

    def _solve(self, fn, tri, words, cases, fill, alias=None):
        n, A, d, x = self._stage(cases, tri)
        out = np.zeros((len(cases), words), np.float32)
        args = [len(cases), _p(n, ctypes.c_int), _p(A, ctypes.c_float), _p(d, ctypes.c_float), _p(x, ctypes.c_float)]
        if alias is not None:
            args.append(int(alias))
        self._check(getattr(self.L, fn)(*args, ctypes.c_uint(fill), _p(out, ctypes.c_float)), fn)
        return out

    # images: sweep A | x; chol A | x | T; inverse A | Ainv; factor A; tree A | x | T
    def sweep_solve30(self, cases, fill=POISON):
        return self._solve("dxh_sweep_solve30", TRI32, TRI32 + VEC, cases, fill)

    def chol_solve32(self, cases, alias=False, fill=POISON):
        return self._solve("dxh_chol_solve32", TRI32, 2 * TRI32 + VEC, cases, fill, alias)

    def chol_solve64(self, cases, alias=False, fill=POISON):
        return self._solve("dxh_chol_solve64", TRI64, 2 * TRI64 + VEC, cases, fill, alias)

    def _mat(self, fn, words, mats, fill):
        n, A, _, _ = self._stage([(m,) for m in mats], TRI32, with_x=False)
        out = np.zeros((len(mats), words), np.float32)
        self._check(getattr(self.L, fn)(len(mats), _p(n, ctypes.c_int), _p(A, ctypes.c_float), ctypes.c_uint(fill),
                                        _p(out, ctypes.c_float)), fn)
        return out

    def sweep_inverse30(self, mats, fill=POISON):
        return self._mat("dxh_sweep_inverse30", 2 * TRI32, mats, fill)

    def chol_factor30(self, mats, fill=POISON):
        return self._mat("dxh_chol_factor30", TRI32, mats, fill)

    def tree_solve(self, cases, tables, fill=POISON):
        """tables: (nslot, sync, tab) per case (ldl_table)."""
        n, A, d, x = self._stage(cases, TRI64)
        ns = np.array([t[0] for t in tables], np.int32)
        sy = np.array([t[1] for t in tables], np.uint32)
        tab = np.stack([t[2] for t in tables]).astype(np.int32)
        out = np.zeros((len(cases), 2 * TRI64 + VEC), np.float32)
        self._check(self.L.dxh_tree_solve(len(cases), _p(n, ctypes.c_int), _p(ns, ctypes.c_int), _p(sy, ctypes.c_uint),
                                          _p(tab, ctypes.c_int), _p(A, ctypes.c_float), _p(d, ctypes.c_float),
                                          _p(x, ctypes.c_float), ctypes.c_uint(fill), _p(out, ctypes.c_float)),
                    "dxh_tree_solve")
        return out

    def chol_pivots32(self, mats, thr, fill=POISON):
        """-> [ncase][64] int: every lane's return value."""
        n, A, _, _ = self._stage([(m,) for m in mats], TRI32, with_x=False)
        thr = np.ascontiguousarray(thr, np.float32)
        out = np.zeros((len(mats), WAVE), np.int32)
        self._check(self.L.dxh_chol_pivots32(len(mats), _p(n, ctypes.c_int), _p(A, ctypes.c_float),
                                             _p(thr, ctypes.c_float), ctypes.c_uint(fill), _p(out, ctypes.c_int)),
                    "dxh_chol_pivots32")
        return out

    def pgs_gram64(self, P, diag, full):
        """P [nc][64][30], diag [nc][64], full [nc] -> [nc][lane][64 rows]."""
        P = np.ascontiguousarray(P, np.float32)
        diag = np.ascontiguousarray(diag, np.float32)
        full = np.ascontiguousarray(full, np.int32)
        out = np.zeros((len(P), WAVE, 64), np.float32)
        self._check(self.L.dxh_pgs_gram64(len(P), _p(P, ctypes.c_float), _p(diag, ctypes.c_float),
                                          _p(full, ctypes.c_int), _p(out, ctypes.c_float)), "dxh_pgs_gram64")
        return out

    def reduce_scatter32(self, t):
        """t [nc][64 lanes][32] -> [nc][64]."""
        t = np.ascontiguousarray(t, np.float32)
        out = np.zeros((len(t), WAVE), np.float32)
        self._check(self.L.dxh_reduce_scatter32(len(t), _p(t, ctypes.c_float), _p(out, ctypes.c_float)),
                    "dxh_reduce_scatter32")
        return out

    def wave_ops(self, iv, fv, bi):
        """[nc][64] each -> [nc][8][64] int32 words: sum_i, max_i, min_i, incl, excl of iv;
        wave_sum, wave_max_f of fv (float bits); wave_argmax_first(fv, bi)."""
        iv = np.ascontiguousarray(iv, np.int32)
        fv = np.ascontiguousarray(fv, np.float32)
        bi = np.ascontiguousarray(bi, np.int32)
        out = np.zeros((len(iv), 8, WAVE), np.int32)
        self._check(self.L.dxh_wave_ops(len(iv), _p(iv, ctypes.c_int), _p(fv, ctypes.c_float), _p(bi, ctypes.c_int),
                                        _p(out, ctypes.c_int)), "dxh_wave_ops")
        return out
