"""dx_jac_object and dx_dls_map (dexterity_amd/csrc/dx_dls.hip) on the GPU against the fp64
oracle and numpy: object Jacobians for bodies, geoms and sites, the damped-least-squares
Cartesian-to-joint velocity mapper (controllers/dls/dls.py:43-77), its rank guard, the
reference's single-env call shape, device-memory arguments, closed-loop use against the IK
solver, and the argument errors.

B = 8 environments throughout, at the states of test_ik.py::test_jac_site_matches_oracle:
qpos0 with every limited hinge uniform in its range (RandomState(1)), rounded to fp32.

Mapper bound (per env): the max-norm relative error against the fp64 reference --
np.linalg.solve(J^T J + reg I, J^T V), or np.linalg.lstsq(J, V) for reg = 0, with J from the
oracle at the same fp32 qpos -- must be <= 8 * max(e32, 1e-6) and <= 1e-3, where e32 is the
error of a numpy float32 evaluation of the formula the device runs (Gram matrix, Cholesky,
J^T y) on the same inputs; the factor 8 covers the summation orders of the matrix cores and
of the wave reductions, the cap keeps the emulation from excusing a wrong kernel.
Measured on the MI355X: device errors 7e-7 .. 2.7e-5 over the 120
states, all of it the error its fp32 Jacobian carries; the worst ratio to max(e32, 1e-6) is
2.1.  The e32 of one state is a single draw of rounding noise (1e-7 .. 1.2e-4 here), which is
why the kernel refines its fp32 solve once with an fp64 residual: a bare fp32 solve is as
accurate as numpy's on the whole but missed this per-state bound in 2 of the 120 states.
"""

import ctypes
import os

import numpy as np
import pytest

from dexterity_amd import blob
from dexterity_amd.mjcf.compiler import CompiledModel
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

B = 8
BODY, GEOM, SITE = 1, 5, 6
_FINGERS = ("ff", "mf", "rf", "lf", "th")


@pytest.fixture(scope="module")
def gpu():
    from dexterity_amd import build, physics

    build.build()
    return physics


class _Scene:
    """One asset: its compiled model, oracle, device batch at the B test states, and the
    oracle's fp64 Jacobians of whatever objects the tests ask for (computed once)."""

    def __init__(self, physics, oracle_mod, asset):
        from dexterity_amd import _lib

        self.O = oracle_mod
        self.cm = cm = CompiledModel.load(os.path.join(ROOT, "assets", f"{asset}.npz"))
        self.om = oracle_mod.OracleModel(blob.pack(cm.arrays))
        self.model = physics.Model(cm)
        rs = np.random.RandomState(1)
        qpos = np.tile(cm.qpos0, (B, 1))
        for j in range(cm.njnt):
            if cm.jnt_type[j] == 3 and cm.jnt_limited[j]:
                lo, hi = cm.jnt_range[j]
                qpos[:, cm.jnt_qposadr[j]] = rs.uniform(lo, hi, size=B)
        self.qpos = qpos.astype(np.float32)
        self.phys = physics.BatchedPhysics(self.model, B)
        self.phys.set(_lib.QPOS, self.qpos)
        self.nv = cm.nv
        self._data = {}
        self._bodyjac = {}
        self._jac = {}

    def close(self):
        self.phys.close()

    def data(self, e):
        """The oracle at env e's fp32 state, after fk()."""
        if e not in self._data:
            d = self.O.OracleData(self.om)
            d.qpos[:] = self.qpos[e]
            d.fk()
            self._data[e] = d
        return self._data[e]

    def body_jac(self, e, b):
        """[6, nv]: column d is mj_objectVelocity of body b's frame origin ([lin, ang],
        world) with qvel = e_d, which is linear in qvel: (mj_jacBody jacp, jacr)."""
        if e not in self._bodyjac:
            d = self.O.OracleData(self.om)
            d.qpos[:] = self.qpos[e]
            out = np.zeros((self.cm.nbody, 6, self.nv))
            for k in range(self.nv):
                d.qvel[:] = 0.0
                d.qvel[k] = 1.0
                d.observe()
                for bb in range(self.cm.nbody):
                    out[bb, :, k] = d.object_velocity("xbody", bb)
            self._bodyjac[e] = out
        return self._bodyjac[e][b]

    def jac(self, e, typ, idx):
        """(jacp, jacr) [3, nv] fp64 of one object in env e."""
        key = (e, typ, idx)
        if key not in self._jac:
            cm = self.cm
            if typ == SITE:
                self._jac[key] = self.data(e).jac_site(idx)
            elif typ == BODY:
                j = self.body_jac(e, idx)
                self._jac[key] = (j[:3].copy(), j[3:].copy())
            else:
                # the body's [lin, ang] transported to xpos + xmat . geom_pos: lin + ang x r
                b = int(np.asarray(cm.geom_bodyid).ravel()[idx])
                j = self.body_jac(e, b)
                r = self.data(e).xmat.reshape(-1, 3, 3)[b] @ np.asarray(cm.geom_pos).reshape(-1, 3)[idx]
                self._jac[key] = (j[:3] + np.cross(j[3:].T, r).T, j[3:].copy())
        return self._jac[key]

    def stacked_jacp(self, e, types, ids):
        return np.concatenate([self.jac(e, t, i)[0] for t, i in zip(types, ids)], axis=0)

    def chain_dofs(self, types, ids):
        """Mask [nv] of the dofs on some object's path to the root."""
        cm = self.cm
        parent = np.asarray(cm.body_parent).ravel()
        adr, num = np.asarray(cm.body_dofadr).ravel(), np.asarray(cm.body_dofnum).ravel()
        mask = np.zeros(self.nv, bool)
        for t, i in zip(types, ids):
            b = i if t == BODY else int(np.asarray(cm.geom_bodyid if t == GEOM else cm.site_bodyid).ravel()[i])
            while b > 0:
                mask[adr[b]:adr[b] + num[b]] = True
                b = int(parent[b])
        return mask


@pytest.fixture(scope="module")
def scenes(gpu, oracle_mod):
    cache = {}

    def get(asset):
        if asset not in cache:
            cache[asset] = _Scene(gpu, oracle_mod, asset)
        return cache[asset]

    yield get
    for s in cache.values():
        s.close()


def _hand_prefixes(cm):
    return sorted({n.split("/")[0] + "/" for n in cm.names["body"] if "/" in n and not n.startswith("prop")})


def _fingertip_sites(cm):
    """The fingertip sites of every hand of the scene, in hand order."""
    from dexterity_amd import hands

    names = cm.names["site"]
    out = []
    for p in _hand_prefixes(cm):
        if p.startswith("adroit"):
            out += [names.index(p + s) for s in hands.ADROIT_FINGERTIP_SITES]
        else:
            out += [names.index(p + f"{t}_site") for t in hands.SHADOW_FINGERTIPS]
    return out


def _test_bodies(cm):
    """One body per finger (its distal link), the palm and the forearm of the first hand,
    and the prop body where the scene has one."""
    names = cm.names["body"]
    p = _hand_prefixes(cm)[0]
    out = [names.index(p + f + "distal") for f in _FINGERS] + [names.index(p + "palm"), names.index(p + "forearm")]
    if "prop/" in names:
        out.append(names.index("prop/"))
    return out


def _test_geoms(cm):
    """Three geoms: the named ones first (the Shadow scenes name only the ground and the
    prop's geom), topped up with the last geoms of the hand's distal links, by id."""
    names = cm.names["geom"]
    named = [i for i, n in enumerate(names) if n]
    if len(named) >= 3:
        # a palm, a finger and a thumb geom of the Adroit hand
        want = ("C_palm0", "C_ffdistal", "C_thdistal")
        return [next(i for i in named if names[i].endswith(w)) for w in want]
    gb = np.asarray(cm.geom_bodyid).ravel()
    p = _hand_prefixes(cm)[0]
    th = cm.names["body"].index(p + "thdistal")
    extra = [int(np.flatnonzero(gb == th)[-1])]
    return (named + extra)[:3]


# --------------------------------------------------------------------------- #
# 1. object Jacobians
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("asset", ["adroit_reach", "shadow_reorient", "bimanual_handover"])
def test_jac_object_matches_oracle(scenes, asset):
    s = scenes(asset)
    cm, phys = s.cm, s.phys
    # sites: bit-equal to dx_jac_site
    sites = _fingertip_sites(cm)
    jp0, jr0 = phys.jac_site(sites)
    jp, jr = phys.jac_object([SITE] * len(sites), sites)
    np.testing.assert_array_equal(jp, jp0)
    np.testing.assert_array_equal(jr, jr0)
    jp_only, none = phys.jac_object([SITE] * len(sites), sites, rotational=False)
    assert none is None
    np.testing.assert_array_equal(jp_only, jp0)
    # bodies and geoms against the oracle's mj_objectVelocity columns
    bodies, geoms = _test_bodies(cm), _test_geoms(cm)
    assert len(geoms) == 3 and len(bodies) >= 7
    for typ, ids in ((BODY, bodies), (GEOM, geoms)):
        jp, jr = phys.jac_object([typ] * len(ids), ids)
        assert jp.shape == (B, len(ids), 3, cm.nv) and jr.shape == jp.shape
        worst_p = worst_r = 0.0
        for e in range(B):
            for k, i in enumerate(ids):
                rp, rr = s.jac(e, typ, i)
                scale = max(1.0, np.abs(rp).max())
                worst_p = max(worst_p, np.abs(jp[e, k] - rp).max() / scale)
                worst_r = max(worst_r, np.abs(jr[e, k] - rr).max())
                np.testing.assert_allclose(jp[e, k], rp, atol=1e-5 * scale)
                np.testing.assert_allclose(jr[e, k], rr, atol=1e-5)
        print(f"{asset} type {typ}: jacp err {worst_p:.2e}, jacr err {worst_r:.2e}")
    # a mixed call keeps the objects' order
    types = [BODY, GEOM, SITE]
    ids = [bodies[0], geoms[-1], sites[0]]
    jp, jr = phys.jac_object(types, ids)
    for k, (t, i) in enumerate(zip(types, ids)):
        rp, rr = s.jac(0, t, i)
        np.testing.assert_allclose(jp[0, k], rp, atol=1e-5 * max(1.0, np.abs(rp).max()))
        np.testing.assert_allclose(jr[0, k], rr, atol=1e-5)
    # the batch state is untouched
    np.testing.assert_array_equal(phys.qpos, s.qpos)


# --------------------------------------------------------------------------- #
# 2. the mapper against numpy
# --------------------------------------------------------------------------- #
def _ref64(J, V, reg):
    """dls.py:69-77 in fp64."""
    if reg > 0:
        return np.linalg.solve(J.T @ J + reg * np.eye(J.shape[1]), J.T @ V)
    return np.linalg.lstsq(J, V, rcond=None)[0]


def _emulate32(J, V, reg):
    """The device's formula, J^T (J J^T + reg I)^-1 V by Cholesky, in numpy float32."""
    J32, V32 = J.astype(np.float32), V.astype(np.float32)
    H = J32 @ J32.T + np.float32(reg) * np.eye(J32.shape[0], dtype=np.float32)
    L = np.linalg.cholesky(H)
    y = np.linalg.solve(L.T, np.linalg.solve(L, V32))
    assert y.dtype == np.float32
    return J32.T @ y


def _relerr(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / np.abs(ref).max())


def _case_objects(cm, case):
    sites = _fingertip_sites(cm)
    if case == "fingertips":
        return [SITE] * len(sites), sites
    if case == "single":
        return [SITE], [sites[0]]
    # mixed: a thumb link, the prop's geom (its free joint's dofs) or an Adroit palm geom, a fingertip site
    return [BODY, GEOM, SITE], [_test_bodies(cm)[4], _test_geoms(cm)[1 if "prop/" in cm.names["body"] else 0], sites[1]]


def _check_against_numpy(s, types, ids, reg, q, status, V):
    """The bound of the module docstring, per env; returns the worst (error, e32)."""
    worst = (0.0, 0.0)
    for e in range(B):
        J = s.stacked_jacp(e, types, ids)
        ref = _ref64(J, V[e].reshape(-1).astype(np.float64), reg)
        e32 = _relerr(_emulate32(J, V[e].reshape(-1), reg), ref)
        err = _relerr(q[e], ref)
        worst = max(worst, (err, e32))
        print(f"env {e}: device err {err:.3e}  float32 numpy err {e32:.3e}")
        assert status[e] == 0
        assert err <= 8.0 * max(e32, 1e-6), (e, err, e32)
        assert err <= 1e-3, (e, err)
    return worst


_CASES = [("shadow_reorient", "fingertips", 15, 30), ("adroit_reach", "fingertips", 15, 24),
          ("bimanual_handover", "fingertips", 30, 54), ("shadow_reorient", "single", 3, 30),
          ("shadow_reorient", "mixed", 9, 30)]


@pytest.mark.parametrize("reg", [1e-5, 1e-2, 0.0])
@pytest.mark.parametrize("asset,case,n3,nv", _CASES)
def test_dls_map_matches_numpy(scenes, asset, case, n3, nv, reg):
    from dexterity_amd import _lib

    s = scenes(asset)
    types, ids = _case_objects(s.cm, case)
    assert (3 * len(ids), s.nv) == (n3, nv)
    V = np.random.RandomState(3).uniform(-0.1, 0.1, size=(B, len(ids), 3)).astype(np.float32)
    t = np.asarray(types, np.int32)
    i = np.asarray(ids, np.int32)
    q = np.full((B, nv), np.nan, np.float32)
    st = np.full(B, -1, np.int32)
    L = _lib.load()
    _lib.check(L.dx_dls_map(s.phys.ptr, t.ctypes.data, i.ctypes.data, len(i), reg, V.ctypes.data, q.ctypes.data,
                            st.ctypes.data))
    np.testing.assert_array_equal(st, 0)
    err, e32 = _check_against_numpy(s, types, ids, reg, q, st, V)
    print(f"{asset} {case} reg {reg:g}: worst device err {err:.3e} (float32 numpy {e32:.3e})")
    # dofs on no object's chain are exactly zero (the prop's free joint, the other fingers)
    off_chain = ~s.chain_dofs(types, ids)
    assert off_chain.any() or case == "fingertips"
    assert np.all(q[:, off_chain] == 0.0)
    assert np.any(q[:, ~off_chain] != 0.0)
    # the batch state is untouched, and a second call returns the same bits (status may be null)
    np.testing.assert_array_equal(s.phys.qpos, s.qpos)
    q2 = np.full((B, nv), np.nan, np.float32)
    _lib.check(L.dx_dls_map(s.phys.ptr, t.ctypes.data, i.ctypes.data, len(i), reg, V.ctypes.data, q2.ctypes.data,
                            None))
    np.testing.assert_array_equal(q2, q)


# --------------------------------------------------------------------------- #
# 3. rank guard
# --------------------------------------------------------------------------- #
def _mapper(model, types, ids, reg):
    from dexterity_amd.controllers import dls

    kind = {BODY: "body", GEOM: "geom", SITE: "site"}
    names = [model.compiled.names[kind[t]][i] for t, i in zip(types, ids)]
    return dls.DampedLeastSquaresMapper(dls.DampedLeastSquaresParameters(
        model=model, object_types=tuple(types), object_names=tuple(names), regularization_weight=reg))


def test_rank_guard_duplicate_site(gpu, scenes):
    """The same site twice: n3 = 6, rank 3.  Undamped, every env reports status 1 with a
    zero row (np.linalg.lstsq would return a least-squares solution: the stated deviation);
    damped, the system is regular and the numpy bound holds."""
    from dexterity_amd import _lib

    s = scenes("adroit_reach")
    site = _fingertip_sites(s.cm)[0]
    types, ids = [SITE, SITE], [site, site]
    V = np.random.RandomState(3).uniform(-0.1, 0.1, size=(B, 2, 3)).astype(np.float32)
    out = np.full((B, s.nv), np.nan, np.float32)
    q, st = _mapper(s.model, types, ids, 0.0).compute_joint_velocities_batch(s.phys, V, out=out)
    assert q is out
    np.testing.assert_array_equal(st, 1)
    np.testing.assert_array_equal(q, 0.0)
    q, st = _mapper(s.model, types, ids, 1e-2).compute_joint_velocities_batch(s.phys, V)
    np.testing.assert_array_equal(st, 0)
    _check_against_numpy(s, types, ids, 1e-2, q, st, V)
    # the reference's call shape raises instead of returning the zero row
    one = gpu.BatchedPhysics(s.model, 1)
    one.set(_lib.QPOS, s.qpos[:1])
    with pytest.raises(ValueError, match="regularization_weight > 0"):
        _mapper(s.model, types, ids, 0.0).compute_joint_velocities(one, [V[0, 0], V[0, 1]])
    v = _mapper(s.model, types, ids, 1e-2).compute_joint_velocities(one, [V[0, 0], V[0, 1]])
    np.testing.assert_array_equal(v, q[0].astype(np.float64))
    one.close()


# --------------------------------------------------------------------------- #
# 4. the reference's call shape; device-memory arguments
# --------------------------------------------------------------------------- #
def test_single_env_call_and_device_pointers(gpu, scenes):
    from dexterity_amd import _lib
    from dexterity_amd.manipulation import _copy_d2h, _copy_h2d, _hip_runtime

    s = scenes("shadow_reorient")
    types, ids = _case_objects(s.cm, "fingertips")
    m = _mapper(s.model, types, ids, 1e-5)
    V = np.random.RandomState(3).uniform(-0.1, 0.1, size=(B, len(ids), 3)).astype(np.float32)
    q, st = m.compute_joint_velocities_batch(s.phys, V)
    assert q.shape == (B, s.nv) and q.dtype == np.float32 and st.shape == (B,) and st.dtype == np.int32
    # one env, a sequence of nobj [3] arrays -> [nv] float64, equal to env 0 of the batch
    one = gpu.BatchedPhysics(s.model, 1)
    one.set(_lib.QPOS, s.qpos[:1])
    v = m.compute_joint_velocities(one, [V[0, k].astype(np.float64) for k in range(len(ids))],
                                   nullspace_bias=np.ones(s.nv))
    assert v.shape == (s.nv,) and v.dtype == np.float64
    np.testing.assert_array_equal(v, q[0].astype(np.float64))
    with pytest.raises(ValueError):
        m.compute_joint_velocities(one, [V[0, 0]])
    one.close()
    # targets / out / status in device memory: the same bits
    hip = _hip_runtime()
    bufs = [ctypes.c_void_p() for _ in range(3)]
    for b, n in zip(bufs, (V.nbytes, q.nbytes, st.nbytes)):
        assert hip.hipMalloc(ctypes.byref(b), n) == 0
    dV, dq, dst = (b.value for b in bufs)
    _copy_h2d(dV, V)
    _copy_h2d(dq, np.full_like(q, np.nan))
    _copy_h2d(dst, np.full_like(st, -1))
    rq, rst = m.compute_joint_velocities_batch(s.phys, dV, out=dq, status=dst)
    assert (rq, rst) == (dq, dst)
    s.phys.sync()  # the call was only enqueued
    q_dev, st_dev = np.empty_like(q), np.empty_like(st)
    _copy_d2h(q_dev, dq)
    _copy_d2h(st_dev, dst)
    np.testing.assert_array_equal(q_dev, q)
    np.testing.assert_array_equal(st_dev, st)
    # device targets with host outputs mix freely
    q_mix, st_mix = m.compute_joint_velocities_batch(s.phys, dV)
    np.testing.assert_array_equal(q_mix, q)
    np.testing.assert_array_equal(st_mix, st)
    for b in bufs:
        hip.hipFree(b)


# --------------------------------------------------------------------------- #
# 5. closed loop: consistency with the IK solver
# --------------------------------------------------------------------------- #
def test_closed_loop_reaches_what_the_ik_reaches(gpu, scenes, oracle_mod):
    """One IK step's joint velocities cannot be read out, so the mapper is used as the IK
    uses it (ik_solver.py:169-236): twist 0.95 (target - site) over 1 s steps, qpos += qdot
    on the host, clipped to the joint ranges, from the midrange start.  Every fingertip must
    come within 1e-3 inside 100 steps for at least as many of 10 reachable target sets as
    IKSolver.solve_batch(num_attempts=1, early_stop=True) solves."""
    from dexterity_amd import _lib
    from dexterity_amd.inverse_kinematics import IKSolver, hand_elements
    from tests.test_ik import _sample_reachable_targets

    s = scenes("adroit_reach")
    cm = s.cm
    sites, joints = (np.array(x) for x in hand_elements(cm, "adroit"))
    N = 10
    rs = np.random.RandomState(12345)
    targets = np.stack([_sample_reachable_targets(oracle_mod, s.om, cm, sites, joints, rs)[0] for _ in range(N)])
    solver = IKSolver(s.model, "adroit", num_envs=N)
    ik = solver.solve_batch(targets, linear_tol=1e-3, max_steps=100, early_stop=True, num_attempts=1)
    solver.close()

    m = _mapper(s.model, [SITE] * len(sites), list(sites), 1e-5)
    phys = gpu.BatchedPhysics(s.model, N)
    lo, hi = np.asarray(cm.jnt_range, np.float64)[joints].T
    qa, da = np.asarray(cm.jnt_qposadr)[joints], np.asarray(cm.jnt_dofadr)[joints]
    qpos = np.tile(np.asarray(cm.qpos0, np.float32), (N, 1))
    qpos[:, qa] = 0.5 * (lo + hi)
    solved = np.zeros(N, bool)
    for _ in range(100):
        phys.set(_lib.QPOS, qpos)
        phys.forward()
        tips = phys.get(_lib.SITE_XPOS).reshape(N, -1, 3)[:, sites]
        solved |= np.all(np.linalg.norm(targets - tips, axis=2) <= 1e-3, axis=1)
        if solved.all():
            break
        qdot, st = m.compute_joint_velocities_batch(phys, 0.95 * (targets - tips))
        assert not st.any()
        qpos[:, qa] = np.clip(qpos[:, qa] + qdot[:, da], lo, hi)
    phys.close()
    print(f"closed loop: mapper {int(solved.sum())}/{N}, IK attempt 0 {int(ik.success.sum())}/{N}")
    assert ik.success.sum() >= 1
    assert solved.sum() >= ik.success.sum()


# --------------------------------------------------------------------------- #
# 6. argument errors
# --------------------------------------------------------------------------- #
def test_argument_errors(scenes):
    from dexterity_amd import _lib

    s = scenes("adroit_reach")
    cm, ptr, L = s.cm, s.phys.ptr, _lib.load()
    EINVAL, ELIMIT = -1, -5
    V = np.zeros((B, 11, 3), np.float32)
    q = np.full((B, s.nv), 7.0, np.float32)
    jp = np.zeros((B, 11, 3, s.nv), np.float32)

    def both(types, ids, nobj, reg=1e-5):
        t = np.asarray(types, np.int32)
        i = np.asarray(ids, np.int32)
        rc_map = L.dx_dls_map(ptr, t.ctypes.data, i.ctypes.data, nobj, reg, V.ctypes.data, q.ctypes.data, None)
        msg_map = L.dx_last_error()
        rc_jac = L.dx_jac_object(ptr, t.ctypes.data, i.ctypes.data, nobj, jp.ctypes.data, None)
        msg_jac = L.dx_last_error()
        assert msg_map and msg_jac
        return rc_map, rc_jac, msg_map

    assert both([3], [0], 1)[:2] == (EINVAL, EINVAL)                     # mjOBJ_JOINT
    assert b"type" in both([0], [0], 1)[2]
    for typ, n in ((SITE, cm.nsite), (GEOM, cm.ngeom), (BODY, cm.nbody)):
        assert both([typ], [n], 1)[:2] == (EINVAL, EINVAL)               # one past the last id
        rc = both([typ], [-1], 1)
        assert rc[:2] == (EINVAL, EINVAL) and b"range" in rc[2]
    assert both([SITE], [0], 0)[:2] == (EINVAL, EINVAL)                  # nobj = 0
    assert both([SITE], [0], -3)[:2] == (EINVAL, EINVAL)
    rc = both([SITE] * 11, list(range(11)), 11)                          # n3 = 33
    assert rc[:2] == (ELIMIT, ELIMIT) and b"32" in rc[2]
    assert both([SITE] * 11, list(range(10)) + [cm.nsite], 11)[:2] == (EINVAL, EINVAL)
    t = np.array([SITE], np.int32)
    i = np.zeros(1, np.int32)
    for reg in (-1e-5, float("nan"), float("inf"), -float("inf")):
        assert L.dx_dls_map(ptr, t.ctypes.data, i.ctypes.data, 1, reg, V.ctypes.data, q.ctypes.data, None) == EINVAL
        assert b"regularization" in L.dx_last_error()
    assert L.dx_dls_map(ptr, t.ctypes.data, i.ctypes.data, 1, 1e-5, None, q.ctypes.data, None) == EINVAL
    assert L.dx_dls_map(ptr, t.ctypes.data, i.ctypes.data, 1, 1e-5, V.ctypes.data, None, None) == EINVAL
    assert L.dx_dls_map(ptr, None, i.ctypes.data, 1, 1e-5, V.ctypes.data, q.ctypes.data, None) == EINVAL
    # nothing was launched: the output buffer is as it was
    np.testing.assert_array_equal(q, 7.0)
    # the Python layer turns a code into DxError with the library's message
    with pytest.raises(_lib.DxError, match="32"):
        s.phys.jac_object([SITE] * 11, list(range(11)))
    # 10 sites (n3 = 30) is inside the limit
    t10, i10 = np.full(10, SITE, np.int32), np.arange(10, dtype=np.int32)
    assert L.dx_jac_object(ptr, t10.ctypes.data, i10.ctypes.data, 10, jp.ctypes.data, None) == 0
