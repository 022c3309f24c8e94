"""Per-env applied wrenches (include/dx.h dx_set_xfrc_env / dx_get_xfrc_env / dx_xfrc_ptr):
every env of a batch its own xfrc_applied rows, as in MjData, against the fp64 oracle given
the same rows, a known answer, and the exact contracts between the two modes."""

import ctypes
import functools
import os

import numpy as np
import pytest

from dexterity_amd import _lib
from dexterity_amd.mjcf.compiler import CompiledModel
from tests import contact_sense_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_parity import (TIE_QACC_CUBE, TIE_QPOS, _contact_tie, _f32, _load_states, _oracle_pair,
                                   _oracle_states)

pytestmark = pytest.mark.gpu

G = 9.81


@pytest.fixture(scope="module")
def gpu():
    from dexterity_amd import build, physics

    build.build()
    return physics


@functools.lru_cache(maxsize=None)
def _setup():
    """The 12 reorient parity states and one wrench row per state: the gravity compensation
    plus, on the cube and on the first finger's distal body, a force of random direction and
    a magnitude up to 5 m g of the cube, and a torque up to 5 m g x 1 cm."""
    from dexterity_amd import physics
    from oracle import oracle

    oracle.build()
    cm = CompiledModel.load(os.path.join(ROOT, "assets", "shadow_reorient.npz"))
    xfrc = physics.gravity_compensation(cm, "shadow_hand_e/")
    om, states = _oracle_states(oracle, cm, xfrc)
    names = cm.names["body"]
    cube, tip = names.index("prop/"), names.index("shadow_hand_e/ffdistal")
    rng = np.random.RandomState(3)
    top = 5 * cm.body_mass[cube] * G
    rows = np.repeat(np.asarray(xfrc, np.float64)[None], len(states), axis=0)
    for e in range(len(states)):
        for b in (cube, tip):
            for k, scale in ((0, top), (3, top * 0.01)):
                d = rng.normal(size=3)
                rows[e, b, k:k + 3] += rng.uniform(0, scale) * d / np.linalg.norm(d)
    rows32 = rows.astype(np.float32)
    return oracle, cm, xfrc, om, states, physics.Model(cm), rows32, cube, tip


def _load_rows(gpu, model, xfrc, states, rows32):
    phys = _load_states(gpu, model, xfrc, states)
    phys.set_xfrc(rows32)
    return phys


def _oracle_step(oracle, om, x, st, recs=None, step=True):
    d = oracle.OracleData(om)
    d.xfrc_applied[:] = np.asarray(x, np.float64).ravel()
    d.qpos[:], d.qvel[:], d.qacc_warmstart[:], d.ctrl[:] = st
    if recs is not None:
        d.set_contacts(np.asarray(recs, np.float64))
    d.step() if step else d.forward()
    return d


def test_parity_with_oracle(gpu):
    """forward() and step(1) with every state under its own row against the oracle given the
    same fp32-rounded row in d.xfrc_applied: qacc_smooth within 1e-5 of its scale; one
    physics step's qpos within 1e-6 and qvel within 5e-4 of the scale -- tests/test_gpu_parity.py's
    bounds for the shared form, with its handling of contact ties (_check_substep: the looser
    tie bounds, and tight agreement on the GPU's own contact list)."""
    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    n = len(states)
    x64 = rows32.astype(np.float64)
    probe = _load_rows(gpu, model, xfrc, states, rows32)
    np.testing.assert_array_equal(probe.xfrc_applied, rows32)
    probe.debug(True)
    probe.forward()
    a0 = probe.debug_get("qacc_smooth")
    con = probe.debug_get("contact")
    probe.close()
    ties = set()
    for e, st in enumerate(states):
        ds = _oracle_pair(oracle, om, cm, x64[e], st)
        scale = np.abs(ds[0].qacc_smooth).max()
        err = min(np.abs(a0[e] - d.qacc_smooth).max() for d in ds)
        print(f"state {e}: qacc_smooth err {err:.3g} of scale {scale:.4g}")
        assert err <= 1e-5 * scale, e
        for r in con[e, : (con[e, :, 15] != 0).sum()]:
            if _contact_tie(cm, ds, r):
                ties.add(e)
    # the rows matter: the cube's and the fingertip's accelerations differ from the shared form's
    shared = _load_states(gpu, model, xfrc, states)
    shared.debug(True)
    shared.forward()
    moved = np.abs(shared.debug_get("qacc_smooth") - a0).max(axis=1)
    assert (moved > 0).all() and moved.max() > 1.0, moved
    shared.close()
    phys = _load_rows(gpu, model, xfrc, states, rows32)
    phys.step(1)
    qpos, qvel = phys.qpos, phys.qvel
    phys.close()
    for e, st in enumerate(states):
        errs = []
        for y in (st, _f32(st)):
            d = _oracle_step(oracle, om, x64[e], y)
            errs.append((np.abs(qpos[e] - d.qpos).max(),
                         np.abs(qvel[e] - d.qvel).max() / max(1.0, np.abs(d.qacc_smooth).max())))
        qt, vt = (TIE_QPOS, TIE_QACC_CUBE) if e in ties else (1e-6, 5e-4)
        print(f"state {e}: one step (qpos, qvel/scale) {errs}, tie {e in ties}")
        if e in ties:
            d = _oracle_step(oracle, om, x64[e], _f32(st), con[e, : (con[e, :, 15] != 0).sum()])
            assert np.abs(qpos[e] - d.qpos).max() < 1e-6, (e, "on the GPU's contacts")
        assert any(q < qt and v < vt for q, v in errs), (e, e in ties, errs)
    assert len(ties) <= 2


def _air_batch(gpu, n=4):
    """n envs at qpos0 with the cube lifted to z = 0.5 m, at rest: contact-free."""
    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    q = np.repeat(np.asarray(cm.qpos0, np.float32)[None], n, axis=0)
    q[:, cm.nq - 7:cm.nq - 4] = [0.3, 0.3, 0.5]
    phys = gpu.BatchedPhysics(model, n)
    phys.set_xfrc(xfrc)
    phys.set(_lib.QPOS, q)
    return phys


def test_known_answer_and_independence(gpu):
    """Env e gets k_e m g z on the floating cube, k_e = e / 2: its translational acceleration is
    (k_e - 1) g z.  Both terms are fp32 values of size k_e g and g that cancel, so the 1e-5
    qacc_smooth bound is taken of max(1, k_e) g.  Changing one env's row moves no other env's
    result by a bit."""
    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    n = 4
    mg = cm.body_mass[cube] * G
    rows = np.repeat(np.asarray(xfrc, np.float32)[None], n, axis=0)
    k = np.arange(n) / 2.0
    rows[:, cube, 2] = (k * mg).astype(np.float32)
    phys = _air_batch(gpu, n)
    phys.set_xfrc(rows)
    phys.debug(True)
    phys.forward()
    assert not phys.get(_lib.NCON).any()
    a0 = phys.debug_get("qacc_smooth").astype(np.float64)
    qacc = phys.qacc.copy()
    lin = a0[:, cm.nv - 6:cm.nv - 3]
    for e in range(n):
        want = np.array([0.0, 0.0, (k[e] - 1.0) * G])
        err = np.abs(lin[e] - want).max()
        print(f"env {e}: k {k[e]} cube acceleration {lin[e]} err {err:.3g}")
        assert err <= 1e-5 * max(1.0, k[e]) * G
        assert np.abs(a0[e, cm.nv - 3:]).max() <= 1e-5 * G  # a force at the com turns nothing
    # only env 2's row changes: every other env's accelerations keep their bits
    rows2 = rows.copy()
    rows2[2, cube, :3] = [0.3, -0.2, 0.1]
    rows2[2, tip, :3] = [0.0, 0.5, 0.0]
    phys.set_xfrc(rows2[2:3], env0=2)
    np.testing.assert_array_equal(phys.xfrc_applied, rows2)
    phys.forward()
    q2 = phys.qacc
    others = [0, 1, 3]
    np.testing.assert_array_equal(q2[others], qacc[others])
    assert np.abs(q2[2, :cm.nv - 6] - qacc[2, :cm.nv - 6]).max() > 0.1
    assert np.abs(q2[2, cm.nv - 6:] - qacc[2, cm.nv - 6:]).max() > 0.1
    phys.step(3)
    phys.close()


def _outputs(phys, nsub):
    if nsub == 0:
        phys.forward()
    else:
        phys.step(nsub)
    return [phys.get(f).copy() for f in (_lib.QPOS, _lib.QVEL, _lib.QACC, _lib.QACC_WARMSTART, _lib.SITE_XPOS, _lib.NCON)]


@functools.lru_cache(maxsize=None)
def _shared_outputs(defer):
    """forward(), step(1), step(5) of the 12 states under the shared gravity compensation."""
    from dexterity_amd import physics

    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    out = []
    for nsub in (0, 1, 5):
        phys = _load_states(physics, model, xfrc, states)
        out.append(_outputs(phys, nsub))
        h = phys.health()
        phys.close()
    return out, h


@pytest.mark.parametrize("defer", [False, True], ids=["default", "DX_DEFER_AT"])
def test_equal_rows_are_the_shared_mode(gpu, monkeypatch, defer):
    """Per-env rows that all equal the shared array give the shared mode's bits for forward(),
    step(1) and step(5) -- also with every physics step that has more than one contact sent
    through the mid and overflow tiers (DX_DEFER_AT=1); returning to shared mode (the array
    again, or None and the array) equals a batch that never left it."""
    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    if defer:
        monkeypatch.setenv("DX_DEFER_AT", "1")
    want, health = _shared_outputs(defer)
    if defer:
        assert health["contact_deferred"] > 0, health
    n = len(states)
    same = np.repeat(np.asarray(xfrc, np.float32)[None], n, axis=0)
    for nsub, w in zip((0, 1, 5), want):
        phys = _load_rows(gpu, model, xfrc, states, same)
        assert phys.xfrc_ptr() is not None
        for x, y in zip(_outputs(phys, nsub), w):
            np.testing.assert_array_equal(x, y)
        phys.close()
    # per-env rows, then back: the array again, and None then the array
    for back in ("array", "none"):
        phys = _load_rows(gpu, model, xfrc, states, rows32)
        phys.forward()
        if back == "none":
            phys.set_xfrc(None)
            assert phys.xfrc_ptr() is None and not phys.xfrc_applied.any()
        phys.set_xfrc(xfrc)
        assert phys.xfrc_ptr() is None
        np.testing.assert_array_equal(phys.xfrc_applied, np.asarray(xfrc, np.float32))
        for f, s in zip((_lib.QPOS, _lib.QVEL, _lib.QACC_WARMSTART, _lib.CTRL), range(4)):
            phys.set(f, np.stack([st[s] for st in states]))
        for x, y in zip(_outputs(phys, 1), want[1]):
            np.testing.assert_array_equal(x, y)
        phys.close()


@pytest.mark.parametrize("defer", [False, True], ids=["default", "DX_DEFER_AT"])
def test_permuting_envs_permutes_outputs(gpu, monkeypatch, defer):
    """States and rows permuted together: the outputs are the same permutation, bit for bit
    (an env reads its own rows whichever workgroup, queue slot or tier runs it)."""
    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    if defer:
        monkeypatch.setenv("DX_DEFER_AT", "1")
    perm = np.random.RandomState(1).permutation(len(states))
    a = _load_rows(gpu, model, xfrc, states, rows32)
    b = _load_rows(gpu, model, xfrc, [states[i] for i in perm], rows32[perm])
    for nsub in (0, 1, 4):
        for x, y in zip(_outputs(a, nsub), _outputs(b, nsub)):
            np.testing.assert_array_equal(x[perm], y)
    a.close()
    b.close()


def test_read_back_partial_writes_and_pointer(gpu):
    """dx_get_xfrc_env returns what was set, partial env0 / n writes included; the first
    per-env write gives every other env the shared array (zeros without one); dx_xfrc_ptr
    fails in shared mode and names the rows in per-env mode; bad ranges change nothing;
    dx_reset leaves the rows alone."""
    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    L = _lib.load()
    nb, n = cm.nbody, 6
    x32 = np.asarray(xfrc, np.float32)
    for shared in (True, False):
        phys = gpu.BatchedPhysics(model, n)
        if shared:
            phys.set_xfrc(xfrc)
        base = x32 if shared else np.zeros_like(x32)
        p, stride = ctypes.c_void_p(), ctypes.c_int32(-1)
        assert L.dx_xfrc_ptr(phys.ptr, ctypes.byref(p), ctypes.byref(stride)) == -1
        assert b"shared" in L.dx_last_error() and phys.xfrc_ptr() is None
        assert phys.xfrc_applied.shape == (nb, 6)
        np.testing.assert_array_equal(phys.xfrc_applied, base)
        phys.set_xfrc(rows32[2:4], env0=3)
        want = np.repeat(base[None], n, axis=0)
        want[3:5] = rows32[2:4]
        np.testing.assert_array_equal(phys.xfrc_applied, want)
        assert L.dx_xfrc_ptr(phys.ptr, ctypes.byref(p), ctypes.byref(stride)) == 0
        assert p.value and stride.value == 6 * nb and phys.xfrc_ptr() == p.value
        got = np.empty((2, nb, 6), np.float32)
        assert L.dx_get_xfrc_env(phys.ptr, got.ctypes.data, 4, 2) == 0
        np.testing.assert_array_equal(got, want[4:6])
        phys.set_xfrc(rows32[7:8], env0=5)
        want[5] = rows32[7]
        np.testing.assert_array_equal(phys.xfrc_applied, want)
        for env0, cnt in ((-1, 1), (5, 2), (0, 7), (0, -1)):
            assert L.dx_set_xfrc_env(phys.ptr, rows32.ctypes.data, env0, cnt) == -1
            assert L.dx_get_xfrc_env(phys.ptr, got.ctypes.data, env0, cnt) == -1
        assert L.dx_set_xfrc_env(phys.ptr, None, 0, 1) == -1
        with pytest.raises(ValueError):
            phys.set_xfrc(rows32[:, :5])
        phys.reset()
        np.testing.assert_array_equal(phys.xfrc_applied, want)
        # a device-side write through the pointer is what the next step reads
        from dexterity_amd.manipulation import _copy_h2d

        want[0] = rows32[9]
        phys.sync()
        _copy_h2d(p.value, want[0])
        np.testing.assert_array_equal(phys.xfrc_applied, want)
        phys.close()


def test_sensors_read_the_env_rows(gpu):
    """Contact sensing: at the contact-free parity states cfrc_ext is the env's own applied
    wrench moved to the subtree com, within tests/test_gpu_contact_sense.py's 1e-5 of its
    scale against contact_sense_ref's restatement.  Torque sensors: env e's values under its
    own row are the bits of a shared-mode batch given that row."""
    oracle, cm, xfrc, om, states, model, rows32, cube, tip = _setup()
    n = len(states)
    x64 = rows32.astype(np.float64)
    phys = _load_rows(gpu, model, xfrc, states, rows32)
    phys.enable_contact_forces()
    phys.enable_sensors()
    phys.forward()
    cfrc = phys.cfrc_ext().astype(np.float64)
    torque = phys.get(_lib.SENSOR_TORQUE).copy()
    ncon = phys.get(_lib.NCON)[:, 0].copy()
    phys.close()
    free = 0
    for e in range(n):
        if ncon[e]:
            continue
        d = _oracle_step(oracle, om, x64[e], _f32(states[e]), step=False)
        assert d.ncon == 0
        applied = ref.applied_wrench(cm, x64[e], d.subtree_com, d.xipos)
        scale = np.abs(applied).max()
        err = np.abs(cfrc[e] - applied).max()
        other = ref.applied_wrench(cm, x64[(e + 1) % n], d.subtree_com, d.xipos)
        print(f"state {e}: xfrc part err {err:.3g} of scale {scale:.3g} (another env's row: {np.abs(cfrc[e] - other).max():.3g})")
        assert err <= 1e-5 * scale
        assert np.abs(cfrc[e] - other).max() > 1e-2 * scale
        free += 1
    assert free >= 2
    for e in (0, 4, 7, 10):
        one = _load_states(gpu, model, rows32[e], states)
        one.enable_sensors()
        one.forward()
        np.testing.assert_array_equal(one.get(_lib.SENSOR_TORQUE)[e], torque[e])
        one.close()
