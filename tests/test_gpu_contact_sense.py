"""Contact force sensing on the device (include/dx.h dx_contact_enable, DX_CFRC_EXT,
DX_PAD_FORCE, dx_env_set_contact_forces) against the fp64 restatement of
tests/contact_sense_ref.py and the oracle.

Parity is measured as a fraction of the state's largest contact-force magnitude, with the
oracle solving the GPU's own contact list (debug "contact" -> set_contacts), so the figure
is the fp32 solve's and the fp32 wrench arithmetic's, not a narrowphase tie's."""

import ctypes
import functools
import os

import numpy as np
import pytest

from dexterity_amd import _lib, blob
from dexterity_amd.mjcf.compiler import CompiledModel
from tests import contact_sense_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_contact_pool import bar_field, box_field
from tests.test_gpu_parity import _f32, _load_states, _oracle_states

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
# Worst measured |GPU - restatement| / (largest contact force of the state), over the
# contact-only wrenches and the pad forces of the 12 parity states, on an MI355X: 2.07e-6
# (17 fp32 ulps; a hand-hand state with 15 contacts at scale 118 N and a 3-contact cube
# state at 0.25 N give the two largest figures).  The bound is 4 x that, the margin
# tests/test_gpu_linalg.py gives for box-to-box spread.
PARITY_MEASURED = 2.1e-6
PARITY_BOUND = 4 * PARITY_MEASURED
FIRST, MID, LAST = 0, 1, 2


@pytest.fixture(scope="module")
def gpu():
    from dexterity_amd import build, physics

    build.build()
    return physics


@functools.lru_cache(maxsize=None)
def _setup():
    from dexterity_amd import physics
    from oracle import oracle

    oracle.build()
    cm = CompiledModel.load(os.path.join(ROOT, "assets", "shadow_reorient.npz"))
    xfrc = physics.gravity_compensation(cm, "shadow_hand_e/")
    om, states = _oracle_states(oracle, cm, xfrc)
    prop = cm.names["body"].index("prop/")
    pads = ref.prop_pads(cm, prop)
    pads = pads + [(b, -1) for b, _ in pads]
    return oracle, cm, xfrc, om, states, physics.Model(cm), pads


def _sense(phys, pads, torque=False):
    phys.enable_contact_forces()
    phys.set_contact_pads([b for b, _ in pads], [p for _, p in pads])
    if torque:
        phys.enable_sensors()


def _quat_to_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def _forward_run():
    """The 12 parity states in one batch, forward(): every output the tests below read."""
    from dexterity_amd import physics

    oracle, cm, xfrc, om, states, model, pads = _setup()
    phys = _load_states(physics, model, xfrc, states)
    phys.debug(True)
    _sense(phys, pads, torque=True)
    phys.forward()
    out = dict(cfrc=phys.cfrc_ext().copy(), pad=phys.pad_forces().copy(), ncon=phys.get(_lib.NCON)[:, 0].copy(),
               rec=phys.debug_get("contact").copy(), xquat=phys.get(_lib.XQUAT).reshape(len(states), -1, 4).copy(),
               torque=phys.get(_lib.SENSOR_TORQUE).copy())
    phys.close()
    return out


def _oracle_on_gpu_contacts(e):
    oracle, cm, xfrc, om, states, _, _ = _setup()
    run = _forward_run()
    d = oracle.OracleData(om)
    d.xfrc_applied[:] = np.asarray(xfrc, dtype=np.float32).astype(np.float64).ravel()
    d.qpos[:], d.qvel[:], d.qacc_warmstart[:], d.ctrl[:] = _f32(states[e])
    d.set_contacts(np.asarray(run["rec"][e, :run["ncon"][e]], dtype=np.float64))
    d.forward()
    return d


def test_parity_with_restatement(gpu):
    """forward() on the 12 oracle states; per state the oracle runs on the GPU's own contact
    list, and the restatement of its forces gives the contact-only wrench of every body and
    the pad forces (23 pads against the cube, the same 23 against any body).

    Measured on an MI355X: worst ratio 2.07e-6 of the state's largest contact force (wrench
    rows 3.5e-7 .. 2.07e-6, pad rows 1.2e-7 .. 2.04e-6 over the ten states with contacts);
    asserted at 4 x PARITY_MEASURED = 8.4e-6.  The xfrc part at the contact-free states is
    within 1e-5 of its scale, the project's qacc_smooth bound (measured 3.5e-7 and 7e-8 of
    29.4).  Of the three states built with the cube far away, one has 15 contacts between
    the hand's own bodies -- in the oracle too -- so two are contact-free and ten have
    contacts."""
    oracle, cm, xfrc, om, states, model, pads = _setup()
    run = _forward_run()
    x32 = np.asarray(xfrc, dtype=np.float32).astype(np.float64)
    worst, with_contacts, free = 0.0, 0, 0
    for e in range(len(states)):
        d = _oracle_on_gpu_contacts(e)
        assert d.ncon == run["ncon"][e]
        applied = ref.applied_wrench(cm, x32, d.subtree_com, d.xipos)
        got = run["cfrc"][e].astype(np.float64)
        assert not got[0].any()
        if d.ncon == 0:
            free += 1
            scale = np.abs(applied).max()
            err = np.abs(got - applied).max()
            print(f"state {e}: contact-free, xfrc part err {err:.3g} of scale {scale:.3g}")
            assert err <= 1e-5 * scale
            assert not run["pad"][e].any()
            continue
        with_contacts += 1
        cf = ref.contact_forces(cm, d.contacts(), d.efc_force)
        scale = max(np.linalg.norm(f) for _, _, _, f in cf)
        want = ref.contact_wrench(cm, d.contacts(), d.efc_force, d.subtree_com)
        want_pad = ref.pad_forces(cm, d.contacts(), d.efc_force, d.xmat, pads)
        r1 = np.abs(got - applied - want).max() / scale
        r2 = np.abs(run["pad"][e] - want_pad).max() / scale
        print(f"state {e}: ncon {d.ncon} scale {scale:.4g} wrench ratio {r1:.3g} pad ratio {r2:.3g}")
        worst = max(worst, r1, r2)
    print(f"worst ratio {worst:.3g} (bound {PARITY_BOUND:.3g})")
    assert with_contacts >= 6 and free >= 2, (with_contacts, free)
    assert worst <= 2e-2, "a ratio this large is a finding to explain, never a bound to adopt"
    assert worst <= PARITY_BOUND, worst


def test_exact_contracts(gpu):
    """forward() and step(1) from the same state, and two runs, are bit-equal; the
    contact-only forces cancel over the bodies where the world is not involved; pads
    with partner -1 are the body-frame contact force of cfrc_ext; the torque sensors do not
    change with contact sensing on."""
    oracle, cm, xfrc, om, states, model, pads = _setup()
    run = _forward_run()
    n = len(states)
    again = _load_states(gpu, model, xfrc, states)
    _sense(again, pads)
    again.step(1)
    np.testing.assert_array_equal(again.cfrc_ext(), run["cfrc"])
    np.testing.assert_array_equal(again.pad_forces(), run["pad"])
    again.close()
    twice = _load_states(gpu, model, xfrc, states)
    _sense(twice, pads)
    twice.forward()
    np.testing.assert_array_equal(twice.cfrc_ext(), run["cfrc"])
    np.testing.assert_array_equal(twice.pad_forces(), run["pad"])
    twice.close()
    plain = _load_states(gpu, model, xfrc, states)
    plain.enable_sensors()
    plain.forward()
    np.testing.assert_array_equal(plain.get(_lib.SENSOR_TORQUE), run["torque"])
    plain.close()

    x32 = np.asarray(xfrc, dtype=np.float32).astype(np.float64)
    geom_body = np.asarray(cm.arrays["geom_bodyid"])
    npad = len(pads) // 2
    checked = 0
    for e in range(n):
        force = run["cfrc"][e, :, 3:].astype(np.float64) - x32[:, :3]
        total = np.abs(force).sum()
        rec = run["rec"][e, :run["ncon"][e]]
        bodies = geom_body[rec[:, 13:15].astype(int)]
        if run["ncon"][e] and (bodies > 0).all():
            assert total > 0
            assert np.abs(force.sum(axis=0)).max() <= 64 * EPS * total
            checked += 1
        for k in range(npad, 2 * npad):
            b = pads[k][0]
            want = _quat_to_mat(run["xquat"][e, b].astype(np.float64)).T @ force[b]
            assert np.abs(run["pad"][e, k] - want).max() <= 8 * EPS * total, (e, k)
        # against the cube only: never more than against any body, equal where the body
        # touches nothing else
        assert (np.abs(run["pad"][e, :npad]).sum(axis=1) > 0).sum() <= (np.abs(run["pad"][e, npad:]).sum(axis=1) > 0).sum()
    assert checked >= 3, checked


def test_rejected_pads_change_nothing(gpu):
    oracle, cm, xfrc, om, states, model, pads = _setup()
    run = _forward_run()
    L = _lib.load()
    phys = _load_states(gpu, model, xfrc, states)
    _sense(phys, pads)
    nb = cm.nbody
    for bodies, partners, code in (([0], [-1], -1), ([nb], [-1], -1), ([1], [nb], -1), ([1], [-2], -1),
                                   (list(range(1, 2)) * 65, [-1] * 65, -5)):
        table = np.array(list(zip(bodies, partners)), dtype=np.int32)
        assert L.dx_contact_set_pads(phys.ptr, table.ctypes.data, len(table)) == code
        assert L.dx_contact_npad(phys.ptr) == len(pads)
    phys.forward()
    np.testing.assert_array_equal(phys.pad_forces(), run["pad"])
    np.testing.assert_array_equal(phys.cfrc_ext(), run["cfrc"])
    phys.set_contact_pads([])
    assert L.dx_contact_npad(phys.ptr) == 0 and phys.pad_forces().shape == (len(states), 0, 3)
    phys.forward()
    np.testing.assert_array_equal(phys.cfrc_ext(), run["cfrc"])
    phys.close()


@pytest.mark.parametrize("field", ["boxes", "bars"])
def test_resting_cubes_known_answer(gpu, oracle_mod, field):
    """Ten cubes resting on the ground (40 contacts: the mid tier) and ten bars of eight
    cubes with two lifted (256 contacts: the overflow tier), 16 physics steps from 1 mm of
    penetration (eight time constants of the contact's critically damped 10 ms): every
    resting body's cfrc_ext force is its weight within the 5 % of m g the oracle's resting
    test uses, a lifted one's is zero, and forces and torques are within the parity bound of
    the oracle's after the same steps.

    The parity ratio's denominator here is the largest sum of contact-force magnitudes on
    one body, not the largest single force: a body's wrench is the fp32 sum of its contacts'
    (4 per cube, 32 per bar, all equal), whose rounding grows with that sum, while in the
    parity states a body carries one to a few contacts and the two scales agree within a
    small factor.  Measured on an MI355X: 7.7e-7 (cubes) and 5.0e-7 (bars) of that sum --
    3.1e-6 and 1.6e-5 of the largest single force, 0.156 N."""
    cm = box_field(10) if field == "boxes" else bar_field()
    q = cm.qpos0.copy()
    lifted = []
    if field == "bars":
        lifted = [3, 6]
        for b in lifted:
            q[7 * b + 2] += 0.05
    nstep = 16
    ph = gpu.BatchedPhysics(gpu.Model(cm), 3)
    ph.set(_lib.QPOS, np.stack([q] * 3))
    ph.enable_contact_forces()
    ph.health_clear()
    ph.step(nstep)
    h = ph.health()
    ncon = ph.get(_lib.NCON)[:, 0]
    got = ph.cfrc_ext().astype(np.float64)
    ph.close()
    assert h["contact_overflow"] == 0 and h["diverged"] == 0 and h["contact_deferred"] >= 3, h
    assert (ncon == (40 if field == "boxes" else 256)).all(), ncon
    np.testing.assert_array_equal(got[1:], got[:1].repeat(2, axis=0))
    om = oracle_mod.OracleModel(blob.pack(cm.arrays))
    d = oracle_mod.OracleData(om)
    d.qpos[:] = np.asarray(q, np.float32)
    for _ in range(nstep):
        d.step()
    want = d.cfrc_ext.reshape(-1, 6)
    g = 9.81
    for b in range(1, cm.nbody):
        w = cm.body_mass[b] * g
        target = np.zeros(3) if (b - 1) in lifted else np.array([0.0, 0.0, w])
        assert np.abs(got[0, b, 3:] - target).max() <= 0.05 * w, (b, got[0, b], w)
        if (b - 1) in lifted:
            assert not got[0, b].any()
    per_body = np.zeros(cm.nbody)
    single = 0.0
    for b1, b2, _, f in ref.contact_forces(cm, d.contacts(), d.efc_force):
        per_body[b1] += np.linalg.norm(f)
        per_body[b2] += np.linalg.norm(f)
        single = max(single, np.linalg.norm(f))
    scale = per_body[1:].max()
    ratio = np.abs(got[0] - want).max() / scale
    print(f"{field}: largest contact force {single:.4g}, largest sum on a body {scale:.4g}, "
          f"worst |GPU - oracle| ratio {ratio:.3g} ({ratio * scale / single:.3g} of the single force)")
    assert ratio <= PARITY_BOUND, ratio


# --------------------------------------------------------------------------- env
def _env(domain="reorient", n=16, contact=True, **kw):
    from dexterity_amd import manipulation

    env = manipulation.load(domain, "state_dense", num_envs=n, **kw)
    if contact:
        env.enable_contact_forces()
    return env


def _step_dev(env, i):
    env.step(env.sample_actions(i), device_action=True)


def _raw_state(env):
    """The checkpoint's bytes, field by field, without the two fields that hold measured
    shader cycles and the dispatch order built from them (they differ between any two
    runs); their sizes still count."""
    L = _lib.load()
    n = _lib.check(L.dx_env_save(env.ptr, None, 0))
    buf = np.empty(n, dtype=np.uint8)
    _lib.check(L.dx_env_save(env.ptr, buf.ctypes.data, n))
    fields = env._state_fields()
    assert sum(nb for _, _, nb in fields) == n
    return [(name, nb, None if name in ("step_cost", "order") else buf[off:off + nb].copy())
            for name, off, nb in fields]


ENV_KW = dict(seed=11, time_limit=0.3)


def test_env_rows_match_a_separate_batch(gpu, tmp_path):
    """Reorient, 16 envs, 30 random-agent steps with auto-resets (episodes of 12 control
    steps): MID and LAST rows are bit-equal to DX_PAD_FORCE of a separate BatchedPhysics with
    the same pads stepped from the env's pre-step state and ctrl; FIRST rows and the rows
    after reset are exactly zero; at least 20 % of MID env-steps carry force (the oracle's
    random agent: 48 %); a checkpoint at step 10 loaded into a fresh configured env
    continues bit for bit."""
    env = _env(**ENV_KW)
    task = env.task
    names = task.compiled.names["body"]
    pads = ref.prop_pads(task.compiled, task.prop_body)
    assert env.contact_force_bodies == [names[b] for b, _ in pads] and len(pads) == 23
    spec = env.observation_spec()
    assert list(spec)[-1] == "hand_contact_forces" and spec["hand_contact_forces"].shape == (23, 3)
    twin = gpu.BatchedPhysics(env.model, env.num_envs)
    twin.set_xfrc(task.gravity_compensation)
    twin.enable_contact_forces()
    twin.set_contact_pads([b for b, _ in pads], task.prop_body)
    ts = env.reset()
    assert not env.contact_forces().any() and not ts.observation["hand_contact_forces"].any()
    assert (ts.step_type == FIRST).all()
    mid = touched = first = last = 0
    fresh = None
    nsub = task.config.n_sub_steps
    for i in range(30):
        ph = env.physics
        pre = [ph.get(f) for f in (_lib.QPOS, _lib.QVEL, _lib.QACC_WARMSTART)]
        _step_dev(env, i)
        ts = env.timestep()
        rows = env.contact_forces()
        np.testing.assert_array_equal(ts.observation["hand_contact_forces"], rows.astype(np.float64))
        for f, v in zip((_lib.QPOS, _lib.QVEL, _lib.QACC_WARMSTART), pre):
            twin.set(f, v)
        twin.set(_lib.CTRL, ph.get(_lib.CTRL))
        twin.step(nsub)
        want = twin.pad_forces()
        assert np.isfinite(rows).all()
        for e in range(env.num_envs):
            if ts.step_type[e] == FIRST:
                assert not rows[e].any()
                first += 1
            else:
                np.testing.assert_array_equal(rows[e], want[e])
                mid += ts.step_type[e] == MID
                last += ts.step_type[e] == LAST
                touched += ts.step_type[e] == MID and rows[e].any()
        if i == 9:
            path = str(tmp_path / "ckpt.npz")
            env.save(path)
            with np.load(path) as z:
                assert "contact_force" in z.files
            fields = [name for name, _, _ in env._state_fields()]
            assert fields[-1] == "contact_force"
            fresh = _env(**ENV_KW)
            fresh.load(path)
            np.testing.assert_array_equal(fresh.contact_forces(), rows)
            off = _env(contact=False, **ENV_KW)
            with pytest.raises(ValueError, match="contact forces"):
                off.load(path)
            off.close()
        elif fresh is not None:
            _step_dev(fresh, i)
            np.testing.assert_array_equal(fresh.contact_forces(), rows)
            np.testing.assert_array_equal(fresh.timestep().observation["prop/position"], ts.observation["prop/position"])
    print(f"MID {mid} (with force {touched}), LAST {last}, FIRST {first}")
    assert first >= 16 and last >= 16
    assert touched >= 0.2 * mid, (touched, mid)
    for x in (env, fresh):
        x.close()
    twin.close()


def test_env_off_is_unchanged(gpu):
    """Switched on (before the reset, or mid-episode) and then off, an env steps exactly as
    one never configured: outputs and the checkpoint bytes alike; the output is refused
    while off, and enabling mid-episode leaves zeros until the next step."""
    L = _lib.load()
    plain = _env(n=8, contact=False, **ENV_KW)
    before = _env(n=8, **ENV_KW)
    mid = _env(n=8, contact=False, **ENV_KW)
    envs = (plain, before, mid)
    keys = list(plain.observation_spec())
    for env in envs:
        env.reset()
        for i in range(6):
            _step_dev(env, i)
    mid.enable_contact_forces()
    assert L.dx_env_contact_force_dim(mid.ptr) == 69
    assert not mid.contact_forces().any()
    _step_dev(mid, 6)
    _step_dev(before, 6)
    _step_dev(plain, 6)
    np.testing.assert_array_equal(mid.contact_forces(), before.contact_forces())
    for env in (before, mid):
        env.enable_contact_forces(False)
        assert L.dx_env_contact_force_dim(env.ptr) == 0 and env.contact_force_pads == 0
        p = ctypes.c_void_p()
        assert L.dx_env_output(env.ptr, _lib.OUT_CONTACT_FORCE, ctypes.byref(p)) == -1
        assert b"contact forces" in L.dx_last_error()
        with pytest.raises(_lib.DxError):
            env.contact_forces()
        assert list(env.observation_spec()) == keys
    ended = False
    for i in range(7, 16):
        outs = []
        for env in envs:
            _step_dev(env, i)
            ts = env.timestep()
            assert list(ts.observation) == keys
            outs.append((np.concatenate([ts.observation[k] for k in keys], axis=1), ts.reward, ts.discount,
                         ts.step_type, _raw_state(env)))
        ended = ended or (outs[0][3] == LAST).any()
        for other in outs[1:]:
            for x, y in zip(outs[0][:4], other[:4]):
                np.testing.assert_array_equal(x, y)
            assert [f[:2] for f in outs[0][4]] == [f[:2] for f in other[4]]
            for (name, _, x), (_, _, y) in zip(outs[0][4], other[4]):
                if x is not None:
                    np.testing.assert_array_equal(x, y, err_msg=name)
    assert ended
    for env in envs:
        env.close()


def _run_rows(env, how, steps=12):
    from dexterity_amd.manipulation import _copy_d2h

    env.reset()
    rows, types = [env.contact_forces()], []
    for i in range(steps):
        if how == "device":
            _step_dev(env, i)
        elif how == "random":
            env.step_random(i)
        else:  # the host call shape: its own TimeStep carries the same rows
            ptr = env.sample_actions(i)
            env.physics.sync()
            a = np.empty((env.num_envs, env.model.nu), np.float32)
            _copy_d2h(a, ptr)
            ts = env.step(a)
            np.testing.assert_array_equal(ts.observation["hand_contact_forces"], env.contact_forces().astype(np.float64))
        rows.append(env.contact_forces())
        types.append(env.timestep().step_type)
    env.close()
    return rows, np.array(types)


PATH_KW = dict(seed=23, time_limit=0.2)


@functools.lru_cache(maxsize=None)
def _default_rows():
    return _run_rows(_env(n=6, **PATH_KW), "device")


@pytest.mark.parametrize("path", ["DX_NO_FUSE", "DX_DEFER_AT", "random", "host"])
def test_env_paths_agree(gpu, monkeypatch, path):
    """The task kernels around the step kernel (DX_NO_FUSE=1: the step types are written
    after the step's launches), every step with more than one contact sent to the mid tier
    (DX_DEFER_AT=1: the stash is that tier's), dx_env_step_random and the host call shape
    each give the default run's rows on the same seed, bit for bit, over episodes of eight
    control steps."""
    want, types = _default_rows()  # (run, the first time, before the variable is set)
    assert (types == LAST).any() and (types == FIRST).any() and any(r.any() for r in want)
    if path.startswith("DX_"):
        monkeypatch.setenv(path, "1")
    got, _ = _run_rows(_env(n=6, **PATH_KW), path if not path.startswith("DX_") else "device")
    assert len(got) == len(want) == 13
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)


def test_env_handover_and_reach(gpu):
    """The handover reports 2 x 23 pads and finite rows; the reach tasks refuse."""
    L = _lib.load()
    env = _env("bimanual", 4, seed=3)
    assert env.contact_force_pads == 46 and len(env.contact_force_bodies) == 46
    env.reset()
    for i in range(12):
        env.step_random(i)
    rows = env.contact_forces()
    assert rows.shape == (4, 46, 3) and np.isfinite(rows).all()
    env.close()
    reach = _env("reach", 2, contact=False, seed=3)
    with pytest.raises(ValueError):
        reach.enable_contact_forces()
    assert L.dx_env_set_contact_forces(reach.ptr, 1) == -1
    assert L.dx_env_contact_force_dim(reach.ptr) == 0
    reach.close()
