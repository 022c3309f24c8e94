"""Contact force sensing, the parts that need no GPU: the numpy restatement against the
fp64 oracle's cfrc_ext, the CPU evidence behind the env's FIRST rule (a freshly spawned
prop touches nothing), the task's pad table, and the C ABI's new symbols."""

import os

import numpy as np
import pytest

from dexterity_amd import _lib, blob, manipulation
from dexterity_amd.mjcf.compiler import CompiledModel
from dexterity_amd.physics import gravity_compensation
from tests import contact_sense_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_parity import _oracle_forward, _oracle_states

# bodies that carry the fingertip sites: their distal geoms live on the parents, so none
# has a collision pair with the cube
SHADOW_TIP_BODIES = (8, 13, 18, 24, 30)


def _random_quat(rng):
    q = rng.randn(4)
    return q / np.linalg.norm(q)


def test_restatement_equals_oracle_cfrc_ext(oracle_mod, reorient_compiled):
    """The restatement (pyramid rows decoded as mju_decodePyramid, the contact rows the
    last rows of efc) equals the oracle's cfrc_ext within 1e-12 of the state's largest
    entry on the contact-rich reorient states; at least 6 of the 12 states have contacts."""
    cm = reorient_compiled
    xfrc = gravity_compensation(cm, "shadow_hand_e/")
    om, states = _oracle_states(oracle_mod, cm, xfrc)
    with_contacts = 0
    for st in states:
        d = _oracle_forward(oracle_mod, om, cm, xfrc, st)
        want = d.cfrc_ext.reshape(-1, 6)
        got = ref.cfrc_ext(cm, d.contacts(), d.efc_force, d.subtree_com, d.xipos, xfrc)
        scale = np.abs(want).max()
        assert scale > 0
        err = np.abs(got - want).max()
        print(f"ncon {d.ncon} scale {scale:.3g} err {err:.3g}")
        assert err <= 1e-12 * scale, (d.ncon, err, scale)
        assert not want[0].any()
        with_contacts += d.ncon > 0
        # the two parts add up, and the pads with partner -1 are the contact part's force
        cw = ref.contact_wrench(cm, d.contacts(), d.efc_force, d.subtree_com)
        pads = [(b, -1) for b in range(1, cm.nbody)]
        pf = ref.pad_forces(cm, d.contacts(), d.efc_force, d.xmat, pads)
        R = d.xmat.reshape(-1, 3, 3)
        for k, (b, _) in enumerate(pads):
            np.testing.assert_allclose(R[b] @ pf[k], cw[b, 3:], atol=1e-12 * max(scale, 1.0))
    assert with_contacts >= 6, with_contacts


@pytest.mark.parametrize("task_cls", [manipulation.ReOrient, manipulation.Handover])
def test_reset_states_are_contact_free(oracle_mod, task_cls):
    """The env's FIRST rule rests on this: with the hands at qpos0 and the prop anywhere in
    the task's spawn box at any orientation, the oracle finds no contact -- so a freshly
    reset env's true contact forces are zero (64 draws, and qpos0 itself)."""
    task = task_cls()
    cm = task.compiled
    om = oracle_mod.OracleModel(blob.pack(cm.arrays))
    rng = np.random.RandomState(0)
    lo, hi = np.array(task.config.prop_bbox_lower), np.array(task.config.prop_bbox_upper)
    a = task.prop_qadr
    d = oracle_mod.OracleData(om)
    d.forward()
    assert d.ncon == 0
    for _ in range(64):
        d = oracle_mod.OracleData(om)
        d.xfrc_applied[:] = task.gravity_compensation.ravel()
        d.qpos[a:a + 3] = rng.uniform(lo, hi)
        d.qpos[a + 3:a + 7] = _random_quat(rng)
        d.forward()
        assert d.ncon == 0, (d.qpos[a:a + 7], d.contacts()[:, 12:15])


def test_pad_table_shadow_reorient(reorient_compiled):
    """Every Shadow hand body with a collision pair against the cube, in body order: 23, all
    of the hand, none of them a fingertip-site body."""
    task = manipulation.ReOrient()
    cm = task.compiled
    pads = ref.prop_pads(cm, task.prop_body)
    names = cm.names["body"]
    assert len(pads) == 23
    bodies = [b for b, _ in pads]
    assert bodies == sorted(bodies) and all(p == task.prop_body for _, p in pads)
    assert all(names[b].startswith("shadow_hand_e/") for b in bodies)
    assert not set(bodies) & set(SHADOW_TIP_BODIES)
    # listed straight from the pair table
    gg = np.asarray(cm.arrays["gpair_geom"]).reshape(-1, 2)
    gb = np.asarray(cm.arrays["geom_bodyid"])
    pb = gb[gg]
    other = np.where(pb[:, 0] == task.prop_body, pb[:, 1], np.where(pb[:, 1] == task.prop_body, pb[:, 0], -1))
    assert bodies == sorted(set(int(b) for b in other if b > 0 and b != task.prop_body))


def test_pad_table_handover():
    task = manipulation.Handover()
    cm = task.compiled
    pads = ref.prop_pads(cm, task.prop_body)
    names = [cm.names["body"][b] for b, _ in pads]
    assert len(pads) == 46
    assert all(n.startswith("shadow_hand_left/") for n in names[:23])
    assert all(n.startswith("shadow_hand_right/") for n in names[23:])
    assert [n.split("/", 1)[1] for n in names[:23]] == [n.split("/", 1)[1] for n in names[23:]]


def test_abi_symbols_and_field_widths(reorient_compiled):
    from dexterity_amd import build

    build.build()
    lib = _lib.load()
    for s in ("dx_contact_enable", "dx_contact_set_pads", "dx_contact_npad", "dx_env_set_contact_forces",
              "dx_env_contact_force_dim", "dx_env_contact_force_bodies"):
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS
    assert (_lib.CFRC_EXT, _lib.PAD_FORCE, _lib.OUT_CONTACT_FORCE) == (17, 18, 11)
    b = blob.pack(reorient_compiled.arrays)
    m = lib.dx_model_load(b, len(b))
    assert m
    assert lib.dx_field_width(m, _lib.CFRC_EXT) == 6 * reorient_compiled.nbody
    assert lib.dx_field_width(m, _lib.PAD_FORCE) == 0  # no pads are set: they are a batch's
    assert lib.dx_field_width(m, _lib.SENSOR_TORQUE) == 3 * reorient_compiled.nbody
    assert lib.dx_field_width(m, 19) < 0
    lib.dx_model_free(m)
    # null handles are rejected before anything else
    assert lib.dx_contact_enable(None, 1) < 0
    assert lib.dx_contact_set_pads(None, None, 0) < 0
    assert lib.dx_env_set_contact_forces(None, 1) < 0
    assert lib.dx_env_contact_force_dim(None) < 0
    assert lib.dx_env_contact_force_bodies(None, None, 0) < 0
    with open(os.path.join(ROOT, "include", "dx.h")) as f:
        text = f.read()
    assert "DX_CFRC_EXT = 17" in text and "DX_PAD_FORCE = 18" in text and "DX_OUT_CONTACT_FORCE = 11" in text


def test_reach_raises():
    """The reach tasks have no prop: ValueError before the library is asked."""
    env = manipulation.GoalEnvironment.__new__(manipulation.GoalEnvironment)
    env.task = manipulation.Reach(hand="adroit")
    with pytest.raises(ValueError):
        env.enable_contact_forces()
    with pytest.raises(ValueError):
        env.contact_force_bodies
