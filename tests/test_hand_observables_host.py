"""The optional hand observables without a GPU: the numpy restatement that
tests/test_gpu_hand_observables.py holds the device to, checked on the fp64 oracle alone,
and the host surface (exports, header, constants, name handling, wrappers)."""

import os
import re

import numpy as np
import pytest

from dexterity_amd import _lib
from oracle import task_ref
from tests.conftest import ROOT, random_hand_state
from tests.test_gpu_hand_observables import (NAMES, quat_from_mat, reference_extras, root_bodies, root_frame,
                                             task_tip_sites)


def _tasks():
    from dexterity_amd import manipulation

    return {"reorient": manipulation.ReOrient(), "reach": manipulation.Reach(hand="adroit"),
            "reach_shadow": manipulation.Reach(hand="shadow"), "bimanual": manipulation.Handover()}


@pytest.fixture(scope="module")
def tasks():
    return _tasks()


def _posed(oracle_mod, task, rng, n):
    from dexterity_amd import blob

    om = oracle_mod.OracleModel(blob.pack(task.compiled.arrays))
    for _ in range(n):
        d = oracle_mod.OracleData(om)
        d.reset()
        # joints over their WHOLE range: fingertip orientations then reach small |w|
        d.qpos[:], d.qvel[:] = random_hand_state(task.compiled, rng, frac=1.0)
        d.observe()
        yield d


@pytest.mark.parametrize("name", ["reorient", "reach", "reach_shadow", "bimanual"])
def test_restatement_on_the_oracle(oracle_mod, tasks, name):
    """Over random poses of every shipped scene: the eigenvector quaternion of site_xmat is
    quat_mul(xquat[body], site_quat) to 1e-12 up to sign, unit and with w >= 0; the ego
    definition, inverted through the root body's inertial frame, reproduces site_xpos;
    and the angular velocity is the site's body's (mj_objectVelocity's rotation part does
    not depend on the point)."""
    task = tasks[name]
    cm = task.compiled
    site_body = np.asarray(cm.arrays["site_bodyid"]).ravel()
    site_quat = np.asarray(cm.arrays["site_quat"], dtype=np.float64).reshape(-1, 4)
    tips = task_tip_sites(task)
    nt = task.ntips // len(task.hand_names)
    rng = np.random.RandomState(5)
    wmin = 1.0
    for d in _posed(oracle_mod, task, rng, 50):
        xquat = d.xquat.reshape(-1, 4)
        ref = reference_extras(d, task)
        assert list(ref) == [f"{h}/{n}" for h in task.hand_names for n in NAMES]
        for h, (hand, root) in enumerate(zip(task.hand_names, root_bodies(task))):
            sites = tips[h * nt:(h + 1) * nt]
            quats = ref[f"{hand}/fingertip_orientations"].reshape(-1, 4)
            for s, q in zip(sites, quats):
                p = task_ref.quat_mul(xquat[site_body[s]], site_quat[s])
                p = p / np.linalg.norm(p)
                assert min(np.abs(q - p).max(), np.abs(q + p).max()) <= 1e-12
                assert q[0] >= 0 and abs(np.linalg.norm(q) - 1) <= 1e-12
                wmin = min(wmin, q[0])
            xipos, ximat = root_frame(d, cm, root)
            ego = ref[f"{hand}/fingertip_positions_ego"].reshape(-1, 3)
            np.testing.assert_allclose(xipos + ego @ ximat.T, d.site_xpos.reshape(-1, 3)[sites], rtol=0, atol=1e-12)
            ang = ref[f"{hand}/fingertip_angular_velocities"].reshape(-1, 3)
            for s, w in zip(sites, ang):
                np.testing.assert_allclose(w, d.object_velocity("xbody", site_body[s])[3:], rtol=0, atol=1e-12)
    assert wmin < 0.5  # the poses do turn the fingertips


def test_quat_from_mat_sign():
    """w >= 0 also for rotations by more than half a turn about an axis."""
    for ang in (0.3, 3.0, 3.3, 6.0):
        c, s = np.cos(ang), np.sin(ang)
        q = quat_from_mat([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        want = np.array([np.cos(ang / 2), 0, 0, np.sin(ang / 2)])
        want = -want if want[0] < 0 else want
        np.testing.assert_allclose(q, want, atol=1e-12)


def test_adroit_ego_frame_is_not_the_body_frame(oracle_mod, tasks):
    """Adroit's forearm has a rotated inertial frame, so the GPU parity bound (1e-5) tells
    the two candidate ego frames apart by orders of magnitude."""
    task = tasks["reach"]
    d = next(_posed(oracle_mod, task, np.random.RandomState(1), 1))
    root = root_bodies(task)[0]
    ego = reference_extras(d, task)["adroit_hand/fingertip_positions_ego"].reshape(-1, 3)
    sites = task_tip_sites(task)
    body = (d.site_xpos.reshape(-1, 3)[sites] - d.xpos.reshape(-1, 3)[root]) @ d.xmat.reshape(-1, 3, 3)[root]
    assert np.abs(ego - body).max() > 1e-2


def test_exports_header_and_constants():
    assert {"dx_env_set_hand_observables", "dx_env_hand_obs_dim"} <= set(_lib.EXPORTS)
    with open(os.path.join(ROOT, "include", "dx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"int dx_env_set_hand_observables\(dx_env\* e, const dx_hand_obs\* cfg\);", text)
    assert re.search(r"int dx_env_hand_obs_dim\(const dx_env\* e\);", text)
    assert re.search(r"DX_OUT_HAND_OBS = 9\b", text)
    for name, bit in (("JOINT_POSITIONS", 1), ("TIP_ORIENTATIONS", 2), ("TIP_ANGULAR_VELOCITIES", 4),
                      ("TIP_POSITIONS_EGO", 8)):
        assert re.search(rf"DX_HOBS_{name} = {bit}\b", text)
        assert getattr(_lib, f"HOBS_{name}") == bit
    assert _lib.OUT_HAND_OBS == 9
    import ctypes

    assert ctypes.sizeof(_lib.HandObs) == 16


def test_names_order_and_root_bodies(tasks):
    """The Python table is in the reference's declaration order with the header's bits,
    and every shipped hand has the root body the reference names."""
    from dexterity_amd import manipulation

    assert tuple(manipulation.HAND_EXTRA_OBSERVABLES) == NAMES
    assert [v[0] for v in manipulation.HAND_EXTRA_OBSERVABLES.values()] == [1, 2, 4, 8]
    assert root_bodies(tasks["bimanual"]) == [1, 31]
    for name in ("reorient", "reach", "reach_shadow"):
        assert tasks[name].hand_names == (tasks[name].hand_name,)
        assert root_bodies(tasks[name]) == [1]


def test_wrappers_pass_enable_observables_through():
    from dexterity_amd import wrappers

    class Env:
        action_config = dict(noise_scale=None, noise_seed=None, smooth_alpha=None, previous_action=False)
        hand_observables = ()

        def configure_actions(self, **kw):
            self.action_config = kw

        def enable_observables(self, names):
            self.hand_observables = tuple(names)

    env = Env()
    wrapped = wrappers.SmoothAction(wrappers.PreviousAction(env), 0.5)
    wrapped.enable_observables(["joint_positions"])
    assert env.hand_observables == ("joint_positions",) == wrapped.hand_observables
