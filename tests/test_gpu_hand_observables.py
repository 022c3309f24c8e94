"""The optional hand observables on the device (GoalEnvironment.enable_observables,
include/dx.h dx_env_set_hand_observables; dx_observe.hip): joint_positions,
fingertip_orientations, fingertip_angular_velocities and fingertip_positions_ego against
the fp64 oracle on every task, their bit-equalities with the batch arrays, subsets and
layout, off = never configured, enabling mid-episode, every step path, shards, the
checkpoint and the rejections.

The numpy restatement of the four definitions (dexterous_hand.py:250-252, 286-295,
312-325, 327-350) is here; tests/test_hand_observables_host.py checks it on the oracle
alone.
"""

import ctypes
import functools

import numpy as np
import pytest

from dexterity_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = ("joint_positions", "fingertip_orientations", "fingertip_angular_velocities", "fingertip_positions_ego")
TASKS = [("reorient", "state_dense"), ("reach", "state_dense"), ("reach_shadow", "state_dense"),
         ("bimanual", "state_dense")]
FIRST, MID, LAST = 0, 1, 2
BOUND = 1e-5  # tests/test_gpu_env.py _check_observation: max|got - ref| / max(1, max|ref|) per key
W_SMALL = 1e-4  # below this |w| of the reference, a quaternion is compared up to a common sign


# --------------------------------------------------------------------------- #
# the four definitions in numpy (fp64), from the oracle's state after observe()
# --------------------------------------------------------------------------- #
def quat_from_mat(R):
    """[3P] dm_robotics.transformations.mat_to_quat: the top eigenvector of the symmetric
    K matrix of R, negated when its w is negative -- canonical with w >= 0."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = R.flat
    K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0],
                  [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0],
                  [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                  [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)  # (reads the lower triangle)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -q if q[0] < 0 else q


def quat_to_mat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def task_tip_sites(task):
    if hasattr(task, "tip_sites"):
        return list(task.tip_sites)
    return list(range(task.tip_site0, task.tip_site0 + task.ntips))


def root_bodies(task):
    bodies = task.compiled.names["body"]
    return [bodies.index(f"{h}/forearm") for h in task.hand_names]


def root_frame(d, compiled, root):
    """(xipos, ximat) of a body: MuJoCo's frame of objtype / reftype "body" [3P]."""
    iquat = np.asarray(compiled.body_iquat, dtype=np.float64).reshape(-1, 4)[root]
    ximat = d.xmat.reshape(-1, 3, 3)[root] @ quat_to_mat(iquat)
    return d.xipos.reshape(-1, 3)[root].copy(), ximat


def reference_extras(d, task, names=NAMES):
    """The enabled observables of every hand, keyed and ordered as the env's TimeStep."""
    cm = task.compiled
    nh = len(task.hand_names)
    hnq, nt = task.hand_nq // nh, task.ntips // nh
    tips = task_tip_sites(task)
    site_xmat = d.site_xmat.reshape(-1, 3, 3)
    site_xpos = d.site_xpos.reshape(-1, 3)
    xmat = d.xmat.reshape(-1, 3, 3)
    xipos = d.xipos.reshape(-1, 3)
    iquat = np.asarray(cm.body_iquat, dtype=np.float64).reshape(-1, 4)
    out = {}
    for h, (hand, root) in enumerate(zip(task.hand_names, root_bodies(task))):
        sites = tips[h * nt:(h + 1) * nt]
        Ri = quat_to_mat(iquat[root])
        vals = {
            "joint_positions": np.array(d.qpos[h * hnq:(h + 1) * hnq], dtype=np.float64),
            "fingertip_orientations": np.concatenate([quat_from_mat(site_xmat[s]) for s in sites]),
            "fingertip_angular_velocities": np.concatenate([d.object_velocity("site", s)[3:] for s in sites]),
            "fingertip_positions_ego": np.concatenate(
                [Ri.T @ (xmat[root].T @ (site_xpos[s] - xipos[root])) for s in sites]),
        }
        for n in NAMES:
            if n in names:
                out[f"{hand}/{n}"] = vals[n]
    return out


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def orientation_err(got, ref):
    """Component-wise where the reference's |w| > W_SMALL, up to a common sign below."""
    worst = 0.0
    for g, r in zip(got.reshape(-1, 4), ref.reshape(-1, 4)):
        e = np.abs(g - r).max()
        if abs(r[0]) <= W_SMALL:
            e = min(e, np.abs(g + r).max())
        worst = max(worst, float(e))
    return worst / max(1.0, np.abs(ref).max())


# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def built():
    from dexterity_amd import build

    build.build()


def _load(domain, n, seed=13, observables=NAMES, **kw):
    from dexterity_amd import manipulation

    env = manipulation.load(domain, "state_dense", seed=seed, num_envs=n, **kw)
    if observables is not None:
        env.enable_observables(observables)
    return env


def _step_dev(env, i):
    env.step(env.sample_actions(i), device_action=True)


def _snap(env):
    """The extras' rows and the outputs they must agree with, of the env's current state."""
    ts = env.timestep()
    ph = env.physics
    return dict(ts=ts, rows=env.hand_obs(), qpos=ph.get(_lib.QPOS), qvel=ph.get(_lib.QVEL),
                site_vel=ph.get(_lib.SITE_VEL))


@functools.lru_cache(maxsize=None)
def _parity_run(domain):
    """8 envs, all four observables, reset + 12 steps of sample_actions with time_limit
    0.05 s: the records of items 1 and 2, computed once per task.  Reorient and the
    handover (0.025 s control steps) then end an episode every second step.  A reach
    episode starts at 0.04 s -- the goal's two rollout steps -- so at that limit its every
    step is LAST or FIRST: 6 more steps of a second batch with time_limit 0.11 s add its
    MID steps."""
    recs = []
    for limit, steps in ((0.05, 12), (0.11, 6)):
        env = _load(domain, 8, time_limit=limit)
        env.reset()
        recs.append(_snap(env))
        for i in range(steps):
            _step_dev(env, i)
            recs.append(_snap(env))
        task, blob = env.task, env.model.blob
        env.close()
    return task, blob, recs


@pytest.mark.parametrize("domain", [d for d, _ in TASKS])
def test_matches_oracle(built, oracle_mod, domain):
    """Item 1: every float of the four observables within 1e-5 of its key's scale of the
    fp64 restatement on the env's own state, after the reset and each of 12 steps that
    cover freshly reset (FIRST), LAST and MID envs; the device's w >= 0 exactly.  Adroit's
    forearm has a rotated inertial frame, so its ego positions tell the two frames apart."""
    task, blob, recs = _parity_run(domain)
    om = oracle_mod.OracleModel(blob)
    worst, seen = {}, set()
    for rec in recs:
        ts = rec["ts"]
        seen |= set(int(s) for s in ts.step_type)
        for e in range(len(ts.step_type)):
            d = oracle_mod.OracleData(om)
            d.qpos[:], d.qvel[:] = rec["qpos"][e], rec["qvel"][e]
            d.observe()
            ref = reference_extras(d, task)
            assert list(ts.observation)[-len(ref):] == list(ref)
            for k, r in ref.items():
                g = ts.observation[k][e]
                assert g.shape == r.shape and g.dtype == np.float64, k
                if k.endswith("fingertip_orientations"):
                    assert (g.reshape(-1, 4)[:, 0] >= 0).all(), (k, g)
                    err = orientation_err(g, r)
                else:
                    err = rel_err(g, r)
                worst[k] = max(worst.get(k, 0.0), err)
    print(domain, {k: f"{v:.2e}" for k, v in worst.items()})
    assert seen == {FIRST, MID, LAST}
    assert len(worst) == 4 * len(task.hand_names)
    for k, err in worst.items():
        assert err <= BOUND, (k, err, worst)


@pytest.mark.parametrize("domain", [d for d, _ in TASKS])
def test_bit_equalities(built, oracle_mod, domain):
    """Item 2, on the same batch: joint_positions is DX_QPOS, the angular velocities are
    words 3-5 of DX_SITE_VEL, bit for bit; and the ego positions, moved back through the
    oracle's root frame, are the SAME TimeStep's fingertip_positions (within item 1's
    bound) -- which ties the extras to the observation's state across an auto-reset."""
    task, blob, recs = _parity_run(domain)
    om = oracle_mod.OracleModel(blob)
    nh = len(task.hand_names)
    hnq, nt = task.hand_nq // nh, task.ntips // nh
    tips = task_tip_sites(task)
    worst = 0.0
    for rec in recs:
        obs = rec["ts"].observation
        sv = rec["site_vel"].reshape(len(rec["qpos"]), -1, 6)
        for h, (hand, root) in enumerate(zip(task.hand_names, root_bodies(task))):
            np.testing.assert_array_equal(obs[f"{hand}/joint_positions"],
                                          rec["qpos"][:, h * hnq:(h + 1) * hnq].astype(np.float64))
            np.testing.assert_array_equal(
                obs[f"{hand}/fingertip_angular_velocities"],
                sv[:, tips[h * nt:(h + 1) * nt], 3:6].reshape(len(sv), -1).astype(np.float64))
            for e in range(len(sv)):
                d = oracle_mod.OracleData(om)
                d.qpos[:], d.qvel[:] = rec["qpos"][e], rec["qvel"][e]
                d.observe()
                xipos, ximat = root_frame(d, task.compiled, root)
                ego = obs[f"{hand}/fingertip_positions_ego"][e].reshape(-1, 3)
                back = (xipos + ego @ ximat.T).ravel()
                worst = max(worst, rel_err(back, obs[f"{hand}/fingertip_positions"][e]))
    print(domain, f"ego -> world vs fingertip_positions: {worst:.2e}")
    assert worst <= BOUND


def _widths(task):
    nh = len(task.hand_names)
    hnq, nt = task.hand_nq // nh, task.ntips // nh
    return dict(zip(NAMES, (hnq, 4 * nt, 3 * nt, 3 * nt)))


def _columns(task, names):
    """Columns of the all-on row that a row with `names` enabled holds."""
    w = _widths(task)
    cols, k = [], 0
    for _ in task.hand_names:
        for n in NAMES:
            if n in names:
                cols += range(k, k + w[n])
            k += w[n]
    return cols


@pytest.mark.parametrize("domain", ["bimanual", "reach"])
@pytest.mark.parametrize("strip", [True, False])
def test_subsets_and_layout(built, domain, strip):
    """Item 3: for each single observable and for joint_positions + angular velocities
    (mask 5) the row width, the row against the matching columns of the all-on row (bit
    for bit, same state), and the spec's and TimeStep's keys and shapes -- also with the
    singleton buffer dimension kept."""
    L = _lib.load()
    env = _load(domain, 4, strip_singleton_obs_buffer_dim=strip)
    base_keys = list(env._layout)
    env.reset()
    for i in range(3):
        _step_dev(env, i)
    full = env.hand_obs()
    w = _widths(env.task)
    hands = env.task.hand_names
    assert full.shape[1] == len(hands) * sum(w.values()) == L.dx_env_hand_obs_dim(env.ptr)
    lead = () if strip else (1,)
    for names in [(n,) for n in NAMES] + [("fingertip_angular_velocities", "joint_positions")]:
        env.enable_observables(names)
        ordered = [n for n in NAMES if n in names]
        dim = len(hands) * sum(w[n] for n in ordered)
        assert L.dx_env_hand_obs_dim(env.ptr) == dim == env.hand_obs_dim
        assert env.hand_observables == tuple(ordered)
        np.testing.assert_array_equal(env.hand_obs(), full[:, _columns(env.task, names)])
        keys = [f"{h}/{n}" for h in hands for n in ordered]
        spec = env.observation_spec()
        ts = env.timestep()
        assert list(spec) == base_keys + keys == list(ts.observation)
        for k in keys:
            n = k.split("/")[1]
            assert spec[k].shape == lead + (w[n],) and spec[k].dtype == np.float64
            assert ts.observation[k].shape == (4,) + lead + (w[n],)
    env.close()


def _packed_step(env, i):
    """A host-action step: the actions sample_actions(i) draws, through step(np_action)."""
    from dexterity_amd.manipulation import _copy_d2h

    ptr = env.sample_actions(i)
    env.physics.sync()
    a = np.empty((env.num_envs, env.model.nu), np.float32)
    _copy_d2h(a, ptr)
    ts = env.step(a)
    return ts, env._pin_out.copy()


def test_off_is_unchanged(built):
    """Item 4: an env that had the observables on (from before the reset, or switched on
    mid-episode) and then off steps exactly as one never configured: DX_OUT_OBS, reward,
    discount, step type and the packed rows over 6 steps, bit for bit, the spec keys
    today's, and DX_OUT_HAND_OBS refused while off."""
    L = _lib.load()
    kw = dict(seed=31, time_limit=0.08)
    plain = _load("reorient", 6, observables=None, **kw)
    before = _load("reorient", 6, **kw)
    mid = _load("reorient", 6, observables=None, **kw)
    envs = (plain, before, mid)
    keys = list(plain.observation_spec())
    for env in envs:
        env.reset()
        for i in range(2):
            _step_dev(env, i)
    mid.enable_observables(NAMES)
    assert list(mid.observation_spec()) == keys + [f"shadow_hand_e/{n}" for n in NAMES]
    for env in (before, mid):
        env.enable_observables([])
        assert env.hand_obs_dim == 0 == L.dx_env_hand_obs_dim(env.ptr) and env.hand_observables == ()
        p = ctypes.c_void_p()
        assert L.dx_env_output(env.ptr, _lib.OUT_HAND_OBS, ctypes.byref(p)) == -1
        assert b"hand observables" in L.dx_last_error()
        with pytest.raises(_lib.DxError):
            env.hand_obs()
        assert list(env.observation_spec()) == keys
    ended = False
    for i in range(2, 8):
        outs = []
        for env in envs:
            if i % 2:
                ts, packed = _packed_step(env, i)
            else:
                _step_dev(env, i)
                ts, packed = env.timestep(), None
            assert list(ts.observation) == keys
            outs.append((np.concatenate([ts.observation[k] for k in keys], axis=1), ts.reward, ts.discount,
                         ts.step_type, packed, env.physics.get(_lib.TIME)))
        ended = ended or (outs[0][3] == LAST).any()
        for other in outs[1:]:
            for x, y in zip(outs[0], other):
                if x is not None:
                    np.testing.assert_array_equal(x, y)
    assert ended
    for env in envs:
        env.close()


def test_enable_mid_episode(built):
    """Item 5: switching the observables on after three steps gives, from that call on,
    the rows of an env that had them on before its reset, bit for bit."""
    kw = dict(seed=17, time_limit=0.08)
    a = _load("reorient", 6, **kw)
    b = _load("reorient", 6, observables=None, **kw)
    for env in (a, b):
        env.reset()
        for i in range(3):
            _step_dev(env, i)
    b.enable_observables(NAMES)
    np.testing.assert_array_equal(b.hand_obs(), a.hand_obs())
    assert np.abs(a.hand_obs()).max() > 0.1
    for i in range(3, 8):
        for env in (a, b):
            _step_dev(env, i)
        np.testing.assert_array_equal(b.hand_obs(), a.hand_obs())
        np.testing.assert_array_equal(b.timestep().observation["shadow_hand_e/fingertip_orientations"],
                                      a.timestep().observation["shadow_hand_e/fingertip_orientations"])
    a.close()
    b.close()


def _run_rows(env, how, steps=6):
    env.reset()
    rows, types = [env.hand_obs()], []
    for i in range(steps):
        if how == "device":
            _step_dev(env, i)
        elif how == "random":
            env.step_random(i)
        else:
            ts, _ = _packed_step(env, i)
            # the host call's own TimeStep carries the same rows
            got = np.concatenate([ts.observation[k] for k in env._hand_layout], axis=1)
            np.testing.assert_array_equal(got, env.hand_obs().astype(np.float64))
        rows.append(env.hand_obs())
        types.append(env.timestep().step_type)
    env.close()
    return rows, np.array(types)


PATH_KW = dict(seed=23, time_limit=0.05)


@functools.lru_cache(maxsize=None)
def _default_rows():
    return _run_rows(_load("reorient", 6, **PATH_KW), "device")


@pytest.mark.parametrize("path", ["DX_NO_FUSE", "DX_DEFER_AT", "random", "host"])
def test_paths_agree(built, monkeypatch, path):
    """Item 6: the task kernels around the step kernel (DX_NO_FUSE=1), every step with more
    than one contact sent to the mid tier (DX_DEFER_AT=1), dx_env_step_random and the host
    call shape each give the default run's rows on the same seed, bit for bit."""
    ref, types = _default_rows()  # (run, the first time, before the variable is set)
    assert (types == LAST).any() and (types == FIRST).any()
    if path.startswith("DX_"):
        monkeypatch.setenv(path, "1")
    got, _ = _run_rows(_load("reorient", 6, **PATH_KW), path if not path.startswith("DX_") else "device")
    assert len(got) == len(ref) == 7
    for x, y in zip(got, ref):
        np.testing.assert_array_equal(x, y)


def test_shard_and_checkpoint(built, tmp_path):
    """Item 7: a shard with env_offset B gives rows B .. 2B - 1 of a 2B batch; a checkpoint
    saved after three steps and loaded into a fresh env with the same observables on
    holds the saved rows and continues as the uninterrupted run, bit for bit."""
    B = 4
    kw = dict(seed=41, time_limit=0.08)
    full = _load("bimanual", 2 * B, **kw)
    part = _load("bimanual", B, env_offset=B, **kw)
    for env in (full, part):
        env.reset()
    for i in range(3):
        for env in (full, part):
            env.step_random(i)
        np.testing.assert_array_equal(part.hand_obs(), full.hand_obs()[B:])
    path = str(tmp_path / "ckpt.npz")
    full.save(path)
    fresh = _load("bimanual", 2 * B, **kw)
    fresh.load(path)
    np.testing.assert_array_equal(fresh.hand_obs(), full.hand_obs())
    off = _load("bimanual", 2 * B, observables=None, **kw)
    with pytest.raises(ValueError, match="hand observables"):
        off.load(path)
    for i in range(3, 6):
        for env in (full, fresh):
            env.step_random(i)
        np.testing.assert_array_equal(fresh.hand_obs(), full.hand_obs())
    for env in (full, part, fresh, off):
        env.close()


def test_rejections(built):
    """Item 8: an unknown bit, an unknown name, a root body outside the model and a wrong
    hand count are refused with DX_EINVAL / ValueError and a reason, and leave the
    configuration -- and the rows -- as they were."""
    L = _lib.load()
    env = _load("bimanual", 4, observables=("joint_positions", "fingertip_positions_ego"))
    env.reset()
    env.step_random(0)
    rows, dim = env.hand_obs(), env.hand_obs_dim
    roots = root_bodies(env.task)
    nbody = len(env.task.compiled.names["body"])

    def rc(mask, nhands, r0, r1):
        cfg = _lib.HandObs(mask=mask, nhands=nhands)
        cfg.root_body[0], cfg.root_body[1] = r0, r1
        return L.dx_env_set_hand_observables(env.ptr, ctypes.byref(cfg))

    for args, why in (((16, 2, *roots), b"unknown bit"), ((31, 2, *roots), b"unknown bit"),
                      ((15, 2, roots[0], nbody), b"root body"), ((15, 2, -1, roots[1]), b"root body"),
                      ((15, 1, *roots), b"hand count"), ((15, 3, *roots), b"hand count")):
        assert rc(*args) == -1, args
        assert why in L.dx_last_error(), (args, L.dx_last_error())
        assert L.dx_env_hand_obs_dim(env.ptr) == dim
    with pytest.raises(ValueError, match="unknown hand observables"):
        env.enable_observables(["joint_positions", "joint_torques"])
    assert env.hand_observables == ("joint_positions", "fingertip_positions_ego") and env.hand_obs_dim == dim
    np.testing.assert_array_equal(env.hand_obs(), rows)
    env.step_random(1)
    assert env.hand_obs().shape == rows.shape and not np.array_equal(env.hand_obs(), rows)
    assert rc(15, 2, *roots) == 0 and L.dx_env_set_hand_observables(env.ptr, None) == 0
    assert L.dx_env_hand_obs_dim(env.ptr) == 0
    env.close()
