"""The observation pipeline on the device (include/dx.h dx_env_set_obs_pipeline): composer's
buffer, delay, aggregator and Gaussian corruptor behind every control step, compared with
the two host restatements of tests/obs_pipeline_ref.py over the env's own recorded rows.

A handful of envs, at most 30 control steps.  Episode ends are made by construction: a time
limit of ten control steps ends every env at once, and a NaN written into one env's qvel (the
divergence path of tests/test_gpu_health.py) ends that env alone, so the envs' episode clocks
differ -- every run asserts that two envs returned FIRST at different steps."""

import ctypes

import numpy as np
import pytest

from dexterity_amd import _lib
from tests import obs_pipeline_ref as ref

pytestmark = pytest.mark.gpu

FIRST, LAST = 0, 2
HAND_ALL = ("joint_positions", "fingertip_orientations", "fingertip_angular_velocities", "fingertip_positions_ego")
# task -> (load arguments, n_sub_steps, obs_dim, a time limit of ten control steps)
TASKS = {"reorient": (("reorient", "state_dense"), 5, 123, 0.25), "adroit_reach": (("reach", "state_dense"), 1, 117, 0.2),
         "handover": (("bimanual", "state_dense"), 5, 221, 0.25)}


@pytest.fixture(scope="module")
def built():
    from dexterity_amd import build

    build.build()


def _load(n, task="reorient", seed=5, **kw):
    from dexterity_amd import manipulation

    name, nsub, obs_dim, limit = TASKS[task]
    env = manipulation.load(*name, seed=seed, num_envs=n, time_limit=limit, **kw)
    assert env.task.config.n_sub_steps == nsub and env.obs_dim == obs_dim
    return env


def _configure(env, m, d, K, pad="zero", agg=None, **kw):
    """m and d in control steps (composer's options count physics steps)."""
    nsub = env.task.config.n_sub_steps
    env.configure_observations(update_interval=m * nsub, delay=d * nsub, buffer_size=K, padding=pad,
                               aggregator=agg, **kw)


def _step_type(env):
    return env._read(_lib.OUT_STEP_TYPE, np.int32, 1)[:, 0]


def _row(env):
    """The pipeline's input row of every env: DX_OUT_OBS || DX_OUT_HAND_OBS."""
    obs = env._read(_lib.OUT_OBS, np.float32, env.obs_dim)
    return np.concatenate([obs, env.hand_obs()], axis=1) if env.hand_obs_dim else obs


def _inject_nan(env, e):
    qvel = env.physics.get(_lib.QVEL)
    qvel[e, 0] = np.nan
    env.physics.set(_lib.QVEL, qvel)


class Record:
    def __init__(self):
        self.rows, self.st, self.buf = [], [], []

    def take(self, env):
        self.rows.append(_row(env))
        self.st.append(_step_type(env))
        self.buf.append(env.obs_buffer())

    def env(self, e):
        return np.stack([r[e] for r in self.rows]), [int(s[e]) for s in self.st], np.stack([b[e] for b in self.buf])

    def desynchronised(self):
        """Two envs returned FIRST at different steps."""
        st = np.stack(self.st)
        return len({tuple(np.nonzero(st[:, e] == FIRST)[0]) for e in range(st.shape[1])}) > 1


def _run(env, steps, nan=(3, 1), step=None, rec=None):
    """reset(), then `steps` control steps of the random agent's actions, a NaN into env
    nan[1]'s qvel ahead of step nan[0]; records the rows, step types and buffer after each."""
    rec = rec or Record()
    step = step or (lambda k: env.step(env.sample_actions(k), device_action=True))
    env.reset()
    rec.take(env)
    for k in range(steps):
        if nan and k == nan[0]:
            _inject_nan(env, nan[1])
        step(k)
        rec.take(env)
    return rec


def _bits(a, signed_zero=True):
    """The values' bit patterns.  signed_zero=False maps -0 to +0 first: among slots that
    hold zeros of both signs numpy's own min, max and median (a selection, not a stable
    sort) leave the sign of the zero they return open, so an aggregate is compared bit for
    bit up to that sign and everything else with it."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return (a if signed_zero else a + np.float32(0)).view(np.uint32)


def _expect(rec, e, env, m, d, K, pad, agg=None, corrupt=None, events=True):
    rows, st, got = rec.env(e)
    want = ref.closed_form(rows, st, m, d, K, pad, agg, corrupt)
    if events and corrupt is None:  # (a corruptor's stream can be replayed once)
        nsub = env.task.config.n_sub_steps
        sim = ref.simulate_events(rows, st, nsub, m * nsub, d * nsub, K, pad, agg)
        assert np.array_equal(_bits(sim, agg is None), _bits(want, agg is None))
    return got, want.reshape(got.shape)


CONFIGS = [(1, 0, 1, "zero"), (1, 2, 3, "zero"), (2, 3, 4, "initial_value"), (3, 0, 2, "zero")]


@pytest.mark.parametrize("task, n", [("reorient", 4), ("adroit_reach", 3)])
def test_history_is_exact(built, task, n):
    """DX_OUT_OBS_BUFFER equals both restatements of the env's own recorded rows, bit for bit."""
    env = _load(n, task)
    for m, d, K, pad in CONFIGS:
        _configure(env, m, d, K, pad)
        rec = Record()
        rec.take(env)  # the read the setter left: n = 0 at the env's current row
        _run(env, 26, rec=rec)
        assert rec.desynchronised()
        for e in range(n):
            got, want = _expect(rec, e, env, m, d, K, pad)
            assert got.shape == (28, K, env.obs_dim)
            assert np.array_equal(_bits(got), _bits(want)), (m, d, K, pad, e)
            if (m, d, K) == (1, 0, 1):  # the launch alone: the raw row
                assert np.array_equal(_bits(got[:, 0]), _bits(rec.env(e)[0]))
    env.close()


def test_with_hand_observables(built):
    """With all four hand observables on the row is obs || hand row."""
    n = 4
    env = _load(n)
    env.enable_observables(HAND_ALL)
    W = env.obs_dim + env.hand_obs_dim
    assert env.hand_obs_dim == 74 and W == 197
    for m, d, K, pad in [(1, 2, 3, "zero"), (2, 3, 4, "initial_value")]:
        _configure(env, m, d, K, pad)
        rec = Record()
        rec.take(env)
        _run(env, 16, rec=rec)
        assert rec.desynchronised()
        for e in range(n):
            got, want = _expect(rec, e, env, m, d, K, pad)
            assert got.shape == (18, K, W) and np.array_equal(_bits(got), _bits(want))
        ts = env.timestep()
        buf = env.obs_buffer()
        assert np.array_equal(ts.observation["shadow_hand_e/fingertip_positions_ego"],
                              buf[:, :, W - 15:].astype(np.float64))
    env.close()


def test_widest_row(built):
    """The two-hand handover with all four hand observables, the widest shipped row (369
    floats: more than one pass of a wave over a row's 16-B groups, six chunks of noise
    draws): the history bit for bit, an aggregate, and the noise replayed from numpy."""
    n, seed = 3, 21
    env = _load(n, "handover")
    env.enable_observables(HAND_ALL)
    W = env.obs_dim + env.hand_obs_dim
    assert W == 369
    for m, d, K, pad, agg in [(2, 1, 3, "initial_value", None), (1, 1, 4, "zero", "median")]:
        _configure(env, m, d, K, pad, agg)
        rec = Record()
        rec.take(env)
        _run(env, 13, rec=rec)
        assert rec.desynchronised()
        for e in range(n):
            got, want = _expect(rec, e, env, m, d, K, pad, agg)
            assert got.shape == (15, 1 if agg else K, W)
            assert np.array_equal(_bits(got, agg is None), _bits(want, agg is None)), (m, d, K, e)
    sigma = _sigma(W)
    _configure(env, 2, 1, 3, "zero", noise_std=sigma, noise_seed=seed)
    rec = Record()
    rec.take(env)
    _run(env, 13, rec=rec)
    for e in range(n):
        rs = np.random.RandomState(seed + e)
        got, want = _expect(rec, e, env, 2, 1, 3, "zero", None, ref.gaussian_corruptor(rs, sigma))
        np.testing.assert_array_max_ulp(got, want, maxulp=1)
    env.close()


def test_every_aggregator(built):
    """min, max, mean, median and sum over K = 4 and K = 3 delivered slots (the median of an
    even and of an odd K), padding included, bit-equal to the fp64 definitions."""
    n = 3
    env = _load(n)
    for K in (4, 3):
        for agg in ref.AGGREGATORS[1:]:
            _configure(env, 1, 1, K, "zero", agg)
            rec = Record()
            rec.take(env)
            _run(env, 13, rec=rec)
            assert rec.desynchronised()
            for e in range(n):
                got, want = _expect(rec, e, env, 1, 1, K, "zero", agg)
                assert got.shape == (15, 1, env.obs_dim)
                assert np.array_equal(_bits(got, False), _bits(want, False)), (K, agg, e)
    env.close()


def _sigma(W):
    s = np.zeros(W)
    s[1::3] = 0.01
    s[2::7] = 1.5
    s[W - 1] = 0.25
    assert np.count_nonzero(s == 0) > W // 3 and np.count_nonzero(s) > W // 3
    return s


def test_noise_replays_numpy(built):
    """The delivered values are within one fp32 ulp of RandomState(seed + e) replayed in the
    stated order (the action-noise replay's bound: a last-bit difference of log), over samples
    every second step and resets; afterwards the stream is where numpy's is (within 4 fp64
    ulps: W draws per sample, the cached gaussian kept, nothing drawn without a sample)."""
    n, seed, m, d, K = 4, 77, 2, 1, 3
    env = _load(n)
    W = env.obs_dim
    sigma = _sigma(W)
    _configure(env, m, d, K, "initial_value", noise_std=sigma, noise_seed=seed)
    rec = Record()
    rec.take(env)
    _run(env, 20, rec=rec)
    assert rec.desynchronised()
    rs = [np.random.RandomState(seed + e) for e in range(n)]
    for e in range(n):
        got, want = _expect(rec, e, env, m, d, K, "initial_value", None, ref.gaussian_corruptor(rs[e], sigma))
        np.testing.assert_array_max_ulp(got, want, maxulp=1)
        # the newest slot at n = d is s_0 = the FIRST row (entry 1) with the noise on it
        clean = rec.rows[1][e]
        assert np.array_equal(got[1 + d, K - 1, sigma == 0], clean[sigma == 0])
        assert np.mean(got[1 + d, K - 1, sigma > 0] != clean[sigma > 0]) > 0.9
    L = _lib.load()
    for cnt in (3, 64, 2):
        out = np.full((n, cnt), np.nan)
        _lib.check(L.dx_env_obs_noise_draw(env.ptr, cnt, out.ctypes.data))
        np.testing.assert_array_max_ulp(out, np.stack([r.standard_normal(cnt) for r in rs]), maxulp=4)
    assert L.dx_env_obs_noise_draw(env.ptr, 65, out.ctypes.data) == -1
    env.close()


def _outputs(env):
    return (env._read(_lib.OUT_OBS, np.float32, env.obs_dim), env._read(_lib.OUT_REWARD, np.float32, 1),
            env._read(_lib.OUT_DISCOUNT, np.float32, 1), _step_type(env), env.physics.get(_lib.QPOS))


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_off_is_unchanged_and_no_feedback(built):
    n = 4
    plain, piped = _load(n), _load(n)
    L = _lib.load()
    size0 = _lib.check(L.dx_env_save(plain.ptr, None, 0))
    nfield0 = len(plain._state_fields())
    _configure(piped, 1, 2, 3, "zero", noise_std=0.3)
    assert _lib.check(L.dx_env_save(piped.ptr, None, 0)) > size0
    firsts = []
    for env in (plain, piped):
        env.reset()
    for k in range(14):
        for env in (plain, piped):
            if k == 3:
                _inject_nan(env, 1)
            env.step(env.sample_actions(k), device_action=True)
        a, b = _outputs(plain), _outputs(piped)
        assert _same(a, b)  # the pipeline never feeds back
        firsts.append(a[3] == FIRST)
        if k == 7:  # off: every output and the checkpoint are those of an env never configured
            piped.configure_observations()
            assert piped.observation_config is None
            assert _lib.check(L.dx_env_save(piped.ptr, None, 0)) == size0
            assert len(piped._state_fields()) == nfield0
            with pytest.raises(_lib.DxError):
                piped.obs_buffer_ptr()
    firsts = np.stack(firsts)
    assert len({tuple(np.nonzero(firsts[:, e])[0]) for e in range(n)}) > 1
    ta, tb = plain.timestep(), piped.timestep()
    assert list(ta.observation) == list(tb.observation)
    assert all(np.array_equal(ta.observation[k], tb.observation[k]) for k in ta.observation)
    plain.close()
    piped.close()


def test_enabling_mid_episode_restarts_history(built):
    n, m, d, K = 4, 1, 1, 3
    env = _load(n)
    env.reset()
    for k in range(5):
        if k == 2:
            _inject_nan(env, 2)
        env.step(env.sample_actions(k), device_action=True)
    _configure(env, m, d, K, "initial_value")
    row = _row(env)
    buf = env.obs_buffer()
    assert np.array_equal(_bits(buf), _bits(np.repeat(row[:, None], K, axis=1)))  # s_0 = the current row
    _configure(env, m, 0, K, "zero")  # reconfiguring restarts as well
    buf = env.obs_buffer()
    assert not buf[:, :2].any() and np.array_equal(_bits(buf[:, 2]), _bits(row))
    rec = Record()
    rec.take(env)
    for k in range(5, 14):
        env.step(env.sample_actions(k), device_action=True)
        rec.take(env)
    st = np.stack(rec.st)
    assert len({tuple(np.nonzero(st[:, e] == FIRST)[0]) for e in range(n)}) > 1
    for e in range(n):
        got, want = _expect(rec, e, env, m, 0, K, "zero")
        assert np.array_equal(_bits(got), _bits(want))
    env.close()


def test_checkpoint(built, tmp_path):
    """Saved after 7 steps -- the history partly filled, noise on, an odd number of gaussians
    drawn -- and loaded into a fresh env configured the same way: the next 8 steps are
    bit-equal to the uninterrupted run."""
    n = 4
    kw = dict(noise_std=0.05, noise_seed=3)

    def make():
        env = _load(n)
        _configure(env, 2, 3, 4, "initial_value", **kw)
        return env

    env = make()
    env.reset()
    for k in range(7):
        if k == 3:
            _inject_nan(env, 1)
        env.step(env.sample_actions(k), device_action=True)
    path = str(tmp_path / "ckpt.npz")
    env.save(path)
    with np.load(path) as z:
        assert {"obs_ring", "obs_count", "mt_obs_noise", "obs_buffer"} <= set(z.files)
        assert z["obs_count"].dtype == np.int32 and len(set(z["obs_count"][:, 0])) > 1  # the clocks differ
        assert z["obs_count"].max() == 7 and z["obs_ring"].shape == (n, 6 * 128)  # S = 4 + ceil(3 / 2), Wp = 128
        # samples: the setter's, FIRST's, n = 2, 4, 6 (env 1: its own clock) -- 123 draws each
        assert np.all(z["mt_obs_noise"][[0, 2, 3], 625] == 1)
    want, first = [], []
    for k in range(7, 15):
        env.step(env.sample_actions(k), device_action=True)
        want.append(env.obs_buffer())
        first.append(_step_type(env) == FIRST)
    env.close()
    assert np.stack(first).any()
    other = make()
    other.load(path)
    assert np.array_equal(_bits(other.obs_buffer()), _bits(np.load(path)["obs_buffer"].reshape(n, 4, 123)))
    for k in range(7, 15):
        other.step(other.sample_actions(k), device_action=True)
        assert np.array_equal(_bits(other.obs_buffer()), _bits(want[k - 7])), k
    # a checkpoint of the pipeline does not load into an env without it, nor the reverse
    other.configure_observations()
    with pytest.raises(ValueError, match="observation pipeline"):
        other.load(path)
    other.close()


def test_shard_equals_unsharded_rows(built):
    B = 3
    whole, shard = _load(2 * B), _load(B, env_offset=B)
    recs = []
    for env, bad in ((whole, B + 1), (shard, 1)):
        _configure(env, 1, 1, 2, "zero", noise_std=0.1, noise_seed=11)
        rec = Record()
        rec.take(env)
        recs.append(_run(env, 12, nan=(3, bad), rec=rec))
    assert recs[1].desynchronised()
    for a, b in zip(recs[0].buf, recs[1].buf):
        assert np.array_equal(_bits(a[B:]), _bits(b))
    whole.close()
    shard.close()


def test_call_shapes_deliver_the_same_buffer(built, monkeypatch):
    """dx_env_step, dx_env_step_random, dx_env_step_host and the unfused launch sequence
    (DX_NO_FUSE=1) deliver the same buffer for the same actions."""
    from dexterity_amd.manipulation import _copy_d2h

    n, cfg = 4, (2, 1, 3, "initial_value")

    def host_step(env):
        def step(k):
            a = np.empty((n, env.model.nu), np.float32)
            ptr = env.sample_actions(k)
            env.physics.sync()
            _copy_d2h(a, ptr)
            ts = env.step(a)
            assert np.array_equal(ts.observation["goal_state"], env.obs_buffer()[:, :, -4:].astype(np.float64))
        return step

    runs = []
    for shape in ("device", "random", "host", "unfused"):
        if shape == "unfused":
            monkeypatch.setenv("DX_NO_FUSE", "1")
        env = _load(n)
        _configure(env, *cfg, noise_std=0.02)
        step = {"random": env.step_random, "host": host_step(env)}.get(shape)
        rec = _run(env, 12, step=step)
        assert rec.desynchronised()
        runs.append(np.stack(rec.buf))
        env.close()
    for r in runs[1:]:
        assert np.array_equal(_bits(r), _bits(runs[0]))


def test_rejections(built):
    n = 3
    env = _load(n)
    L = _lib.load()
    W = env.obs_dim
    ptr = ctypes.c_void_p()
    assert L.dx_env_output(env.ptr, _lib.OUT_OBS_BUFFER, ctypes.byref(ptr)) == -1  # off
    dims = (ctypes.c_int32 * 3)()
    _lib.check(L.dx_env_obs_pipe_dims(env.ptr, dims))
    assert list(dims) == [W, 0, 0]
    env.reset()
    _configure(env, 2, 1, 3, "zero", noise_std=0.1)
    env.step(env.sample_actions(0), device_action=True)
    before = env.obs_buffer()
    good = np.full(W, 0.5)

    def cfg(sigma=good, **kw):
        p = _lib.ObsPipeline(update_interval=1, delay=0, buffer_size=1, aggregator=0, padding=0, noise=0)
        for k, v in kw.items():
            setattr(p, k, v)
        if sigma is not None:
            p.noise_sigma, p.nsigma = sigma.ctypes.data, sigma.size
        return p

    bad_sigma = [good.copy() for _ in range(3)]
    bad_sigma[0][5], bad_sigma[1][W - 1], bad_sigma[2][0] = -1e-9, np.nan, np.inf
    einval = [cfg(update_interval=0), cfg(update_interval=65), cfg(delay=-1), cfg(delay=65), cfg(buffer_size=0),
              cfg(buffer_size=17), cfg(aggregator=-1), cfg(aggregator=6), cfg(padding=2), cfg(padding=-1),
              cfg(noise=2), cfg(noise=1, sigma=good[:-1].copy()), cfg(noise=1, sigma=None)]
    einval += [cfg(noise=1, sigma=s) for s in bad_sigma]
    for p in einval:
        assert L.dx_env_set_obs_pipeline(env.ptr, ctypes.byref(p)) == -1  # DX_EINVAL
        assert L.dx_last_error().startswith(b"observation pipeline")
        _lib.check(L.dx_env_obs_pipe_dims(env.ptr, dims))
        assert list(dims) == [W, 3, 1]  # the configuration ...
        assert np.array_equal(_bits(env.obs_buffer()), _bits(before))  # ... and the buffer survive
    # the hand observables set the row's width: refused while the pipeline is on
    with pytest.raises(_lib.DxError, match="observation pipeline"):
        env.enable_observables(["joint_positions"])
    env.step(env.sample_actions(1), device_action=True)
    assert env.obs_buffer().shape == (n, 3, W)
    # DX_ELIMIT guards more than 80 ring slots, S = K + ceil(d / m); the field ranges keep
    # S <= 16 + 64, so the largest option set is accepted and runs
    p = cfg(update_interval=1, delay=64, buffer_size=16)
    _lib.check(L.dx_env_set_obs_pipeline(env.ptr, ctypes.byref(p)))
    _lib.check(L.dx_env_obs_pipe_dims(env.ptr, dims))
    assert list(dims) == [W, 16, 1]
    env.step(env.sample_actions(2), device_action=True)
    assert not env._read(_lib.OUT_OBS_BUFFER, np.float32, 16 * W).any()  # 64 steps of delay, zero padding
    env.configure_observations()
    env.enable_observables(["joint_positions"])
    _lib.check(L.dx_env_obs_pipe_dims(env.ptr, dims))
    assert list(dims) == [W + 24, 0, 0]
    p = cfg(noise=1)  # a sigma of the old width
    assert L.dx_env_set_obs_pipeline(env.ptr, ctypes.byref(p)) == -1
    env.close()


def test_python_surface(built):
    n = 3
    for strip in (True, False):
        env = _load(n, strip_singleton_obs_buffer_dim=strip)
        env.enable_observables(["joint_positions"])
        keys = list(env.observation_spec())
        assert keys[-1] == "shadow_hand_e/joint_positions" and keys[0] == "shadow_hand_e/joint_positions_sin_cos"
        widths = {k: v.shape[-1] for k, v in env.observation_spec().items()}
        env.reset()

        def check(lead):
            spec = env.observation_spec()
            for ts in (env.timestep(), env.step(np.zeros((n, env.model.nu), np.float32))):
                assert list(ts.observation) == keys == list(spec)
                for k in keys:
                    assert ts.observation[k].shape == (n,) + lead + (widths[k],) == (n,) + spec[k].shape
                    assert ts.observation[k].dtype == np.float64

        check(() if strip else (1,))  # off
        _configure(env, 1, 1, 3)
        check((3,))
        before = env.physics.get(_lib.QPOS)[:, :24].astype(np.float64)
        ts = env.step(np.zeros((n, env.model.nu), np.float32))
        assert np.array_equal(ts.observation["shadow_hand_e/joint_positions"][:, 2], before)  # delayed by a step
        _configure(env, 1, 0, 3)
        env.step(np.zeros((n, env.model.nu), np.float32))
        ts = env.timestep()
        qpos = env.physics.get(_lib.QPOS)[:, :24].astype(np.float64)
        assert np.array_equal(ts.observation["shadow_hand_e/joint_positions"][:, 2], qpos)
        assert not ts.observation["goal_state"][:, 0].any()  # zero padding: the oldest slot
        _configure(env, 1, 0, 1)
        check(() if strip else (1,))
        _configure(env, 1, 0, 4, agg="mean")
        check(())
        assert env.obs_buffer_ptr() == env._out(_lib.OUT_OBS_BUFFER)
        env.configure_observations()
        check(() if strip else (1,))
        with pytest.raises(ValueError, match="not a multiple"):
            env.configure_observations(update_interval=7)
        env.close()
