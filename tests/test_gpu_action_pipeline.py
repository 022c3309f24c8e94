"""The action pipeline on the device (include/dx.h dx_env_set_action_filter): ActionNoise,
PreviousAction and SmoothAction of the reference ahead of every control step, replayed
from numpy.  Shadow reorient (nu = 20), a handful of envs, at most 40 control steps; a
time limit places the episode ends (0.25 s: the 10th control step returns LAST, the 11th
re-initialises and returns FIRST; 0.11 s: the 5th and the 6th)."""

import ctypes

import numpy as np
import pytest

from dexterity_amd import _lib

pytestmark = pytest.mark.gpu

NU = 20
LAST = 2


@pytest.fixture(scope="module")
def built():
    from dexterity_amd import build

    build.build()


def _load(n, time_limit=0.25, seed=5, **kw):
    from dexterity_amd import manipulation

    env = manipulation.load("reorient", "state_dense", seed=seed, num_envs=n, time_limit=time_limit, **kw)
    assert env.model.nu == NU
    return env


def _step_type(env):
    return env._read(_lib.OUT_STEP_TYPE, np.int32, 1)[:, 0]


def _obs(env):
    return env._read(_lib.OUT_OBS, np.float32, env.obs_dim)


def _ctrl(env):
    return env.physics.get(_lib.CTRL)


def _drive(env, actions, steps):
    """reset(), then `steps` host steps of actions(k); per step: whether the step
    re-initialised its env (the one before returned LAST: task_pre's test), the previous
    action and ctrl after it."""
    env.reset()
    st = _step_type(env)
    rec = []
    for k in range(steps):
        reinit = st == LAST
        env.step(actions(k))
        st = _step_type(env)
        rec.append((reinit, env.previous_action(), _ctrl(env), st.copy()))
    return rec


def _bounds(env):
    spec = env.action_spec()
    assert spec.minimum.dtype == np.float32 and np.all(np.isfinite(spec.maximum - spec.minimum))
    return spec.minimum, spec.maximum


def _noisy(rs, a_row, lo, hi, scale):
    """ActionNoise.step for one env (manipulation/wrappers/action_noise.py), as numpy
    computes it: the stddev from the float32 bounds, the sum and the clip in fp64."""
    std = scale * (hi - lo)
    return np.clip(a_row.astype(np.float64) + rs.normal(scale=std), lo, hi).astype(np.float32)


def _ema_replay(rec, alpha, commands):
    """The fp64 restatement of SmoothAction over a recorded run; commands(k) are the
    commands the smoother received at step k.  Returns the expected ctrl per step."""
    n = rec[0][1].shape[0]
    held = np.zeros((n, NU), np.float32)
    has = np.zeros(n, bool)
    out = []
    for k, (reinit, _, _, _) in enumerate(rec):
        x = commands(k)
        want = np.zeros((n, NU), np.float32)
        for e in range(n):
            if reinit[e]:  # initialize_episode: no value, and mj_resetData zeroes ctrl
                has[e] = False
                continue
            if not has[e]:
                held[e], has[e] = x[e], True
            else:
                held[e] = (alpha * held[e].astype(np.float64) + (1 - alpha) * x[e].astype(np.float64)).astype(np.float32)
            want[e] = held[e]
        out.append(want)
    return out


def test_noise_replays_numpy(built):
    """previous_action over 40 steps of fixed actions equals clip(a + RandomState(99 +
    e).normal(scale=0.05 * (hi - lo)), lo, hi) within one fp32 ulp (a last-bit difference of
    log); numpy draws on every step, the device row is zero on a re-initialising one."""
    n, steps, scale = 4, 40, 0.05
    # a gaussian pair takes at least 4 stream words: every env crosses its 624-word block
    # more than once
    assert (steps * NU // 2) * 4 >= 2 * 624
    env = _load(n, noise_scale=scale, noise_seed=99)
    lo, hi = _bounds(env)
    a = np.random.RandomState(0).uniform(lo, hi, size=(n, NU)).astype(np.float32)
    a[0], a[1] = hi, lo  # the clip engages on about half the draws
    rec = _drive(env, lambda k: a, steps)
    env.close()
    rs = [np.random.RandomState(99 + e) for e in range(n)]
    reinits = clipped = 0
    for k, (reinit, prev, _, _) in enumerate(rec):
        for e in range(n):
            want = _noisy(rs[e], a[e], lo, hi, scale)
            clipped += int(np.sum((want == lo) | (want == hi)))
            if reinit[e]:
                want = np.zeros(NU, np.float32)
                reinits += 1
            np.testing.assert_array_max_ulp(prev[e], want, maxulp=1)
    assert reinits >= n  # every env was re-initialised at least once in the window
    assert clipped >= steps * NU // 2


def test_noise_stream_alignment(built):
    """Successive dx_env_action_noise_draw calls equal successive standard_normal calls of
    RandomState(seed + e), within 4 fp64 ulps (sqrt and the division are correctly rounded,
    OCML's log is within 1 ulp: f * x stays under 3); odd counts leave numpy's cached
    second gaussian for the next call."""
    n = 3
    env = _load(n, noise_scale=0.05, noise_seed=1234)
    L = _lib.load()
    rs = [np.random.RandomState(1234 + e) for e in range(n)]
    for cnt in (1, 3, 64, 2, 5):
        out = np.full((n, cnt), np.nan)
        _lib.check(L.dx_env_action_noise_draw(env.ptr, cnt, out.ctypes.data))
        want = np.stack([r.standard_normal(cnt) for r in rs])
        np.testing.assert_array_max_ulp(out, want, maxulp=4)
    assert L.dx_env_action_noise_draw(env.ptr, 65, out.ctypes.data) == -1
    env.close()


@pytest.mark.parametrize("alpha", [0.7, 0.0, 1.0])
def test_ema_is_exact(built, alpha):
    """DX_CTRL after every step is the fp64 restatement of the moving average, bit for
    bit: the command itself on an episode's first step, 0 on the re-initialising step;
    alpha = 0 passes the action, alpha = 1 holds the episode's first command."""
    n, steps = 3, 12
    env = _load(n, time_limit=0.11, smooth_alpha=alpha)
    lo, hi = _bounds(env)
    acts = np.random.RandomState(1).uniform(lo, hi, size=(steps, n, NU)).astype(np.float32)
    rec = _drive(env, lambda k: acts[k], steps)
    env.close()
    want = _ema_replay(rec, alpha, lambda k: acts[k])
    first = np.zeros((n, NU), np.float32)  # per env: the episode's first command
    fresh = np.ones(n, bool)               # the env's next command is its episode's first
    for k, (reinit, prev, ctrl, _) in enumerate(rec):
        np.testing.assert_array_equal(ctrl, want[k])
        np.testing.assert_array_equal(prev, np.where(reinit[:, None], np.float32(0), acts[k]))
        for e in range(n):
            if reinit[e]:
                assert not ctrl[e].any()
                fresh[e] = True
                continue
            if fresh[e]:
                np.testing.assert_array_equal(ctrl[e], acts[k, e])  # an episode's first command passes
                first[e], fresh[e] = acts[k, e], False
            if alpha == 0.0:
                np.testing.assert_array_equal(ctrl[e], acts[k, e])
            elif alpha == 1.0:
                np.testing.assert_array_equal(ctrl[e], first[e])
    # the time limit re-initialises every env in the middle of the run
    assert 0 < next(k for k, r in enumerate(rec) if r[0].all()) < steps - 2


def test_order_noise_then_previous_then_ema(built):
    """Both stages on: previous_action is the noisy command (numpy's, within an ulp) and
    ctrl the moving average of exactly those commands.  Six envs: two workgroups of the
    filter, the second half full."""
    n, steps, scale, alpha = 6, 20, 0.05, 0.7
    env = _load(n, noise_scale=scale, noise_seed=99, smooth_alpha=alpha)
    lo, hi = _bounds(env)
    acts = np.random.RandomState(2).uniform(lo, hi, size=(steps, n, NU)).astype(np.float32)
    rec = _drive(env, lambda k: acts[k], steps)
    env.close()
    rs = [np.random.RandomState(99 + e) for e in range(n)]
    for k, (reinit, prev, _, _) in enumerate(rec):
        for e in range(n):
            want = _noisy(rs[e], acts[k, e], lo, hi, scale)
            np.testing.assert_array_max_ulp(prev[e], np.zeros(NU, np.float32) if reinit[e] else want, maxulp=1)
    assert any(r[0].any() for r in rec)
    want = _ema_replay(rec, alpha, lambda k: rec[k][1])
    for k, (_, _, ctrl, _) in enumerate(rec):
        np.testing.assert_array_equal(ctrl, want[k])
    assert not np.array_equal(rec[3][1], rec[3][2])  # smoothed: ctrl is no longer the command


def test_off_is_unchanged(built):
    """An env whose pipeline was on for three steps, then switched off and reset, runs as
    one never configured: 10 random-agent steps give bit-equal observations, rewards, step
    types, qpos and ctrl, and the checkpoint has the same size.  (No falls, no successes:
    both envs make the same reset draws whatever their first three steps did.)"""
    from dexterity_amd import manipulation

    n = 8
    L = _lib.load()
    cfg = manipulation.ReOrientConfig(fall_termination=False, orientation_threshold=0.0)
    outs, sizes = [], []
    for configured in (False, True):
        env = manipulation.GoalEnvironment(manipulation.ReOrient(cfg), num_envs=n, seed=7, time_limit=0.11)
        plain = _lib.check(L.dx_env_save(env.ptr, None, 0))
        if configured:
            env.configure_actions(noise_scale=0.05, smooth_alpha=0.5, previous_action=True)
            # the pipeline's state travels with the checkpoint only while it is on
            assert _lib.check(L.dx_env_save(env.ptr, None, 0)) == plain + n * (2 * NU * 4 + 4 + 628 * 4)
        env.reset()
        for i in range(3):
            env.step_random(i)
        if configured:
            assert env.previous_action().any()
            env.configure_actions()
        env.reset()
        rec = []
        for i in range(10):
            env.step_random(100 + i)
            ts = env.timestep()
            rec.append((_obs(env), ts.reward, ts.step_type, env.physics.qpos, _ctrl(env)))
        assert any((r[2] == LAST).any() for r in rec)
        sizes.append(_lib.check(L.dx_env_save(env.ptr, None, 0)))
        outs.append(rec)
        env.close()
    assert sizes[0] == sizes[1]
    for ra, rb in zip(*outs):
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)


def _draw(env, cnt=5):
    out = np.empty((env.num_envs, cnt))
    _lib.check(_lib.load().dx_env_action_noise_draw(env.ptr, cnt, out.ctypes.data))
    return out


def test_checkpoint_resume(built, tmp_path):
    """Noise and smoothing on: a run saved after 8 steps and resumed in a fresh env
    configured the same way equals the uninterrupted run after 8 more -- observations,
    ctrl, previous action and the noise stream's next draws, bit for bit."""
    n = 5
    kw = dict(noise_scale=0.05, noise_seed=21, smooth_alpha=0.7)

    def run(env, steps):
        for i in steps:
            env.step_random(i)

    a = _load(n, time_limit=0.3, seed=21, **kw)
    a.reset()
    run(a, range(8))
    path = str(tmp_path / "ckpt.npz")
    a.save(path)
    with np.load(path) as z:
        assert {"act_ema", "act_ema_set", "prev_action", "mt_noise"} <= set(z.files)
        assert z["act_ema_set"].dtype == np.int32 and z["mt_noise"].shape == (n, 628)
    run(a, range(8, 16))
    ref = (_obs(a), _ctrl(a), a.previous_action(), _step_type(a), _draw(a))
    a.close()
    b = _load(n, time_limit=0.3, seed=77)
    b.reset()
    with pytest.raises(ValueError, match="action pipeline"):  # the settings are not in the checkpoint
        b.load(path)
    b.configure_actions(**kw)
    b.load(path)
    run(b, range(8, 16))
    got = (_obs(b), _ctrl(b), b.previous_action(), _step_type(b), _draw(b))
    b.close()
    for x, y in zip(ref, got):
        np.testing.assert_array_equal(x, y)
    assert ref[2].any()


def test_shard_equals_rows_of_the_batch(built):
    """A shard of 2 envs at env_offset 2 draws its noise as envs 2..3 of a batch of 4."""
    kw = dict(noise_scale=0.05, noise_seed=3, smooth_alpha=0.7)
    full = _load(4, **kw)
    part = _load(2, env_offset=2, **kw)
    full.reset()
    part.reset()
    for i in range(5):
        full.step_random(i)
        part.step_random(i)
        np.testing.assert_array_equal(part.previous_action(), full.previous_action()[2:])
        np.testing.assert_array_equal(_ctrl(part), _ctrl(full)[2:])
    assert part.previous_action().any()
    full.close()
    part.close()


def test_unfused_path(built, monkeypatch):
    """DX_NO_FUSE=1 (the task kernels around the step kernel) reads the same filtered
    buffer: observations, ctrl and previous action over 6 steps, bit for bit, with a
    re-initialising step among them."""
    outs = []
    for variant in ("kernels", "fused"):
        if variant == "kernels":
            monkeypatch.setenv("DX_NO_FUSE", "1")
        else:
            monkeypatch.delenv("DX_NO_FUSE", raising=False)
        env = _load(4, time_limit=0.11, noise_scale=0.05, noise_seed=8, smooth_alpha=0.7)
        env.reset()
        rec = []
        for i in range(6):
            env.step_random(i)
            rec.append((_obs(env), _ctrl(env), env.previous_action(), _step_type(env)))
        outs.append(rec)
        env.close()
    assert (outs[0][4][3] == LAST).all() and not outs[0][5][2].any()
    for ra, rb in zip(*outs):
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)


def test_call_shapes_agree(built):
    """step(host array), step(ptr, device_action=True) and step_random(k) go through the
    same filter: bit-equal observations, ctrl and previous actions; the caller's device
    buffer (here the library's action buffer, and a buffer of the caller's own) is not
    written."""
    from dexterity_amd.manipulation import _copy_d2h, _copy_h2d, _hip_runtime

    n, steps = 4, 4
    kw = dict(noise_scale=0.05, noise_seed=11, smooth_alpha=0.7)
    envs = [_load(n, **kw) for _ in range(4)]
    for env in envs:
        env.reset()
    own = ctypes.c_void_p()
    assert _hip_runtime().hipMalloc(ctypes.byref(own), n * NU * 4) == 0
    for k in range(steps):
        envs[0].step_random(k)
        ptr = envs[1].sample_actions(k)
        envs[1].physics.sync()
        a = np.empty((n, NU), np.float32)
        _copy_d2h(a, ptr)
        envs[1].step(ptr, device_action=True)
        envs[2].step(a)
        _copy_h2d(own.value, a)
        envs[3].step(own.value, device_action=True)
        for env in envs:
            env.physics.sync()
        for p in (ptr, own.value):
            after = np.empty_like(a)
            _copy_d2h(after, p)
            np.testing.assert_array_equal(after, a)
        ref = (_obs(envs[0]), _ctrl(envs[0]), envs[0].previous_action())
        assert not np.array_equal(ref[2], a)  # the command was filtered
        for env in envs[1:]:
            for x, y in zip(ref, (_obs(env), _ctrl(env), env.previous_action())):
                np.testing.assert_array_equal(x, y)
    _hip_runtime().hipFree(own)
    for env in envs:
        env.close()


def test_rejections(built):
    """Bad settings return DX_EINVAL and dx_last_error says why; an env never configured
    has no previous action."""
    L = _lib.load()
    env = _load(2)
    with pytest.raises(_lib.DxError, match="never configured"):
        env.previous_action()

    def rc(flags, scale=0.0, alpha=0.0):
        f = _lib.ActionFilter(flags=flags, noise_scale=scale, smooth_alpha=alpha, noise_seed=0)
        return L.dx_env_set_action_filter(env.ptr, ctypes.byref(f))

    nan = float("nan")
    for flags, scale, alpha, why in ((_lib.ACT_SMOOTH, 0.0, 1.5, b"smooth_alpha"), (_lib.ACT_SMOOTH, 0.0, -0.1, b"smooth_alpha"),
                                     (_lib.ACT_SMOOTH, 0.0, nan, b"smooth_alpha"), (_lib.ACT_NOISE, -1.0, 0.0, b"noise_scale"),
                                     (_lib.ACT_NOISE, nan, 0.0, b"noise_scale"), (_lib.ACT_NOISE, float("inf"), 0.0, b"noise_scale"),
                                     (8, 0.0, 0.0, b"flags")):
        assert rc(flags, scale, alpha) == -1, (flags, scale, alpha)
        assert why in L.dx_last_error()
    with pytest.raises(_lib.DxError, match="smooth_alpha"):
        env.configure_actions(smooth_alpha=1.5)
    # nothing was switched on by the refused calls
    assert env.action_config["smooth_alpha"] is None
    assert L.dx_env_action_noise_draw(env.ptr, 1, ctypes.c_void_p()) == -1
    assert rc(_lib.ACT_SMOOTH | _lib.ACT_NOISE, 0.0, 1.0) == 0 and rc(0) == 0
    assert L.dx_env_set_action_filter(env.ptr, None) == 0
    env.close()
