"""Host side of the per-env applied wrenches and the random pushes: the numpy replay of the
schedule (tests/perturb_ref.py) shows what the device test compares against, the pushes'
statistics, and the argument checks that run before any library call."""

import types

import numpy as np
import pytest

from dexterity_amd import _lib
from tests import perturb_ref as ref


def _replay(nb=1, **over):
    st = ref.fixed_episodes(ref.NENV, ref.NSTEPS, ref.EPISODE)
    kw = dict(ref.SETTINGS, **over)
    w, started = ref.replay(st, nb, **kw)
    return st, w, started, kw


def test_replay_shows_cut_chained_and_frequent_pushes():
    """16 envs x 30 steps, 12-step episodes, probability 0.25, duration 3: the replay alone
    has a push cut short by an episode reset, a push followed by a new one on the very next
    step, and a wrench on at least a quarter of the non-FIRST env-steps."""
    st, w, started, kw = _replay()
    s = ref.summary(w, started, st, kw["duration"])
    print(s)
    assert s["cut"] >= 1 and s["back_to_back"] >= 1 and s["carrying"] >= 0.25
    # FIRST rows carry nothing, and no push outlasts its duration
    assert not w[st == ref.FIRST].any()
    on = np.abs(w).sum(axis=3)[:, :, 0] > 0
    for e in range(ref.NENV):
        run = 0
        for i in range(ref.NSTEPS):
            run = 0 if (not on[i, e] or started[i, e, 0]) else run
            run += on[i, e]
            assert run <= kw["duration"]
    # a held push keeps its value
    for i in range(1, ref.NSTEPS):
        held = on[i] & ~started[i, :, 0]
        np.testing.assert_array_equal(w[i][held], w[i - 1][held])


def test_replay_consumption_is_fixed():
    """Seven doubles per body and step whatever branch is taken: after n steps every env's
    stream stands where RandomState(seed + e) stands after 7 nb n doubles, for two bodies and
    whatever the step types were."""
    nb = 2
    r = ref.Replay(4, nb, **{k: v for k, v in ref.SETTINGS.items()})
    rng = np.random.RandomState(0)
    for _ in range(9):
        r.step(rng.rand(4) < 0.3)
    for e in range(4):
        want = np.random.RandomState(ref.SETTINGS["seed"] + e)
        want.random_sample(ref.DRAWS * nb * 9)
        assert r.rs[e].random_sample() == want.random_sample()


def test_push_statistics():
    """10^4 pushes: unit directions to 1e-12, magnitudes inside their ranges, and a mean
    direction within 4 standard errors of zero (a uniform direction's components have
    variance 1/3)."""
    n = 10000
    u = np.random.RandomState(5).random_sample((n, ref.DRAWS))
    fr, tr = (0.5, 2.0), (0.01, 0.03)
    dirs = np.array([ref.direction(x[2], x[3]) for x in u])
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1.0).max() <= 1e-12
    se = np.sqrt(1.0 / 3.0 / n)
    assert np.abs(dirs.mean(axis=0)).max() <= 4 * se, dirs.mean(axis=0)
    w = np.array([ref.wrench(x, fr, tr) for x in u]).astype(np.float64)
    f, t = np.linalg.norm(w[:, :3], axis=1), np.linalg.norm(w[:, 3:], axis=1)
    eps = 2.0 ** -23
    assert f.min() >= fr[0] * (1 - 2 * eps) and f.max() <= fr[1] * (1 + 2 * eps)
    assert t.min() >= tr[0] * (1 - 2 * eps) and t.max() <= tr[1] * (1 + 2 * eps)
    # a degenerate range gives exactly that magnitude
    w0 = ref.wrench(u[0], (1.5, 1.5), (0.0, 0.0))
    assert abs(np.linalg.norm(w0[:3].astype(np.float64)) - 1.5) <= 1.5 * 2 * eps and not w0[3:].any()


def test_symbols_and_struct():
    for name in ("dx_set_xfrc_env", "dx_get_xfrc_env", "dx_xfrc_ptr", "dx_env_set_perturbation", "dx_env_perturb_draw"):
        assert name in _lib.EXPORTS
    assert _lib.OUT_PERTURB == 12 and _lib.PERTURB_MAX_BODIES == 4
    p = _lib.Perturbation()
    assert [f[0] for f in p._fields_] == ["nbody", "bodies", "probability", "force_min", "force_max", "torque_min",
                                          "torque_max", "duration", "seed"]
    import ctypes
    # the C layout: int32 nbody, int32[4], (4 bytes padding), 5 doubles, int32, (padding), uint64
    assert ctypes.sizeof(p) == 80 and _lib.Perturbation.probability.offset == 24 and _lib.Perturbation.seed.offset == 72


def _physics_stub(nbody=5, nenv=3):
    from dexterity_amd import physics

    # ptr None: any library call would fail loudly; the shape checks come first
    return physics.BatchedPhysics.borrowed(types.SimpleNamespace(nbody=nbody), None, nenv, 0)


@pytest.mark.parametrize("shape", [(30,), (5, 5), (4, 6), (2, 4, 6), (4, 5, 6), (0, 5, 6), (1, 3, 5, 6), ()])
def test_set_xfrc_wrong_shapes(shape, monkeypatch):
    ph = _physics_stub()
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("a library call before the shape check"))
    with pytest.raises(ValueError, match="xfrc must be"):
        ph.set_xfrc(np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="xfrc must be"):
        ph.set_xfrc(np.zeros((2, 5, 6), np.float32), env0=2)  # env0 + n beyond nenv


@pytest.fixture(scope="module")
def reorient_task():
    from dexterity_amd import manipulation

    return manipulation.ReOrient()


BAD = [
    dict(bodies=()), dict(bodies=("prop",) * 2), dict(bodies=("world",)), dict(bodies=("no such body",)),
    dict(bodies=("shadow_hand_e/ffdistal", "shadow_hand_e/mfdistal", "shadow_hand_e/rfdistal", "shadow_hand_e/lfdistal",
                 "prop")),
    dict(probability=-0.1), dict(probability=1.5), dict(probability=float("nan")),
    dict(force_range=(1.0, 0.5)), dict(force_range=(-1.0, 0.5)), dict(force_range=(0.0, float("inf"))),
    dict(force_range=1.0), dict(torque_range=(0.2, 0.1)), dict(torque_range=(float("nan"), 1.0)),
    dict(duration_steps=0), dict(duration_steps=-3), dict(duration_steps=1.5), dict(duration_steps=True),
]


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_configure_perturbations_rejects_before_the_library(reorient_task, bad, monkeypatch):
    from dexterity_amd import manipulation

    good = dict(bodies=("prop",), probability=0.25, force_range=(0.1, 0.6), torque_range=(0.0, 0.002), duration_steps=3)
    opt = manipulation.perturbation_settings(reorient_task, seed=3, **good)
    assert opt["body_ids"] == (reorient_task.prop_body,) and opt["duration_steps"] == 3 and opt["seed"] == 3
    env = object.__new__(manipulation.GoalEnvironment)
    env.task, env.ptr, env._seed, env.perturbation_options = reorient_task, None, 0, None
    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("a library call before the argument check"))
    with pytest.raises(ValueError):
        env.configure_perturbations(**dict(good, **bad))
    assert env.perturbation_options is None


def test_reach_refuses(monkeypatch):
    from dexterity_amd import manipulation

    reach = types.SimpleNamespace(kind=_lib.TASK_REACH)
    with pytest.raises(ValueError, match="reach"):
        manipulation.perturbation_settings(reach, ("prop",), 0.5, (0.0, 1.0))


def test_body_names_resolve(reorient_task):
    from dexterity_amd import manipulation

    names = reorient_task.compiled.names["body"]
    opt = manipulation.perturbation_settings(reorient_task, ("prop", "shadow_hand_e/ffdistal"), 1.0, (0, 1))
    assert opt["body_ids"] == (names.index("prop/"), names.index("shadow_hand_e/ffdistal"))
    assert manipulation.perturbation_settings(reorient_task, "prop", 0.0, (0, 0))["body_ids"] == (names.index("prop/"),)
