"""The stage profiler is compiled out of the production step kernels and kept in instrumented
twins (dx_device.h DX_PROF; build.py compiles every dx_step.hip unit twice).  A batch runs the
twins exactly while stage timing is on (dx_stage_timing), so the same calls with timing off
and on run two different kernels, which must compute the same thing bit for bit: the
reorient specialization's queue kernel, the generic kernel (a scene no specialization
matches) and the mid and overflow tiers.  And the twins still profile: dx_stage_read hands
out cycles and counts with timing on and fails with timing off."""

import ctypes
import functools

import numpy as np
import pytest

from dexterity_amd import _lib, build

pytestmark = pytest.mark.gpu

SEED = 4321
SWITCHES = ("DX_GENERIC_KERNEL", "DX_DEFER_AT", "DX_MID_DEFER_AT", "DX_NO_MID", "DX_NO_QUEUE")
HEALTH = ("contact_overflow", "row_overflow", "diverged", "contact_deferred")  # (those that timing cannot change)
COMPARED = ("qpos", "qvel", "warmstart", "observation", "reward", "discount", "step_type")


@pytest.fixture(scope="module")
def built():
    build.build()


def _power3(compiled):
    """The scene with every geom pair's solimp power 3: no specialization is a power-3
    kernel (tests/test_solimp_power.py), so it runs the generic kernel."""
    from dexterity_amd.mjcf.compiler import CompiledModel

    arrays = {k: np.array(v, copy=True) for k, v in compiled.arrays.items()}
    t = arrays["gpair_solimp"].reshape(-1, 5)
    assert t.shape[0] > 0
    t[:, 4] = 3.0
    arrays["gpair_solimp"] = t.reshape(compiled.arrays["gpair_solimp"].shape)
    return CompiledModel(arrays, {k: list(v) for k, v in compiled.names.items()})


def _run(monkeypatch, nenv, steps, timing, env=None, power3=False):
    """`steps` control steps of reorient with the device random agent; the final state, the
    task outputs, the step types of every step, the health counters, the most contacts an
    env ended a step with, and (timing on) the stage record summed over the envs."""
    from dexterity_amd import manipulation

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    task = manipulation.SUITE[("reorient", "state_dense")]()
    if power3:
        task.compiled = _power3(task.compiled)
    e = manipulation.GoalEnvironment(task, num_envs=nenv, seed=SEED)
    L, ph = _lib.load(), e.physics
    if power3:  # the model's last layout word is the power-2 flag: clear, so no specialization matches
        buf = (ctypes.c_int32 * 256)()
        n = L.dx_model_layout(ph.model.ptr, buf, 256)
        assert n > 0 and buf[n - 1] == 0
    if timing:
        _lib.check(L.dx_stage_timing(ph.ptr, 1))
    e.reset()
    types, ncon_max = [], 0
    for i in range(steps):
        e.step_random(i)
        types.append(np.asarray(e.timestep().step_type).astype(np.int32))
        ncon_max = max(ncon_max, int(ph.get(_lib.NCON).max()))
    ts = e.timestep()
    h = ph.health()
    out = {"qpos": ph.qpos, "qvel": ph.qvel, "warmstart": ph.get(_lib.QACC_WARMSTART),
           "observation": np.concatenate([np.asarray(v).reshape(nenv, -1) for v in ts.observation.values()], axis=1),
           "reward": np.asarray(ts.reward), "discount": np.asarray(ts.discount), "step_type": np.stack(types),
           "health": {k: int(h[k]) for k in HEALTH}, "ncon_max": ncon_max}
    stage = (ctypes.c_uint64 * _lib.NSTAGE)()
    out["stage_rc"] = L.dx_stage_read(ph.ptr, stage, _lib.NSTAGE)
    out["stage_error"] = L.dx_last_error().decode() if out["stage_rc"] < 0 else ""
    out["stage"] = np.array(stage[:], dtype=np.uint64)
    e.close()
    return out


def _assert_same(off, on):
    for name in COMPARED:
        a, b = off[name], on[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.isfinite(a).all(), name
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name
    assert off["health"] == on["health"]
    assert off["health"]["contact_overflow"] == 0 and off["health"]["row_overflow"] == 0 and off["health"]["diverged"] == 0


@functools.lru_cache(maxsize=None)
def _reorient_runs():
    """Reorient (Newton) at 64 envs x 6 control steps, stage timing off and on: shared by the
    two tests below."""
    mp = pytest.MonkeyPatch()
    try:
        return _run(mp, 64, 6, False), _run(mp, 64, 6, True)
    finally:
        mp.undo()


def test_twin_equals_production_reorient(built):
    """The reorient specialization's production kernels and their twins: bit for bit."""
    off, on = _reorient_runs()
    assert off["ncon_max"] > 0 and on["ncon_max"] > 0  # the narrowphase and the solver ran
    _assert_same(off, on)


def test_twin_equals_production_generic_kernel(built, monkeypatch):
    """A power-3 scene, which no specialization matches: the generic kernel and its twin."""
    off = _run(monkeypatch, 16, 2, False, power3=True)
    on = _run(monkeypatch, 16, 2, True, power3=True)
    assert off["ncon_max"] > 0
    _assert_same(off, on)
    assert on["stage_rc"] == 0 and on["stage"][_lib.STAGES.index("kinematics")] > 0  # (the twin ran)


@pytest.mark.parametrize("env", [{"DX_DEFER_AT": "0"}, {"DX_DEFER_AT": "0", "DX_MID_DEFER_AT": "0"}],
                         ids=["mid", "overflow"])
def test_twin_equals_production_tiers(built, monkeypatch, env):
    """Every physics step with a contact deferred to the mid tier, and through it to the
    overflow tier: the tier kernels and their twins."""
    off = _run(monkeypatch, 16, 2, False, env=env)
    on = _run(monkeypatch, 16, 2, True, env=env)
    assert off["ncon_max"] > 0 and off["health"]["contact_deferred"] > 0
    _assert_same(off, on)


def test_profiler_still_profiles(built):
    """Timing on: cycles for kinematics, the MPR narrowphase and the Newton Cholesky, counts
    of Newton iterations and narrowphase trips.  Timing off: dx_stage_read fails as before."""
    off, on = _reorient_runs()
    assert on["stage_rc"] == 0
    stage = on["stage"]
    for name in ("kinematics", "np_mpr", "newton_chol"):
        assert stage[_lib.STAGES.index(name)] > 0, name
    counters = {v: k for k, v in _lib.COUNTERS.items()}
    for name in ("newton_iter", "np_trips"):
        assert stage[counters[name]] > 0, name
    assert off["stage_rc"] < 0 and "stage timing not enabled" in off["stage_error"]
