"""How many rows the exact line search keeps in registers (Ctx::ls_slots: a scene
specialization keeps its own row bound, three slots of 64 in reorient instead of five) is
bookkeeping, not arithmetic: every result stays what it was.
tests/golden/newton_parent.npz (tools/record_newton_golden.py, run with the parent
revision's library) holds Newton solves the other goldens do not reach -- one that ends with
no iteration on a non-empty row set, solves of one and of four or more iterations,
friction-loss rows in both linear zones, a joint on its limit beside active contacts, 65..128
rows on the reorient specialization (its second slot), and 129..176 rows inside the
32-contact pool.  Each case is replayed on this tree's library and compared byte for byte.
Not covered: the 129..176-row scene matches no specialization, so it runs the generic
kernel, whose five slots did not change; no case here, and no scene the suite has, puts more
than 128 rows through a specialization's three-slot line search (the reorient runs reach
100).  The cases were chosen for a wider change of the Newton path that was measured and not
kept and stay as the yardstick for the next one.

The tiers compile the same functions with other pool sizes: a run with every contact step
forced to the mid tier, and one with DX_MID_DEFER_AT=0 on top (the mid tier then hands every
step that has a contact on to the overflow tier), equal the default path bit for bit.  The
library exports no counter that tells the two tiers apart (contact_deferred counts the step
kernel's deferrals only), so that the second run went through the overflow tier rests on
that switch, as in tests/test_gpu_prof_twin.py."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_newton_golden", os.path.join(ROOT, "tools", "record_newton_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def newton_golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "newton_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def _case(golden, key):
    return {k[len(key) + 1:]: v for k, v in golden.items() if k.startswith(key + "/")}


def _assert_equal(got, want):
    assert set(got) == set(want)
    for name, a in got.items():
        a, b = np.asarray(a), want[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name


def test_golden_holds_the_solves(newton_golden):
    """The recorded runs (the parent's own) contain each solve the golden is there for."""
    REC.check_env_run(_case(newton_golden, "reorient_64"))
    for key in REC.PHYS_CASES:
        REC.check_phys_run(key, _case(newton_golden, key))


def test_env_results_are_the_parents(newton_golden):
    """64 reorient envs x 6 control steps: state, warm start, qacc, task outputs, step types,
    health counters, the census and the final state's contact records, bit for bit."""
    _assert_equal(REC.run_env_case(**REC.ENV_CASE), _case(newton_golden, "reorient_64"))


@pytest.mark.parametrize("key", REC.PHYS_CASES)
def test_phys_results_are_the_parents(newton_golden, key):
    """The small scenes: the forward pass and three substeps, bit for bit."""
    _assert_equal(REC.run_phys_case(key), _case(newton_golden, key))


TIER_ENVS = {"mid": {"DX_DEFER_AT": "0"}, "overflow": {"DX_DEFER_AT": "0", "DX_MID_DEFER_AT": "0"}}
COMPARED = ("qpos", "qvel", "warmstart", "qacc", "observation", "reward", "discount", "step_types")


def _tier_run(monkeypatch, env):
    """16 reorient envs x 2 control steps with the device random agent."""
    from dexterity_amd import _lib, manipulation

    for k in REC.GUARD.ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = manipulation.GoalEnvironment(manipulation.SUITE[("reorient", "state_dense")](), num_envs=16, seed=REC.GUARD.SEED)
    ph = e.physics
    e.reset()
    types, ncon_max = [], 0
    for i in range(2):
        e.step_random(i)
        types.append(np.asarray(e.timestep().step_type).astype(np.int32))
        ncon_max = max(ncon_max, int(ph.get(_lib.NCON).max()))
    ts = e.timestep()
    out = {"qpos": ph.qpos, "qvel": ph.qvel, "warmstart": ph.get(_lib.QACC_WARMSTART), "qacc": ph.qacc,
           "observation": np.concatenate([np.asarray(v).reshape(16, -1) for v in ts.observation.values()], axis=1),
           "reward": np.asarray(ts.reward), "discount": np.asarray(ts.discount), "step_types": np.stack(types),
           "deferred": int(ph.health()["contact_deferred"]), "ncon_max": ncon_max}
    e.close()
    return out


@pytest.fixture(scope="module")
def default_run():
    mp = pytest.MonkeyPatch()
    try:
        return _tier_run(mp, {})
    finally:
        mp.undo()


@pytest.mark.parametrize("tier", list(TIER_ENVS))
def test_tiers_equal_the_default_path(default_run, monkeypatch, tier):
    """Every physics step with a contact deferred to the mid tier, and through it to the
    overflow tier: the same results as the step kernel's own solves, bit for bit."""
    got = _tier_run(monkeypatch, TIER_ENVS[tier])
    assert default_run["ncon_max"] > 0 and default_run["deferred"] == 0 and got["deferred"] > 0
    for name in COMPARED:
        a, b = got[name], default_run[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.isfinite(a).all(), name
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name
