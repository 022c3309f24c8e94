"""The action wrappers' host side (no GPU): ExponentialSmoother against the reference's
semantics (effectors/wrappers/smooth_action.py), the wrappers' delegation and stage
merging against a stand-in env, and the C ABI's new names."""

import numpy as np
import pytest

from dexterity_amd import _lib, wrappers
from dexterity_amd.specs import BoundedArray


def test_exponential_smoother_semantics():
    ema = wrappers.ExponentialSmoother(0.7)
    assert ema.alpha == 0.7
    with pytest.raises(ValueError):
        ema.smoothed_value  # nothing seen yet
    x0 = np.array([0.25, -1.0, 3.0])
    ema.update(x0)
    np.testing.assert_array_equal(ema.smoothed_value, x0)  # the first value seeds it
    held = x0
    for x in (np.array([1.0, 1.0, 1.0]), np.array([-0.5, 0.125, 2.0])):
        ema.update(x)
        held = 0.7 * held + (1 - 0.7) * x
        np.testing.assert_array_equal(ema.smoothed_value, held)


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_exponential_smoother_edges(alpha):
    ema = wrappers.ExponentialSmoother(alpha)
    a, b = np.array([1.0, 2.0]), np.array([5.0, -3.0])
    ema.update(a)
    ema.update(b)
    np.testing.assert_array_equal(ema.smoothed_value, b if alpha == 0.0 else a)


@pytest.mark.parametrize("alpha", [-0.01, 1.5, float("nan"), float("inf")])
def test_exponential_smoother_rejects_alpha_outside_unit_interval(alpha):
    with pytest.raises(ValueError):
        wrappers.ExponentialSmoother(alpha)


class _Env:
    """What the wrappers use of GoalEnvironment."""

    def __init__(self, lo=-1.0, hi=1.0):
        self.action_config = dict(noise_scale=None, noise_seed=None, smooth_alpha=None, previous_action=False)
        self.calls = []
        self.num_envs = 3
        self._spec = BoundedArray((2,), np.float32, np.full(2, lo, np.float32), np.full(2, hi, np.float32))

    def action_spec(self):
        return self._spec

    def configure_actions(self, **kw):
        self.calls.append(kw)
        self.action_config = dict(kw)

    def previous_action(self):
        return np.zeros((3, 2), np.float32)


def test_wrappers_switch_their_stage_on_and_delegate():
    env = _Env()
    w = wrappers.PreviousAction(wrappers.ActionNoise(wrappers.SmoothAction(env, 0.7), 0.05))
    assert env.calls[0] == dict(noise_scale=None, noise_seed=None, smooth_alpha=0.7, previous_action=False)
    # each wrapper keeps the stages already on
    assert env.action_config == dict(noise_scale=0.05, noise_seed=None, smooth_alpha=0.7, previous_action=True)
    assert w.num_envs == 3 and w.environment.environment.environment is env  # every other attribute is the env's
    assert w.previous_action.shape == (3, 2)
    assert wrappers.PreviousAction(w).previous_action.shape == (3, 2)


def test_wrappers_reject_what_the_reference_rejects():
    with pytest.raises(ValueError):
        wrappers.SmoothAction(_Env(), 1.5)
    with pytest.raises(ValueError):
        wrappers.ActionNoise(_Env(hi=np.inf), 0.05)  # scale * (max - min) would be infinite
    env = _Env()
    env._spec = object()
    with pytest.raises(ValueError):
        wrappers.ActionNoise(env, 0.05)


def test_action_pipeline_symbols_are_declared():
    """The new entry points are in _lib.EXPORTS (test_abi's
    test_every_declared_symbol_is_exported then checks the header and the library)."""
    assert {"dx_env_set_action_filter", "dx_env_action_noise_draw"} <= set(_lib.EXPORTS)
    assert _lib.OUT_PREV_ACTION == 8
    assert (_lib.ACT_NOISE, _lib.ACT_SMOOTH, _lib.ACT_PREVIOUS) == (1, 2, 4)
    # struct dx_action_filter: int32, float, double, uint64 -- 24 bytes, no padding surprises
    import ctypes

    assert ctypes.sizeof(_lib.ActionFilter) == 24
    assert _lib.ActionFilter.smooth_alpha.offset == 8 and _lib.ActionFilter.noise_seed.offset == 16
