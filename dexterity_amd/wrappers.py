"""The reference's action-side wrappers, by their names and call shapes.

In the reference these wrap one environment (or its effector) in Python:
  ActionNoise     manipulation/wrappers/action_noise.py      clipped Gaussian action noise
  SmoothAction    effectors/wrappers/smooth_action.py        exponential moving average
  PreviousAction  effectors/wrappers/previous_action.py      the last command
Here each one switches on its stage of the batched env's device pipeline
(`GoalEnvironment.configure_actions`, include/dx.h dx_env_set_action_filter), which runs
ahead of every control step and sees the auto-reset inside it; every other attribute is
the wrapped env's.  They nest in any order -- the device applies noise, then stores the
previous action, then smooths, as the reference's environment wrapper sits outside its
effector wrappers.  Two deviations from the reference: the noise has a stream of its own
per env, RandomState(noise_seed + env_offset + e), not the environment's; and
`previous_action` is the command after the noise and before the smoothing.

`ExponentialSmoother` is the host restatement of the moving average.
"""

from __future__ import annotations

from typing import Any, Optional

import numpy as np

from dexterity_amd.specs import BoundedArray


class ExponentialSmoother:
    """An exponential moving average (smooth_action.py:10-34): the first value seeds it,
    every later one gives alpha * held + (1 - alpha) * value."""

    def __init__(self, alpha: float) -> None:
        if not (alpha >= 0.0 and alpha <= 1.0):  # (also refuses NaN, as the device does)
            raise ValueError(f"alpha = {alpha!r} is outside [0, 1]")
        self.alpha = alpha
        self._held = None  # nothing seen yet (this episode)

    def update(self, value: np.ndarray) -> None:
        held, a = self._held, self.alpha
        self._held = value if held is None else a * held + (1 - a) * value

    @property
    def smoothed_value(self) -> np.ndarray:
        if self._held is None:
            raise ValueError("the smoother has not been given a value yet")
        return self._held


class Wrapper:
    """Delegates every attribute to the wrapped env (manipulation/wrappers/base.py)."""

    def __init__(self, environment) -> None:
        self._environment = environment

    def __getattr__(self, name: str) -> Any:
        return getattr(self._environment, name)

    @property
    def environment(self):
        return self._environment

    def _configure(self, **stage) -> None:
        """Switches a stage on beside the ones already on."""
        self._environment.configure_actions(**{**self._environment.action_config, **stage})


class ActionNoise(Wrapper):
    """Gaussian noise of stddev scale * (maximum - minimum) on every action, clipped to
    the action spec (action_noise.py:9-26)."""

    def __init__(self, environment, scale: float, seed: Optional[int] = None) -> None:
        super().__init__(environment)
        spec = environment.action_spec()
        if not isinstance(spec, BoundedArray):
            raise ValueError("Only `BoundedArray` action specs are supported.")
        if not (np.all(np.isfinite(spec.minimum)) and np.all(np.isfinite(spec.maximum))):
            raise ValueError("ActionNoise needs an action spec that is bounded everywhere.")
        self._configure(noise_scale=scale, noise_seed=seed)


class SmoothAction(Wrapper):
    """Smooths the commands with an exponential moving average that restarts with every
    episode (smooth_action.py:37-63)."""

    def __init__(self, environment, alpha: float) -> None:
        super().__init__(environment)
        ExponentialSmoother(alpha)  # the reference's ValueError for alpha outside [0, 1]
        self._alpha = alpha
        self._configure(smooth_alpha=alpha)

    @property
    def alpha(self) -> float:
        return self._alpha


class PreviousAction(Wrapper):
    """Stores the most recent command of every env (previous_action.py:10-34)."""

    def __init__(self, environment) -> None:
        super().__init__(environment)
        self._configure(previous_action=True)

    @property
    def previous_action(self) -> np.ndarray:
        """[num_envs, nu] host copy; zeros at the start of an episode."""
        inner = self._environment.previous_action  # the env's method, or a nested wrapper's value
        return inner() if callable(inner) else inner


__all__ = ["ActionNoise", "SmoothAction", "PreviousAction", "ExponentialSmoother", "Wrapper"]
