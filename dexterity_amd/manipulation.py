"""Task suite and batched environments (manipulation/__init__.py in the reference).

`load(domain, task, seed, num_envs, device)` mirrors `manipulation.load`
(manipulation/__init__.py:56-86) and returns a `GoalEnvironment` whose
`reset()` / `step(action)` follow dm_env semantics for every one of `num_envs`
environments at once (batched TimeStep, leading env axis).  The physics and the
task logic run on the GPU (dx_env_* in include/dx.h); these classes hold the
reference's constants and the host-side API.

Suite (names as in the reference):
  reorient.state_dense   manipulation/tasks/reorient.py:367-371  (Shadow hand + cube)
  reach.state_dense      manipulation/tasks/reach.py:252-259     (Adroit hand, fingertip goals)
  reach.state_sparse     manipulation/tasks/reach.py:262-269
  reach_shadow.state_dense  BASELINE.json config 2: reach with the Shadow hand,
                         contact-free smooth dynamics (not a reference suite entry)
  bimanual.state_dense   BASELINE.json config 5: two Shadow hands hand the cube over
                         (Handover; not a reference suite entry)
"""

from __future__ import annotations

import collections
import ctypes
import dataclasses
import os
from typing import Dict, Optional

import numpy as np

from dexterity_amd import _lib
from dexterity_amd import cameras as cameras_lib
from dexterity_amd import effectors as effectors_lib
from dexterity_amd import hands as hands_lib
from dexterity_amd import physics as physics_lib
from dexterity_amd.mjcf.compiler import CompiledModel
from dexterity_amd.specs import Array, BoundedArray, StepType, TimeStep

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


@dataclasses.dataclass(frozen=True)
class ReOrientConfig:
    """Constants of manipulation/tasks/reorient.py:40-78 and GoalTask defaults."""

    physics_timestep: float = 0.005  # reorient.py:58
    control_timestep: float = 0.025  # reorient.py:61
    orientation_eps: float = 0.1  # reorient.py:50
    orientation_threshold: float = 0.1  # reorient.py:52
    orientation_weight: float = 1.0  # reorient.py:54
    success_bonus_weight: float = 800.0  # reorient.py:55
    action_smoothing_weight: float = -0.1  # reorient.py:56
    successes_needed: int = 1  # reorient.py:64
    max_steps_single_solve: int = 300  # reorient.py:67
    steps_before_moving_target: int = 5  # reorient.py:70
    fall_termination: bool = True  # reorient.py:103
    prop_bbox_lower: tuple = (-0.025, -0.155, 0.16)  # reorient.py:72-78
    prop_bbox_upper: tuple = (0.025, -0.105, 0.16)

    @property
    def n_sub_steps(self) -> int:
        return int(round(self.control_timestep / self.physics_timestep))

    @property
    def max_time_per_goal(self) -> float:
        return self.max_steps_single_solve * self.control_timestep


# The optional hand observables (GoalEnvironment.enable_observables; include/dx.h
# dx_env_set_hand_observables), in the reference's declaration order
# (dexterous_hand.py:245-372) -- the order of a hand's blocks in a DX_OUT_HAND_OBS row:
# name -> (mask bit, floats per joint, floats per fingertip)
HAND_EXTRA_OBSERVABLES = collections.OrderedDict((
    ("joint_positions", (_lib.HOBS_JOINT_POSITIONS, 1, 0)),
    ("fingertip_orientations", (_lib.HOBS_TIP_ORIENTATIONS, 0, 4)),
    ("fingertip_angular_velocities", (_lib.HOBS_TIP_ANGULAR_VELOCITIES, 0, 3)),
    ("fingertip_positions_ego", (_lib.HOBS_TIP_POSITIONS_EGO, 0, 3)),
))
HAND_ROOT_BODY = "forearm"  # hand.root_body: shadow_hand_e.py:62, adroit_hand.py:57
CONTACT_FORCES_KEY = "hand_contact_forces"  # GoalEnvironment.enable_contact_forces


def _whole_number(name: str, value) -> int:
    if callable(value):
        raise ValueError(f"{name}: callables are not supported (composer allows them; the device pipeline "
                         "takes constants)")
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {value!r}")
    return int(value)


def obs_pipeline_options(n_sub_steps: int, update_interval=None, buffer_size=1, delay=0, aggregator=None,
                         padding: str = "zero", noise_std=None, widths=None):
    """Composer's observable options (ObservableSpec, manipulation/shared/observations.py:8-17)
    in the units of include/dx.h dx_obs_pipeline.  Pure host code: no library, no GPU.

    Composer counts `update_interval` and `delay` in PHYSICS steps; the device has an
    observation only at control-step boundaries, so both must be multiples of
    `n_sub_steps` -- except composer's default, interval 1 with buffer 1, which reads the
    same as interval `n_sub_steps` (`update_interval=None` means that default).  `widths` is
    the row: an ordered mapping from observable name to its width or its slice of the row.
    `noise_std` (additive Gaussian noise, one draw per row element and sample) is None for
    no noise, a float, an array [W], or a dict from observable name to a float or an array
    of that observable's width; names absent from the dict get 0.

    Returns (m, d, K, aggregator code, padding code, sigma) with m and d in control steps
    and sigma a float64 [W] array or None.  Raises ValueError with the reason otherwise."""
    nsub = _whole_number("n_sub_steps", n_sub_steps)
    if nsub < 1:
        raise ValueError("n_sub_steps must be at least 1")
    K = _whole_number("buffer_size", buffer_size)
    if K < 1:
        raise ValueError(f"buffer_size must be at least 1, got {K}")
    if K > _lib.OBS_BUFFER_MAX:
        raise ValueError(f"buffer_size {K} is above the device limit of {_lib.OBS_BUFFER_MAX}")
    interval = nsub if update_interval is None else _whole_number("update_interval", update_interval)
    if interval < 1:
        raise ValueError(f"update_interval must be at least 1, got {interval}")
    if interval % nsub == 0:
        m = interval // nsub
    elif interval == 1 and K == 1:
        m = 1  # composer's default: the boundary read returns the boundary's own sample
    else:
        raise ValueError(f"update_interval {interval} is not a multiple of n_sub_steps {nsub}: samples inside a "
                         "control step are not built (only interval 1 with buffer_size 1 is, composer's default)")
    delay = _whole_number("delay", delay)
    if delay < 0:
        raise ValueError(f"delay must not be negative, got {delay}")
    if delay % nsub:
        raise ValueError(f"delay {delay} is not a multiple of n_sub_steps {nsub}: arrivals inside a control step "
                         "are not built")
    d = delay // nsub
    if m > _lib.OBS_INTERVAL_MAX or d > _lib.OBS_DELAY_MAX:
        raise ValueError(f"update_interval / delay of {m} / {d} control steps are above the device limits of "
                         f"{_lib.OBS_INTERVAL_MAX} / {_lib.OBS_DELAY_MAX}")
    if callable(aggregator):
        raise ValueError("aggregator: callables are not supported, name one of min, max, mean, median, sum")
    if aggregator not in _lib.OBS_AGG:
        raise ValueError(f"unknown aggregator {aggregator!r}: one of None, min, max, mean, median, sum")
    pad = padding.lower() if isinstance(padding, str) else padding
    if pad not in _lib.OBS_PAD:
        raise ValueError(f"unknown padding {padding!r}: 'zero' or 'initial_value' (composer's ObservationPadding)")
    slices, W = collections.OrderedDict(), 0
    for name, w in (widths or {}).items():
        w = (w.stop - w.start) if isinstance(w, slice) else int(w)
        slices[name] = slice(W, W + w)
        W += w
    sigma = None
    if noise_std is not None:
        if callable(noise_std):
            raise ValueError("noise_std: callables (custom corruptors) are not supported")
        if isinstance(noise_std, dict):
            unknown = [k for k in noise_std if k not in slices]
            if unknown:
                raise ValueError(f"noise_std names unknown observables {unknown}; the row has {list(slices)}")
            sigma = np.zeros(W, dtype=np.float64)
            for name, v in noise_std.items():
                if callable(v):
                    raise ValueError(f"noise_std[{name!r}]: callables are not supported")
                v = np.asarray(v, dtype=np.float64)
                s = slices[name]
                if v.ndim > 1 or (v.ndim == 1 and v.size != s.stop - s.start):
                    raise ValueError(f"noise_std[{name!r}] has {v.size} entries, the observable {s.stop - s.start}")
                sigma[s] = v
        else:
            v = np.asarray(noise_std, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.size != W):
                raise ValueError(f"noise_std has {v.size} entries, the row {W}")
            sigma = np.broadcast_to(v, (W,)).astype(np.float64)
        if not np.all(np.isfinite(sigma)) or np.any(sigma < 0):
            raise ValueError("noise_std must be finite and not negative")
    return m, d, K, _lib.OBS_AGG[aggregator], _lib.OBS_PAD[pad], sigma


def perturbation_settings(task, bodies=("prop",), probability=0.0, force_range=(0.0, 0.0), torque_range=(0.0, 0.0),
                          duration_steps=1, seed=0) -> dict:
    """`GoalEnvironment.configure_perturbations`' arguments, checked and resolved against
    `task` without touching the library: body names to ids ("prop" is the task's prop body),
    ranges to (min, max) floats.  ValueError for anything include/dx.h dx_env_set_perturbation
    would refuse."""
    if task.kind == _lib.TASK_REACH:
        raise ValueError("perturbations need a prop to push and a reset that does not step the physics: "
                         "the reach tasks have neither")
    names = [bodies] if isinstance(bodies, str) else list(bodies)
    if not 1 <= len(names) <= _lib.PERTURB_MAX_BODIES:
        raise ValueError(f"between 1 and {_lib.PERTURB_MAX_BODIES} bodies, got {len(names)}")
    body_names = task.compiled.names["body"]
    ids = []
    for n in names:
        if n == "prop":
            ids.append(int(task.prop_body))
        elif isinstance(n, str) and n in body_names:
            ids.append(body_names.index(n))
        else:
            raise ValueError(f"unknown body {n!r}")
    if any(i < 1 for i in ids):
        raise ValueError("the world body cannot be pushed")
    if len(set(ids)) != len(ids):
        raise ValueError(f"a body is named twice: {names}")
    probability = float(probability)
    if not 0.0 <= probability <= 1.0:  # (false for a NaN too)
        raise ValueError(f"probability must be within [0, 1], got {probability}")

    def rng(name, r):
        try:
            lo, hi = (float(v) for v in r)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a (min, max) pair, got {r!r}") from None
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo <= hi):
            raise ValueError(f"{name} must be finite with 0 <= min <= max, got {r!r}")
        return lo, hi

    force_range, torque_range = rng("force_range", force_range), rng("torque_range", torque_range)
    duration_steps = _whole_number("duration_steps", duration_steps)
    if duration_steps < 1:
        raise ValueError(f"duration_steps must be at least 1, got {duration_steps}")
    return dict(bodies=tuple(names), body_ids=tuple(ids), probability=probability, force_range=force_range,
                torque_range=torque_range, duration_steps=duration_steps, seed=int(seed))


def observation_layout(hand_nq: int, hand_nv: int, ntips: int, with_prop: bool, hand: str,
                       goal_dim: int = 4) -> "collections.OrderedDict[str, slice]":
    """Named slices of the flat observation vector written by dx_task_post_kernel."""
    out = collections.OrderedDict()
    k = 0

    def add(name, n):
        nonlocal k
        out[name] = slice(k, k + n)
        k += n

    add(f"{hand}/joint_positions_sin_cos", 2 * hand_nq)
    add(f"{hand}/joint_velocities", hand_nv)
    add(f"{hand}/fingertip_positions", 3 * ntips)
    add(f"{hand}/fingertip_linear_velocities", 3 * ntips)
    if with_prop:
        add("prop/position", 3)
        add("prop/orientation", 4)
        add("prop/linear_velocity", 3)
        add("prop/angular_velocity", 3)
        add("target_prop/orientation", 4)
    add("goal_state", goal_dim)
    return out


class ReOrient:
    """Batched counterpart of `ReOrient` (reorient.py:90-235)."""

    domain = "reorient"
    kind = _lib.TASK_REORIENT

    def __init__(self, config: ReOrientConfig = ReOrientConfig(), asset: str = "shadow_reorient.npz"):
        self.config = config
        self.compiled = CompiledModel.load(os.path.join(ASSETS, asset))
        cm = self.compiled
        if abs(cm.timestep - config.physics_timestep) > 1e-12:
            raise ValueError("asset timestep does not match the task's physics timestep")
        self.hand_name = "shadow_hand_e"
        self.hand_names = (self.hand_name,)
        names = cm.names
        self.hand_joint_ids = [i for i, n in enumerate(names["joint"]) if n.startswith(self.hand_name + "/")]
        self.hand_nq = len(self.hand_joint_ids)
        self.hand_nv = self.hand_nq
        prop_j = names["joint"].index("prop/")
        self.prop_qadr = int(cm.jnt_qposadr[prop_j])
        self.prop_dadr = int(cm.jnt_dofadr[prop_j])
        self.prop_body = names["body"].index("prop/")
        self.ground_geom = names["geom"].index("ground")
        tip_sites = [f"{self.hand_name}/{t}_site" for t in ("fftip", "mftip", "rftip", "lftip", "thtip")]
        self.tip_site0 = names["site"].index(tip_sites[0])
        assert [names["site"].index(s) for s in tip_sites] == list(range(self.tip_site0, self.tip_site0 + 5))
        self.ntips = 5
        self.actuator_ids = list(range(cm.nu))
        self.hand_effector = effectors_lib.HandEffector(self.actuator_ids, self.hand_name)
        self.gravity_compensation = physics_lib.gravity_compensation(cm, self.hand_name + "/")

    def params(self) -> np.ndarray:
        c = self.config
        p = np.zeros(38, dtype=np.float32)
        p[0] = c.n_sub_steps
        p[1], p[2] = self.hand_nq, self.hand_nv
        p[3], p[4] = self.prop_qadr, self.prop_dadr
        p[5], p[6] = self.tip_site0, self.ntips
        p[7], p[8], p[9] = c.successes_needed, c.steps_before_moving_target, int(c.fall_termination)
        p[10], p[11] = c.orientation_threshold, c.orientation_eps
        p[12], p[13], p[14] = c.orientation_weight, c.success_bonus_weight, c.action_smoothing_weight
        p[15] = c.max_time_per_goal
        p[16:19] = c.prop_bbox_lower
        p[19:22] = c.prop_bbox_upper
        p[22], p[23] = self.ground_geom, self.prop_body
        # the box in fp64 for the numpy-compatible spawn draws: raw bits in 26-37
        box = np.array(c.prop_bbox_lower + c.prop_bbox_upper, dtype=np.float64)
        p[26:38] = box.view(np.float32)
        return p

    def observation_layout(self):
        return observation_layout(self.hand_nq, self.hand_nv, self.ntips, True, self.hand_name)


@dataclasses.dataclass(frozen=True)
class HandoverConfig:
    """BASELINE.json config 5 as a task (synthetic: the reference has no bimanual task; its
    two-hand pattern is Juggle's hands and effectors, juggle.py:147-177 with
    arenas/arena.py:58-105).  Two Shadow hands palm-up side by side (mjcf/scenes.py
    bimanual_handover), the reorient cube spawned over the first (left) hand and handed to
    the target point above the other palm; GoalTask bookkeeping, reward in the shape of
    reorient.py:238-284 on the cube-to-target distance, fall termination of
    reorient.py:229-235.  Timesteps as reorient's."""

    physics_timestep: float = 0.005
    control_timestep: float = 0.025
    distance_eps: float = 0.05  # 1 / (d + eps), d in metres
    success_threshold: float = 0.02  # the cube within 2 cm of the receiving palm's target
    distance_weight: float = 1.0
    success_bonus_weight: float = 800.0  # reorient.py:55
    action_smoothing_weight: float = -0.1  # reorient.py:56
    successes_needed: int = 3  # handovers (there and back, and there again)
    max_steps_single_solve: int = 300  # reorient.py:67
    steps_before_moving_target: int = 5  # task.py's goal change: the cube goes back
    fall_termination: bool = True
    # the reorient spawn box (reorient.py:72-78) over the left hand (+0.12 m in x)
    prop_bbox_lower: tuple = (0.095, -0.155, 0.16)
    prop_bbox_upper: tuple = (0.145, -0.105, 0.16)
    # where the cube comes to rest on each palm from the spawn box's centre (the fp64
    # oracle: 0.1308 m high, 0.13 m in front of the forearms), left then right
    hand_targets: tuple = ((0.12, -0.13, 0.131), (-0.12, -0.13, 0.131))

    @property
    def n_sub_steps(self) -> int:
        return int(round(self.control_timestep / self.physics_timestep))

    @property
    def max_time_per_goal(self) -> float:
        return self.max_steps_single_solve * self.control_timestep


class Handover(ReOrient):
    """The two-hand cube handover behind the Task / Effector / Environment surface
    (HandoverConfig).  Both hands' joints, velocities and fingertips are the hand block of
    the observation (left then right, as the scene orders them), then the cube's pose and
    velocities and the goal [target xyz, receiving hand]."""

    domain = "bimanual"
    kind = _lib.TASK_HANDOVER

    def __init__(self, config: HandoverConfig = HandoverConfig(), asset: str = "bimanual_handover.npz"):
        self.config = config
        self.compiled = CompiledModel.load(os.path.join(ASSETS, asset))
        cm = self.compiled
        if abs(cm.timestep - config.physics_timestep) > 1e-12:
            raise ValueError("asset timestep does not match the task's physics timestep")
        names = cm.names
        self.hand_names = ("shadow_hand_left", "shadow_hand_right")
        self.hand_name = "bimanual"
        self.hand_joint_ids = [i for i, n in enumerate(names["joint"]) if n.startswith("shadow_hand_")]
        self.hand_nq = len(self.hand_joint_ids)
        self.hand_nv = self.hand_nq
        prop_j = names["joint"].index("prop/")
        self.prop_qadr = int(cm.jnt_qposadr[prop_j])
        self.prop_dadr = int(cm.jnt_dofadr[prop_j])
        if self.prop_qadr != self.hand_nq:  # the hands' joints first, then the cube's
            raise ValueError("bimanual scene: hand joints must precede the prop's")
        self.prop_body = names["body"].index("prop/")
        self.ground_geom = names["geom"].index("ground")
        tips = [f"{h}/{t}_site" for h in self.hand_names for t in ("fftip", "mftip", "rftip", "lftip", "thtip")]
        self.tip_site0 = names["site"].index(tips[0])
        assert [names["site"].index(s) for s in tips] == list(range(self.tip_site0, self.tip_site0 + 10))
        self.ntips = 10
        self.actuator_ids = list(range(cm.nu))
        self.hand_effector = effectors_lib.HandEffector(self.actuator_ids, self.hand_name)
        self.gravity_compensation = physics_lib.gravity_compensation(cm, "shadow_hand_")

    def params(self) -> np.ndarray:
        c = self.config
        p = np.zeros(44, dtype=np.float32)
        p[0] = c.n_sub_steps
        p[1], p[2] = self.hand_nq, self.hand_nv
        p[3], p[4] = self.prop_qadr, self.prop_dadr
        p[5], p[6] = self.tip_site0, self.ntips
        p[7], p[8], p[9] = c.successes_needed, c.steps_before_moving_target, int(c.fall_termination)
        p[10], p[11] = c.success_threshold, c.distance_eps
        p[12], p[13], p[14] = c.distance_weight, c.success_bonus_weight, c.action_smoothing_weight
        p[15] = c.max_time_per_goal
        p[16:19] = c.prop_bbox_lower
        p[19:22] = c.prop_bbox_upper
        p[22], p[23] = self.ground_geom, self.prop_body
        box = np.array(c.prop_bbox_lower + c.prop_bbox_upper, dtype=np.float64)
        p[26:38] = box.view(np.float32)
        p[38:44] = np.asarray(c.hand_targets, dtype=np.float32).ravel()
        return p

    def observation_layout(self):
        """Per-hand keys: the scene orders the left hand's joints, dofs and fingertips
        before the right's, so each hand's block is a contiguous slice."""
        out = collections.OrderedDict()
        nh, k = self.hand_nq // 2, 0
        blocks = (("joint_positions_sin_cos", 2 * nh), ("joint_velocities", nh), ("fingertip_positions", 15),
                  ("fingertip_linear_velocities", 15))
        for name, n in blocks:
            for h in self.hand_names:
                out[f"{h}/{name}"] = slice(k, k + n)
                k += n
        for name, n in (("prop/position", 3), ("prop/orientation", 4), ("prop/linear_velocity", 3),
                        ("prop/angular_velocity", 3), ("goal_state", 4)):
            out[name] = slice(k, k + n)
            k += n
        return out


@dataclasses.dataclass(frozen=True)
class ReachConfig:
    """Constants of manipulation/tasks/reach.py:30-70 and fingertip_position.py:21-35."""

    physics_timestep: float = 0.02  # reach.py:54
    control_timestep: float = 0.02  # reach.py:59
    success_threshold: float = 0.01  # reach.py:47 (_DISTANCE_TO_TARGET_THRESHOLD)
    successes_needed: int = 50  # reach.py:62
    steps_before_moving_target: int = 5  # reach.py:37
    max_steps_single_solve: int = 150  # reach.py:65
    init_joint_range_fraction: float = 0.5  # reach.py:34
    goal_scale: float = 0.1  # fingertip_position.py:26
    max_rejection_samples: int = 100  # fingertip_position.py:25
    dense_reward: bool = True  # reach.py:252-269 (state_dense / state_sparse)

    @property
    def n_sub_steps(self) -> int:
        return int(round(self.control_timestep / self.physics_timestep))

    @property
    def max_time_per_goal(self) -> float:
        return self.max_steps_single_solve * self.control_timestep


class Reach:
    """Batched counterpart of `Reach` (reach.py:73-210) over `GoalTask`.

    Goals come from the batched `FingertipCartesianPosition.next_goal`
    (fingertip_position.py:72-125: joint targets ~ N(midrange, 0.1 * range), two
    physics steps, rejected while the hand self-collides) and episodes start from
    `sample_collision_free_joint_angles(range_fraction=0.5)` (dexterous_hand.py:
    120-168); both run on the device inside the step kernel (dx_step.hip reach_prep).
    """

    domain = "reach"
    kind = _lib.TASK_REACH

    def __init__(self, config: ReachConfig = ReachConfig(), hand: str = "adroit"):
        self.config = config
        asset = {"adroit": "adroit_reach.npz", "shadow": "shadow_reach.npz"}[hand]
        self.compiled = CompiledModel.load(os.path.join(ASSETS, asset))
        cm = self.compiled
        if abs(cm.timestep - config.physics_timestep) > 1e-12:
            raise ValueError("asset timestep does not match the task's physics timestep")
        names = cm.names
        if hand == "adroit":
            self.hand_name = "adroit_hand"
            tips = [f"{self.hand_name}/{s}" for s in hands_lib.ADROIT_FINGERTIP_SITES]
            self.position_to_control = np.eye(cm.nu, cm.nq)  # adroit_hand.py:106-112
            coupled = []
        else:
            self.hand_name = "shadow_hand_e"
            tips = [f"{self.hand_name}/{t}_site" for t in hands_lib.SHADOW_FINGERTIPS]
            self.position_to_control = hands_lib.POSITION_TO_CONTROL  # shadow_hand_e.py:109-119
            coupled = [(ids[0], ids[-1]) for ids in hands_lib.COUPLED_JOINT_IDS]  # shadow_hand_e.py:124-129
        self.hand_names = (self.hand_name,)
        self.tip_sites = [names["site"].index(t) for t in tips]
        self.coupled = coupled
        self.hand_nq = cm.nq
        self.hand_nv = cm.nv
        self.ntips = len(self.tip_sites)
        self.actuator_ids = list(range(cm.nu))
        self.hand_effector = effectors_lib.HandEffector(self.actuator_ids, self.hand_name)
        # FingertipCartesianPosition.initialize_episode (fingertip_position.py:55-62)
        self.gravity_compensation = physics_lib.gravity_compensation(cm, self.hand_name + "/")
        rng = np.asarray(cm.arrays["jnt_range"], dtype=np.float64).reshape(-1, 2)[: cm.nq]
        self.joint_range = rng

    def params(self) -> np.ndarray:
        c, cm = self.config, self.compiled
        head = np.zeros(_lib.REACH_NPARAMS_HEAD, dtype=np.float32)
        head[0] = c.n_sub_steps
        head[1], head[2], head[3] = self.hand_nq, self.hand_nv, self.ntips
        head[4:4 + self.ntips] = self.tip_sites
        head[9], head[10] = c.successes_needed, c.steps_before_moving_target
        head[11], head[12] = c.success_threshold, c.max_time_per_goal
        head[13] = 1.0 if c.dense_reward else 0.0
        head[14], head[15], head[16] = c.init_joint_range_fraction, c.goal_scale, c.max_rejection_samples
        head[17] = len(self.coupled)
        for k, (j, src) in enumerate(self.coupled):
            head[18 + 2 * k], head[19 + 2 * k] = j, src
        lo, hi = self.joint_range[:, 0], self.joint_range[:, 1]
        mid = self.joint_range.mean(axis=1)  # fingertip_position.py:80-82
        tail = np.concatenate([mid, lo, hi, np.asarray(self.position_to_control, dtype=np.float64).ravel()])
        assert tail.size == 3 * cm.nq + cm.nu * cm.nq
        # fp64 draw constants, as the reference computes them (raw bits): the goal's
        # normal(loc=midrange, scale=0.1 * range) and clip (fingertip_position.py:67-86),
        # the initial joints' uniform(range_fraction * limits) (dexterous_hand.py:137-142)
        f64 = np.concatenate([mid, c.goal_scale * (hi - lo), lo, hi, c.init_joint_range_fraction * lo,
                              c.init_joint_range_fraction * hi]).astype(np.float64)
        return np.concatenate([head, tail.astype(np.float32), f64.view(np.float32)])

    def observation_layout(self):
        return observation_layout(self.hand_nq, self.hand_nv, self.ntips, False, self.hand_name, 3 * self.ntips)


class GoalEnvironment:
    """Batched `GoalEnvironment` (environment.py:9-34) over `num_envs` environments.

    `step(action)` accepts a host array [num_envs, nu] or, with `device_action=True`,
    the integer address of a device buffer; outputs stay on the device unless read
    through `timestep()` / `observation()`.
    """

    def __init__(self, task: ReOrient, num_envs: int, seed: Optional[int] = None, device: int = 0,
                 time_limit: Optional[float] = None, strip_singleton_obs_buffer_dim: bool = True,
                 env_offset: int = 0):
        self.task = task
        self.num_envs = int(num_envs)
        # this batch's env e is env env_offset + e of the job (a shard of a sharded
        # job, dexterity_amd.distributed.env_shard); it draws from seed + env_offset + e
        self.env_offset = int(env_offset)
        # composer.Environment(time_limit=..., strip_singleton_obs_buffer_dim=...)
        # (manipulation/__init__.py:81-86): `time_limit or task.time_limit`, so None and 0
        # both mean the task's own limit, inf for every suite task
        self.time_limit = float(time_limit) if time_limit else float("inf")
        self.strip_singleton_obs_buffer_dim = bool(strip_singleton_obs_buffer_dim)
        self.model = physics_lib.Model(task.compiled)
        L = _lib.load()
        p = task.params()
        self._seed = 0 if seed is None else int(seed)
        self.ptr = L.dx_env_create_shard(self.model.ptr, self.num_envs, device, task.kind,
                                         self._seed, self.env_offset, p.ctypes.data, len(p))
        if not self.ptr:
            raise _lib.DxError(f"dx_env_create_shard failed: {L.dx_last_error().decode()}")
        batch_ptr = L.dx_env_batch(self.ptr)
        self.physics = physics_lib.BatchedPhysics.borrowed(self.model, batch_ptr, self.num_envs, device)
        # gravity compensation (shadow_hand_e.py:35-41 in initialize_episode)
        self.physics.set_xfrc(task.gravity_compensation)
        self.obs_dim = _lib.check(L.dx_env_obs_dim(self.ptr))
        self.goal_dim = _lib.check(L.dx_env_goal_dim(self.ptr))
        self._layout = task.observation_layout()
        self._action_spec = task.hand_effector.action_spec(self.physics)
        self._host_action = np.zeros((self.num_envs, self.model.nu), dtype=np.float32)
        self._dev_action = self._out(-1)
        self._pins = []  # page-locked host buffers of step() (freed by close)
        self._pin_act = self._pin_out = None
        # configure_actions' current arguments (the action pipeline is off by default)
        self.action_config = dict(noise_scale=None, noise_seed=None, smooth_alpha=None, previous_action=False)
        # enable_observables' current names, the row width and the named slices of a row
        self.hand_observables = ()
        self.hand_obs_dim = 0
        self._hand_layout = collections.OrderedDict()
        # configure_observations' current settings (None: the observation pipeline is off)
        self.observation_config = None
        self._obs_pipe = None  # (row width W, delivered rows per env, aggregated)
        # enable_contact_forces: the pads of DX_OUT_CONTACT_FORCE (0: off)
        self.contact_force_pads = 0
        # configure_perturbations' current settings (None: the random pushes are off)
        self.perturbation_options = None
        # enable_cameras' current settings (None: the cameras are off)
        self.camera_options = None
        if np.isfinite(self.time_limit):
            _lib.check(L.dx_env_set_time_limit(self.ptr, self.time_limit))
        # max_time_per_goal in fp64 (the params carry it as a float)
        _lib.check(L.dx_env_set_goal_time_limit(self.ptr, float(task.config.max_time_per_goal)))

    def close(self):
        for p in getattr(self, "_pins", ()):
            _hip_runtime().hipHostFree(ctypes.c_void_p(p))
        self._pins = []
        self._pin_act = self._pin_out = None
        if getattr(self, "physics", None) is not None:
            self.physics.ptr = None
        if getattr(self, "ptr", None) and _lib._lib is not None:
            _lib._lib.dx_env_destroy(self.ptr)
        self.ptr = None

    def __del__(self):
        self.close()

    def _out(self, which: int) -> int:
        p = ctypes.c_void_p()
        L = _lib.load()
        if which < 0:
            _lib.check(L.dx_env_action_buffer(self.ptr, ctypes.byref(p)))
        else:
            _lib.check(L.dx_env_output(self.ptr, which, ctypes.byref(p)))
        return p.value

    # ---------------------------------------------------------------- specs
    def action_spec(self) -> BoundedArray:
        return self._action_spec

    def observation_spec(self) -> "collections.OrderedDict[str, Array]":
        lead = () if self.strip_singleton_obs_buffer_dim else (1,)
        if self._obs_pipe is not None:  # composer: (buffer_size, n), no buffer axis behind an aggregator
            _, rows, aggregated = self._obs_pipe
            lead = () if aggregated or (rows == 1 and self.strip_singleton_obs_buffer_dim) else (rows,)
        spec = collections.OrderedDict(
            (k, Array(lead + (s.stop - s.start,), np.float64, name=k))
            for k, s in list(self._layout.items()) + list(self._hand_layout.items())
        )
        if self.contact_force_pads:  # (never buffered: the observation pipeline's row does not carry them)
            lead = () if self.strip_singleton_obs_buffer_dim else (1,)
            spec[CONTACT_FORCES_KEY] = Array(lead + (self.contact_force_pads, 3), np.float64, name=CONTACT_FORCES_KEY)
        if self.camera_options:  # (never buffered either)
            o = self.camera_options
            for name in o["names"]:
                if o["depth"]:
                    spec[f"{name}_depth"] = Array((o["height"], o["width"], 1), np.float32, name=f"{name}_depth")
                if o["segmentation"]:
                    spec[f"{name}_segmentation"] = Array((o["height"], o["width"], 2), np.int32,
                                                         name=f"{name}_segmentation")
                if o.get("rgb"):
                    spec[f"{name}_rgb"] = BoundedArray((o["height"], o["width"], 3), np.uint8, 0, 255, name=f"{name}_rgb")
        return spec

    # ---------------------------------------------------------------- stepping
    def reset(self) -> TimeStep:
        _lib.check(_lib.load().dx_env_reset(self.ptr))
        return self.timestep(first=True)

    def _hand_observation(self) -> "collections.OrderedDict[str, np.ndarray]":
        """The enabled optional hand observables (one device-to-host copy of
        DX_OUT_HAND_OBS); empty, and no copy, while none is enabled."""
        out = collections.OrderedDict()
        if self.hand_obs_dim:
            rows = self.hand_obs()
            for k, s in self._hand_layout.items():
                out[k] = (rows[:, s] if self.strip_singleton_obs_buffer_dim else rows[:, None, s]).astype(np.float64)
        return out

    def _contact_observation(self) -> "collections.OrderedDict[str, np.ndarray]":
        """`hand_contact_forces` while enable_contact_forces is on (one device-to-host copy of
        DX_OUT_CONTACT_FORCE); empty, and no copy, while it is off."""
        out = collections.OrderedDict()
        if self.contact_force_pads:
            rows = self.contact_forces().astype(np.float64)
            out[CONTACT_FORCES_KEY] = rows if self.strip_singleton_obs_buffer_dim else rows[:, None]
        return out

    def step(self, action, device_action: bool = False) -> Optional[TimeStep]:
        L = _lib.load()
        if device_action:
            _lib.check(L.dx_env_step(self.ptr, ctypes.c_void_p(int(action))))
            return None
        a = np.asarray(action, dtype=np.float32).reshape(self.num_envs, -1)
        if a.shape[1] != self.model.nu:
            raise ValueError(f"action must be [{self.num_envs}, {self.model.nu}], got {a.shape}")
        # the reference's call shape (environment.py:25-34): host actions in, the host
        # TimeStep out, through page-locked buffers -- dx_env_step_host uploads them into
        # the library's action buffer (the step kernel writes ctrl from it:
        # mujoco_actuation.py:33), steps, packs [obs | reward | discount | step_type] and
        # downloads it, all on the env's stream with one synchronisation
        if self._pin_act is None:
            self._pin_act = _pinned((self.num_envs, self.model.nu), np.float32, self._pins)
            self._pin_out = _pinned((self.num_envs, self.obs_dim + 3), np.float32, self._pins)
        np.copyto(self._pin_act, a)
        _lib.check(L.dx_env_step_host(self.ptr, self._pin_act.ctypes.data, self._pin_out.ctypes.data))
        ts = self._timestep_packed(self._pin_out)
        if self._obs_pipe is not None:  # the packed row keeps the raw observation: one more copy
            ts = ts._replace(observation=self._pipeline_observation())
        elif self.hand_obs_dim:  # the packed row does not carry them: one more copy
            ts.observation.update(self._hand_observation())
        ts.observation.update(self._contact_observation())
        ts.observation.update(self._camera_observation())
        return ts

    def _timestep_packed(self, packed: np.ndarray) -> TimeStep:
        """A TimeStep (copies) from the packed [obs | reward | discount | step_type] rows."""
        d = self.obs_dim
        observation = collections.OrderedDict(
            (k, packed[:, s].astype(np.float64) if self.strip_singleton_obs_buffer_dim
             else packed[:, None, s].astype(np.float64)) for k, s in self._layout.items()
        )
        return TimeStep(packed[:, d + 2].astype(np.int32), packed[:, d].astype(np.float64),
                        packed[:, d + 1].astype(np.float64), observation)

    def step_random(self, step: int) -> None:
        """One control step under the random agent: the actions `sample_actions(step)`
        would draw (manipulation_test.py:44-45), drawn inside the step kernel."""
        _lib.check(_lib.load().dx_env_step_random(self.ptr, self._seed, step))

    def sample_actions(self, step: int) -> int:
        """Fills the device action buffer with uniform actions; returns its address."""
        _lib.check(_lib.load().dx_env_sample_actions(self.ptr, self._seed, step))
        return self._dev_action

    # ---------------------------------------------------------------- action pipeline
    def configure_actions(self, noise_scale: Optional[float] = None, noise_seed: Optional[int] = None,
                          smooth_alpha: Optional[float] = None, previous_action: bool = False) -> None:
        """The reference's action-side wrappers on the device, ahead of every control step
        (include/dx.h dx_env_set_action_filter; `dexterity_amd.wrappers` has their names):
        `noise_scale` -- ActionNoise, clipped Gaussian noise of stddev noise_scale * (max -
        min), env e drawing from RandomState(noise_seed + env_offset + e), `noise_seed`
        defaulting to the env's seed; `smooth_alpha` -- SmoothAction's exponential moving
        average; `previous_action` -- PreviousAction (kept whenever a stage is on).  All
        None / False switches the pipeline off.  A checkpoint carries the pipeline's state
        but not these settings: load it into an env configured the same way."""
        f = _lib.ActionFilter()
        if noise_scale is not None:
            f.flags |= _lib.ACT_NOISE
            f.noise_scale = float(noise_scale)
            f.noise_seed = int(self._seed if noise_seed is None else noise_seed) & (2**64 - 1)
        if smooth_alpha is not None:
            f.flags |= _lib.ACT_SMOOTH
            f.smooth_alpha = float(smooth_alpha)
        if previous_action:
            f.flags |= _lib.ACT_PREVIOUS
        _lib.check(_lib.load().dx_env_set_action_filter(self.ptr, ctypes.byref(f)))
        self.action_config = dict(noise_scale=noise_scale, noise_seed=noise_seed, smooth_alpha=smooth_alpha,
                                  previous_action=bool(previous_action))

    @property
    def previous_action_ptr(self) -> int:
        """Device address of the [num_envs, nu] float32 previous action."""
        return self._out(_lib.OUT_PREV_ACTION)

    def previous_action(self) -> np.ndarray:
        """PreviousAction.previous_action of every env (host copy): the last command,
        after the noise and before the smoothing; zeros at the start of an episode."""
        return self._read(_lib.OUT_PREV_ACTION, np.float32, self.model.nu)

    # ---------------------------------------------------------------- hand observables
    def enable_observables(self, names) -> None:
        """The reference's `hand.observables.<name>.enabled = True` for the observables the
        fixed observation does not carry (HAND_EXTRA_OBSERVABLES: joint_positions,
        fingertip_orientations, fingertip_angular_velocities, fingertip_positions_ego),
        computed on the device behind every control step (include/dx.h
        dx_env_set_hand_observables).  `names` is the whole set to have on; an empty one
        switches the feature off.  They arrive as `f"{hand}/{name}"` after the existing
        keys of `observation_spec()` and of every TimeStep, and describe the same state
        as the rest of the observation -- also right after this call, before or after
        `reset`.  A checkpoint carries their values but not this setting."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in HAND_EXTRA_OBSERVABLES]
        if unknown:
            raise ValueError(f"unknown hand observables {unknown}; the optional ones are "
                             f"{list(HAND_EXTRA_OBSERVABLES)}")
        L = _lib.load()
        hands = self.task.hand_names
        cfg = _lib.HandObs()
        cfg.nhands = len(hands)
        for name in names:
            cfg.mask |= HAND_EXTRA_OBSERVABLES[name][0]
        bodies = self.task.compiled.names["body"]
        for h, hand in enumerate(hands):
            cfg.root_body[h] = bodies.index(f"{hand}/{HAND_ROOT_BODY}")
        _lib.check(L.dx_env_set_hand_observables(self.ptr, ctypes.byref(cfg)))
        enabled = tuple(n for n in HAND_EXTRA_OBSERVABLES if n in names)
        nq, nt = self.task.hand_nq // len(hands), self.task.ntips // len(hands)
        layout, k = collections.OrderedDict(), 0
        for hand in hands:
            for n in enabled:
                _, per_joint, per_tip = HAND_EXTRA_OBSERVABLES[n]
                w = per_joint * nq + per_tip * nt
                layout[f"{hand}/{n}"] = slice(k, k + w)
                k += w
        self.hand_obs_dim = _lib.check(L.dx_env_hand_obs_dim(self.ptr))
        assert self.hand_obs_dim == k, (self.hand_obs_dim, k)
        self.hand_observables = enabled
        self._hand_layout = layout

    @property
    def hand_obs_ptr(self) -> int:
        """Device address of the [num_envs, hand_obs_dim] float32 rows (while enabled)."""
        return self._out(_lib.OUT_HAND_OBS)

    def hand_obs(self) -> np.ndarray:
        """[num_envs, hand_obs_dim] float32 host copy of the rows (DxError while off)."""
        return self._read(_lib.OUT_HAND_OBS, np.float32, self.hand_obs_dim)

    # ---------------------------------------------------------------- contact forces
    def enable_contact_forces(self, enable: bool = True) -> None:
        """Tactile force between the hands and the prop, on the device behind every control
        step (include/dx.h dx_env_set_contact_forces): for every hand body that can collide
        with the prop (`contact_force_bodies`; 23 per Shadow hand) the force the prop's
        contacts exert on it, in that body's frame.  It arrives as `hand_contact_forces`,
        [B, npad, 3], after the other keys of `observation_spec()` and of every TimeStep: the
        last physics step's forces on MID and LAST steps, zeros on FIRST ones and until the
        first step after enabling.  A checkpoint carries the rows but not this setting.  The
        reach tasks have no prop: ValueError."""
        if self.task.kind == _lib.TASK_REACH:
            raise ValueError("contact forces need a prop: the reach tasks have none")
        L = _lib.load()
        _lib.check(L.dx_env_set_contact_forces(self.ptr, int(bool(enable))))
        dim = _lib.check(L.dx_env_contact_force_dim(self.ptr))
        assert dim % 3 == 0 and (dim > 0) == bool(enable), dim
        self.contact_force_pads = dim // 3

    @property
    def contact_force_bodies(self):
        """Names of the pads' bodies, in the order of the rows of `contact_forces()`."""
        if self.task.kind == _lib.TASK_REACH:
            raise ValueError("contact forces need a prop: the reach tasks have none")
        L = _lib.load()
        ids = (ctypes.c_int32 * _lib.MAX_PADS)()
        n = _lib.check(L.dx_env_contact_force_bodies(self.ptr, ids, _lib.MAX_PADS))
        names = self.task.compiled.names["body"]
        return [names[i] for i in list(ids)[:n]]

    @property
    def contact_force_ptr(self) -> int:
        """Device address of the [num_envs, npad, 3] float32 forces (while enabled)."""
        return self._out(_lib.OUT_CONTACT_FORCE)

    def contact_forces(self) -> np.ndarray:
        """[num_envs, npad, 3] float32 host copy of DX_OUT_CONTACT_FORCE (DxError while off)."""
        if not self.contact_force_pads:
            raise _lib.DxError("contact forces are off (enable_contact_forces)")
        n = self.contact_force_pads
        return self._read(_lib.OUT_CONTACT_FORCE, np.float32, 3 * n).reshape(self.num_envs, n, 3)

    # ---------------------------------------------------------------- cameras
    def enable_cameras(self, configs_or_names, height: int = 84, width: int = 84, depth: bool = True,
                       segmentation: bool = False, near: float = 0.01, far: float = 10.0, rgb: bool = False,
                       shading: Optional[dict] = None) -> None:
        """The reference's camera observables (manipulation/shared/cameras.py:53-64 at the
        84 x 84 spec of observations.py:62-74) as depth and segmentation images, ray cast on
        the device behind every control step (include/dx.h dx_env_set_cameras).  Cameras are
        `dexterity_amd.cameras.CameraConfig`s or names of its five (`front_close`, ...); an
        empty list switches the feature off.  Per camera, after the existing keys of
        `observation_spec()` and of every TimeStep:
          f"{name}_depth"         [B, H, W, 1] float32, metres along the optical axis, `far`
                                  where nothing is seen (dm_control's depth=True);
          f"{name}_segmentation"  [B, H, W, 2] int32, (geom id, 5 = mjOBJ_GEOM), or (-1, -1)
                                  where nothing is seen (dm_control's segmentation=True);
          f"{name}_rgb"           [B, H, W, 3] uint8 (`rgb=True`: dm_control's default camera
                                  output), shaded by the model include/dx.h states under
                                  "Shaded RGB" -- flat per hull facet, no textures, colours a
                                  runtime input.  `shading` holds `set_shading`'s keywords
                                  (geom_rgb, box_faces, lights, shading); None keeps the
                                  settings in force, the defaults at first.
        They describe the same state as the rest of the observation, also for an env that
        returned FIRST, and right after this call.  Only the compiled (collision) geoms
        exist.  The packed rows, the observation pipeline and the checkpoint do not carry
        the images.  Bad options raise ValueError."""
        cfgs = cameras_lib.resolve(configs_or_names)
        if not cfgs:
            _lib.check(_lib.load().dx_env_set_cameras(self.ptr, None, 0, 0, 0, 0))
            self.camera_options = None
            self.physics._cameras = ()
            return
        bodies = cameras_lib.validate(cfgs, width, height, depth, segmentation, near, far, self.num_envs,
                                      self.task.compiled.names["body"], rgb=rgb)
        if rgb and (shading is not None or not getattr(self, "_shading_set", False)):
            self.set_shading(**(shading or {}))
        arr = (_lib.Camera * len(cfgs))()
        for c, cfg, body in zip(arr, cfgs, bodies):
            c.pos[:] = [float(v) for v in cfg.pos]
            c.xyaxes[:] = [float(v) for v in cfg.xyaxes]
            c.fovy, c.near_, c.far_, c.body = float(cfg.fovy), float(near), float(far), body
        flags = (_lib.RENDER_DEPTH if depth else 0) | (_lib.RENDER_SEGMENTATION if segmentation else 0) | \
            (_lib.RENDER_RGB if rgb else 0)
        _lib.check(_lib.load().dx_env_set_cameras(self.ptr, arr, len(cfgs), int(width), int(height), flags))
        self.camera_options = dict(names=tuple(c.name for c in cfgs), configs=tuple(cfgs), height=int(height),
                                   width=int(width), depth=bool(depth), segmentation=bool(segmentation),
                                   near=float(near), far=float(far), rgb=bool(rgb))
        # (the borrowed batch handle's host copies -- physics.rgb() -- read the same images)
        self.physics._cameras = tuple(cfgs)
        self.physics._camera_shape = (self.num_envs, len(cfgs), int(height), int(width))

    def set_shading(self, geom_rgb=None, box_faces=None, lights=None, shading=None) -> None:
        """The shading settings of the RGB images (`BatchedPhysics.set_shading`'s arguments;
        include/dx.h dx_env_set_shading).  They persist across `enable_cameras`; images that
        are on are rendered afresh.  Bad settings raise ValueError before any library call."""
        cm = self.task.compiled
        if geom_rgb is None and box_faces is None:
            geom_rgb, box_faces = cameras_lib.default_palette(cm)
        elif geom_rgb is None:
            geom_rgb = cameras_lib.default_palette(cm)[0]
        elif box_faces is None:
            box_faces = {}
        parts = cameras_lib.validate_shading(geom_rgb, box_faces, cameras_lib.DEFAULT_LIGHTS if lights is None else lights,
                                             cameras_lib.DEFAULT_SHADING if shading is None else shading,
                                             np.asarray(cm.geom_type))
        args, keep = _lib.shading_args(*parts)
        _lib.check(_lib.load().dx_env_set_shading(self.ptr, *args))
        del keep
        self._shading_set = True

    def rgb_ptr(self) -> int:
        """Device address of the [num_envs, ncam, H, W, 3] uint8 RGB images (while enabled)."""
        return self._out(_lib.OUT_RGB)

    def depth_ptr(self) -> int:
        """Device address of the [num_envs, ncam, H, W] float32 depth images (while enabled)."""
        return self._out(_lib.OUT_DEPTH)

    def segmentation_ptr(self) -> int:
        """Device address of the [num_envs, ncam, H, W] int32 geom ids (while enabled)."""
        return self._out(_lib.OUT_SEGMENTATION)

    def _camera_observation(self) -> "collections.OrderedDict[str, np.ndarray]":
        """The cameras' images while enable_cameras is on (one device-to-host copy per
        enabled output); empty, and no copy, while it is off."""
        out = collections.OrderedDict()
        o = self.camera_options
        if not o:
            return out
        n = len(o["names"]) * o["height"] * o["width"]
        shape = (self.num_envs, len(o["names"]), o["height"], o["width"])
        dep = self._read(_lib.OUT_DEPTH, np.float32, n).reshape(shape) if o["depth"] else None
        seg = self._read(_lib.OUT_SEGMENTATION, np.int32, n).reshape(shape) if o["segmentation"] else None
        rgb = self._read(_lib.OUT_RGB, np.uint8, 3 * n).reshape(shape + (3,)) if o.get("rgb") else None
        for k, name in enumerate(o["names"]):
            if dep is not None:
                out[f"{name}_depth"] = dep[:, k, :, :, None].copy()
            if seg is not None:
                s = seg[:, k]
                out[f"{name}_segmentation"] = np.stack([s, np.where(s >= 0, cameras_lib.OBJ_GEOM, -1)],
                                                       axis=-1).astype(np.int32)
            if rgb is not None:
                out[f"{name}_rgb"] = rgb[:, k].copy()
        return out

    # ---------------------------------------------------------------- random pushes
    def configure_perturbations(self, bodies=("prop",), probability: float = 0.0, force_range=(0.0, 0.0),
                                torque_range=(0.0, 0.0), duration_steps: int = 1, seed: Optional[int] = None) -> None:
        """Random pushes on the device, ahead of every control step (include/dx.h
        dx_env_set_perturbation): each of `bodies` (1 to 4 body names; "prop" is the task's
        prop) starts a push with `probability` per control step while it holds none -- a force
        of magnitude uniform in `force_range` (N) and a torque uniform in `torque_range` (N m),
        both uniformly directed, world frame at the body's com -- and holds it for
        `duration_steps` control steps.  Env e draws from RandomState(seed + env_offset + e),
        `seed` defaulting to the env's.  `bodies=None` switches the feature off.  The pushes
        are added to the gravity compensation in the env's own xfrc_applied rows;
        `applied_perturbations()` reads them back.  A checkpoint carries the held pushes and
        the streams but not these settings: load it into an env configured the same way.
        The reach tasks refuse (ValueError)."""
        L = _lib.load() if bodies is None else None
        if bodies is None:
            _lib.check(L.dx_env_set_perturbation(self.ptr, None))
            self.perturbation_options = None
            return
        opt = perturbation_settings(self.task, bodies, probability, force_range, torque_range, duration_steps,
                                    self._seed if seed is None else seed)
        p = _lib.Perturbation()
        p.nbody = len(opt["body_ids"])
        for k, b in enumerate(opt["body_ids"]):
            p.bodies[k] = b
        p.probability = opt["probability"]
        p.force_min, p.force_max = opt["force_range"]
        p.torque_min, p.torque_max = opt["torque_range"]
        p.duration = opt["duration_steps"]
        p.seed = opt["seed"] & (2**64 - 1)
        _lib.check(_lib.load().dx_env_set_perturbation(self.ptr, ctypes.byref(p)))
        self.perturbation_options = opt

    def applied_perturbations_ptr(self) -> int:
        """Device address of the [num_envs, nb, 6] float32 pushes (while configured)."""
        return self._out(_lib.OUT_PERTURB)

    def applied_perturbations(self) -> np.ndarray:
        """[num_envs, nb, 6] float32 host copy of DX_OUT_PERTURB: per configured body the
        (force, torque) the last control step applied on top of the gravity compensation;
        zeros on FIRST steps and after `reset` (DxError while off)."""
        if self.perturbation_options is None:
            raise _lib.DxError("perturbations are off (configure_perturbations)")
        nb = len(self.perturbation_options["body_ids"])
        return self._read(_lib.OUT_PERTURB, np.float32, 6 * nb).reshape(self.num_envs, nb, 6)

    # ---------------------------------------------------------------- observation pipeline
    def _row_layout(self) -> "collections.OrderedDict[str, slice]":
        """Named slices of the pipeline's row: the observation, then the hand observables."""
        out = collections.OrderedDict(self._layout)
        for k, s in self._hand_layout.items():
            out[k] = slice(self.obs_dim + s.start, self.obs_dim + s.stop)
        return out

    def configure_observations(self, update_interval: Optional[int] = None, buffer_size: int = 1, delay: int = 0,
                               aggregator: Optional[str] = None, padding: str = "zero", noise_std=None,
                               noise_seed: Optional[int] = None) -> None:
        """Composer's observable options on the device, behind every control step (include/dx.h
        dx_env_set_obs_pipeline): `update_interval` and `delay` in PHYSICS steps as composer
        counts them (multiples of the task's n_sub_steps; `obs_pipeline_options` has the
        rule), `buffer_size`, `aggregator` (None, "min", "max", "mean", "median", "sum"),
        `padding` ("zero" or "initial_value": composer's delayed_observation_padding) and
        `noise_std`, additive Gaussian noise per sample (a float, an array over the row, or a
        dict by observable name), env e drawing from RandomState(noise_seed + env_offset + e),
        `noise_seed` defaulting to the env's seed.  One option set covers every observable,
        the enabled hand observables included -- enable those first: the library refuses to
        change them while the pipeline is on.  Every TimeStep's observation[name] is then
        [B, buffer_size, n], or [B, n] with an aggregator or with buffer_size 1 under
        strip_singleton_obs_buffer_dim, and `observation_spec()` says the same.  Calling this
        starts every env's history afresh from its current observation; with all defaults
        it switches the pipeline off.  A checkpoint carries the pipeline's state but not
        these settings: load it into an env configured the same way."""
        L = _lib.load()
        args = dict(update_interval=update_interval, buffer_size=buffer_size, delay=delay, aggregator=aggregator,
                    padding=padding, noise_std=noise_std)
        layout = self._row_layout()
        m, d, K, agg, pad, sigma = obs_pipeline_options(self.task.config.n_sub_steps, widths=layout, **args)
        if (update_interval is None and (m, d, K, agg) == (1, 0, 1, 0) and sigma is None
                and pad == _lib.OBS_PAD["zero"]):
            _lib.check(L.dx_env_set_obs_pipeline(self.ptr, None))
            self.observation_config = self._obs_pipe = None
            return
        p = _lib.ObsPipeline(update_interval=m, delay=d, buffer_size=K, aggregator=agg, padding=pad)
        if sigma is not None:
            sigma = np.ascontiguousarray(sigma, dtype=np.float64)
            p.noise = 1
            p.noise_seed = int(self._seed if noise_seed is None else noise_seed) & (2**64 - 1)
            p.noise_sigma = sigma.ctypes.data
            p.nsigma = sigma.size
        _lib.check(L.dx_env_set_obs_pipeline(self.ptr, ctypes.byref(p)))
        dims = (ctypes.c_int32 * 3)()
        _lib.check(L.dx_env_obs_pipe_dims(self.ptr, dims))
        assert dims[0] == self.obs_dim + self.hand_obs_dim and dims[2] == 1, list(dims)
        self._obs_pipe = (int(dims[0]), int(dims[1]), agg != 0)
        self.observation_config = dict(args, noise_seed=noise_seed)

    def obs_buffer_ptr(self) -> int:
        """Device address of DX_OUT_OBS_BUFFER: [num_envs, buffer_size, W] float32 oldest first,
        [num_envs, W] with an aggregator (DxError while the pipeline is off)."""
        return self._out(_lib.OUT_OBS_BUFFER)

    def obs_buffer(self) -> np.ndarray:
        """[num_envs, rows, W] float32 host copy of DX_OUT_OBS_BUFFER (rows = 1 with an aggregator)."""
        if self._obs_pipe is None:
            raise _lib.DxError("the observation pipeline is off (configure_observations)")
        W, rows, _ = self._obs_pipe
        return self._read(_lib.OUT_OBS_BUFFER, np.float32, rows * W).reshape(self.num_envs, rows, W)

    def _pipeline_observation(self) -> "collections.OrderedDict[str, np.ndarray]":
        _, rows, aggregated = self._obs_pipe
        buf = self.obs_buffer()
        flat = aggregated or (rows == 1 and self.strip_singleton_obs_buffer_dim)
        return collections.OrderedDict(
            (k, (buf[:, 0, s] if flat else buf[:, :, s]).astype(np.float64)) for k, s in self._row_layout().items())

    # ---------------------------------------------------------------- checkpoint
    # dtype of the state fields that are not float32 (include/dx.h dx_env_save)
    _STATE_DTYPES = {"nstep": np.int32, "diverged": np.int32, "successes": np.int32, "counter": np.int32,
                     "registered": np.int32, "exceeded": np.int32, "step_type": np.int32, "episode": np.int32,
                     "skip": np.int32, "failure": np.int32, "need": np.int32, "goalnum": np.int32,
                     "goalfail": np.int32, "time_d": np.float64, "solve_start_d": np.float64,
                     "nsub_d": np.int32, "solve_n": np.int32, "mt_env": np.uint32, "mt_goal": np.uint32,
                     "mt_reach": np.uint32, "step_cost": np.uint32, "order": np.int32,
                     "act_ema_set": np.int32, "mt_noise": np.uint32,
                     "obs_count": np.int32, "mt_obs_noise": np.uint32,
                     "perturb_remain": np.int32, "mt_perturb": np.uint32}

    def _state_fields(self):
        L = _lib.load()
        name, off, nb = ctypes.c_char_p(), ctypes.c_size_t(), ctypes.c_size_t()
        n = _lib.check(L.dx_env_state_field(self.ptr, -1, ctypes.byref(name), ctypes.byref(off), ctypes.byref(nb)))
        out = []
        for i in range(n):
            _lib.check(L.dx_env_state_field(self.ptr, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(nb)))
            out.append((name.value.decode(), off.value, nb.value))
        return out

    def save(self, path: str) -> None:
        """Checkpoint every env's state (physics, task, RNG streams, dispatch order) to an
        .npz of named [num_envs, ...] arrays (SURVEY.md §5 checkpoint / resume); `load`
        into an env of the same task and size continues the run bit for bit."""
        L = _lib.load()
        nbytes = _lib.check(L.dx_env_save(self.ptr, None, 0))
        buf = np.empty(nbytes, dtype=np.uint8)
        _lib.check(L.dx_env_save(self.ptr, buf.ctypes.data, nbytes))
        arrays = {}
        for name, off, nb in self._state_fields():
            a = buf[off:off + nb].view(self._STATE_DTYPES.get(name, np.float32))
            arrays[name] = a.reshape(self.num_envs, -1) if name not in ("mt_env", "mt_goal") else a.reshape(-1, self.num_envs)
        meta = np.array([self.num_envs, self.model.nq, self.model.nv, self.model.nu, self.obs_dim, self.env_offset],
                        dtype=np.int64)
        # the random agent's key (dx_env_step_random / sample_actions draw from it), so a
        # load into an env created with another seed continues the same action stream
        np.savez(path, __meta__=meta, __agent_seed__=np.array([self._seed], dtype=np.int64), **arrays)

    def load(self, path: str) -> None:
        """Restores a checkpoint written by `save` (same task, model and num_envs),
        including the random agent's key."""
        L = _lib.load()
        with np.load(path, allow_pickle=False) as z:
            meta = z["__meta__"]
            want = [self.num_envs, self.model.nq, self.model.nv, self.model.nu, self.obs_dim, self.env_offset]
            if list(meta) != want:
                raise ValueError(f"checkpoint is for (num_envs, nq, nv, nu, obs_dim, env_offset) = {list(meta)}, "
                                 f"this env is {want}")
            if "__agent_seed__" in z.files:
                self._seed = int(z["__agent_seed__"][0])
            fields = self._state_fields()
            # the action pipeline's state is in a checkpoint only while the pipeline is on,
            # and its settings are not: the env must be configured as the saved one was
            pipeline = {"act_ema", "act_ema_set", "prev_action", "mt_noise"}
            if (pipeline <= set(z.files)) != (pipeline <= {name for name, _, _ in fields}):
                raise ValueError("checkpoint and env differ in the action pipeline (on in one, off in the other): "
                                 "configure_actions as the saved env was, then load")
            if ("hand_obs" in z.files) != ("hand_obs" in {name for name, _, _ in fields}):
                raise ValueError("checkpoint and env differ in the hand observables (on in one, off in the other): "
                                 "enable_observables as the saved env did, then load")
            for key in ("obs_ring", "mt_obs_noise"):
                if (key in z.files) != (key in {name for name, _, _ in fields}):
                    raise ValueError("checkpoint and env differ in the observation pipeline (on in one, off in the "
                                     "other, or its noise): configure_observations as the saved env did, then load")
            if ("contact_force" in z.files) != ("contact_force" in {name for name, _, _ in fields}):
                raise ValueError("checkpoint and env differ in the contact forces (on in one, off in the other): "
                                 "enable_contact_forces as the saved env did, then load")
            if ("mt_perturb" in z.files) != ("mt_perturb" in {name for name, _, _ in fields}):
                raise ValueError("checkpoint and env differ in the perturbations (on in one, off in the other): "
                                 "configure_perturbations as the saved env was, then load")
            nbytes = sum(nb for _, _, nb in fields)
            buf = np.empty(nbytes, dtype=np.uint8)
            for name, off, nb in fields:
                a = np.ascontiguousarray(z[name])
                if a.nbytes != nb:
                    raise ValueError(f"checkpoint field {name}: {a.nbytes} bytes, expected {nb}")
                buf[off:off + nb] = a.view(np.uint8).ravel()
        self.physics.sync()
        _lib.check(L.dx_env_load(self.ptr, buf.ctypes.data, nbytes))

    def _read(self, which: int, dtype, width: int) -> np.ndarray:
        out = np.empty((self.num_envs, width), dtype=dtype)
        ptr = self._out(which)
        self.physics.sync()
        _copy_d2h(out, ptr)
        return out

    def timestep(self, first: bool = False) -> TimeStep:
        obs = self._read(_lib.OUT_OBS, np.float32, self.obs_dim)
        st = self._read(_lib.OUT_STEP_TYPE, np.int32, 1)[:, 0]
        rew = self._read(_lib.OUT_REWARD, np.float32, 1)[:, 0].astype(np.float64)
        disc = self._read(_lib.OUT_DISCOUNT, np.float32, 1)[:, 0].astype(np.float64)
        # an observation buffer of size 1 per observable (dm_control observation
        # updater); kept as [B, 1, n] unless strip_singleton_obs_buffer_dim
        observation = collections.OrderedDict(
            (k, obs[:, s].astype(np.float64) if self.strip_singleton_obs_buffer_dim
             else obs[:, None, s].astype(np.float64)) for k, s in self._layout.items()
        )
        if self._obs_pipe is not None:
            observation = self._pipeline_observation()
        else:
            observation.update(self._hand_observation())
        observation.update(self._contact_observation())
        observation.update(self._camera_observation())
        return TimeStep(st.astype(np.int32), rew, disc, observation)

    def goals(self) -> np.ndarray:
        return self._read(_lib.OUT_GOAL, np.float32, self.goal_dim)

    def goal_qpos(self) -> np.ndarray:
        """Reach: the joints that placed each env's goal (FingertipCartesianPosition.qpos,
        fingertip_position.py:136-139)."""
        return self._read(_lib.OUT_GOAL_QPOS, np.float32, self.model.nq)

    def goal_failures(self) -> np.ndarray:
        return self._read(_lib.OUT_GOAL_FAILURES, np.int32, 1)[:, 0]

    def successes(self) -> np.ndarray:
        return self._read(_lib.OUT_SUCCESSES, np.int32, 1)[:, 0]


def _hip_runtime():
    """The HIP runtime libdx is linked against (for plain host<->device copies)."""
    global _hip
    if _hip is None:
        try:
            _hip = ctypes.CDLL("libamdhip64.so.7")
        except OSError:
            _hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        _hip.hipFree.argtypes = [ctypes.c_void_p]
        _hip.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
        _hip.hipHostFree.argtypes = [ctypes.c_void_p]
    return _hip


def _pinned(shape, dtype, owner: list) -> np.ndarray:
    """A page-locked host array (hipHostMalloc); its address is appended to `owner`."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = ctypes.c_void_p()
    rc = _hip_runtime().hipHostMalloc(ctypes.byref(p), nbytes, 0)
    if rc != 0 or not p.value:
        raise _lib.DxError(f"hipHostMalloc failed ({rc})")
    owner.append(p.value)
    buf = (ctypes.c_byte * nbytes).from_address(p.value)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def _copy_d2h(out: np.ndarray, devptr: int) -> None:
    rc = _hip_runtime().hipMemcpy(out.ctypes.data, ctypes.c_void_p(devptr), out.nbytes, 2)  # DeviceToHost
    if rc != 0:
        raise _lib.DxError(f"hipMemcpy failed ({rc})")


def _copy_h2d(devptr: int, src: np.ndarray) -> None:
    rc = _hip_runtime().hipMemcpy(ctypes.c_void_p(devptr), src.ctypes.data, src.nbytes, 1)  # HostToDevice
    if rc != 0:
        raise _lib.DxError(f"hipMemcpy failed ({rc})")


_hip = None

SUITE = {
    ("reorient", "state_dense"): ReOrient,
    ("reach", "state_dense"): lambda: Reach(ReachConfig(dense_reward=True), hand="adroit"),
    ("reach", "state_sparse"): lambda: Reach(ReachConfig(dense_reward=False), hand="adroit"),
    ("reach_shadow", "state_dense"): lambda: Reach(ReachConfig(dense_reward=True), hand="shadow"),
    ("bimanual", "state_dense"): Handover,
}
ALL_TASKS = tuple(sorted(SUITE))
ALL_NAMES = [".".join(t) for t in ALL_TASKS]
# manipulation/__init__.py:53 (_get_tasks_by_domain)
TASKS_BY_DOMAIN = {d: tuple(t for dd, t in ALL_TASKS if dd == d) for d in sorted({d for d, _ in ALL_TASKS})}


def load(domain_name: str, task_name: str, seed: Optional[int] = None,
         strip_singleton_obs_buffer_dim: bool = True, time_limit: Optional[float] = None,
         num_envs: int = 1, device: int = 0, env_offset: int = 0, noise_scale: Optional[float] = None,
         noise_seed: Optional[int] = None, smooth_alpha: Optional[float] = None,
         previous_action: bool = False, cameras=None, camera_options: Optional[dict] = None) -> GoalEnvironment:
    """manipulation/__init__.py:56-86, batched: the reference's arguments in its order,
    then the batch size and the GPU.  `time_limit=None` keeps the task's own limit
    (inf for every suite task).  Env e of the batch is the reference's environment
    loaded with seed `seed + env_offset + e`; `env_offset` places a shard of a sharded
    job (distributed.env_shard) in the job's env numbering.  The last four arguments are
    `GoalEnvironment.configure_actions`' (default: the action pipeline off).  `cameras`
    (CameraConfigs or names) and `camera_options` (height, width, depth, segmentation, rgb,
    shading, near, far) are `GoalEnvironment.enable_cameras`' (default: no cameras)."""
    key = (domain_name, task_name)
    if domain_name not in {d for d, _ in SUITE}:
        raise ValueError(f"Unknown domain: {domain_name}")
    if key not in SUITE:
        raise ValueError(f"Unknown task: {task_name}")
    env = GoalEnvironment(SUITE[key](), num_envs=num_envs, seed=seed, device=device, time_limit=time_limit,
                          strip_singleton_obs_buffer_dim=strip_singleton_obs_buffer_dim, env_offset=env_offset)
    if noise_scale is not None or smooth_alpha is not None or previous_action:
        env.configure_actions(noise_scale=noise_scale, noise_seed=noise_seed, smooth_alpha=smooth_alpha,
                              previous_action=previous_action)
    if cameras:
        env.enable_cameras(cameras, **(camera_options or {}))
    return env


__all__ = ["load", "GoalEnvironment", "ReOrient", "ReOrientConfig", "Reach", "ReachConfig", "ALL_TASKS",
           "ALL_NAMES", "TASKS_BY_DOMAIN", "StepType", "HAND_EXTRA_OBSERVABLES", "obs_pipeline_options"]
