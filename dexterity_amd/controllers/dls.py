"""Damped-least-squares Cartesian-to-joint velocity mapper: the counterpart of
`dexterity/controllers/dls/dls.py` (DampedLeastSquaresParameters, :13-24, and
DampedLeastSquaresMapper, :27-77), run on the GPU for every environment of a batch.

`compute_joint_velocities` keeps the reference's call shape on a 1-env
`BatchedPhysics`; `compute_joint_velocities_batch` maps one target set per environment in
one `dx_dls_map` call (dexterity_amd/csrc/dx_dls.hip: one wavefront per env), with the
targets and the result in host or device memory.  There is no CPU fallback: without
libdx.so the calls raise DxError.
"""

from __future__ import annotations

import ctypes
import dataclasses
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from dexterity_amd import _lib
from dexterity_amd import physics as dx_physics
from dexterity_amd.controllers import mapper


@dataclasses.dataclass(frozen=True)
class DampedLeastSquaresParameters(mapper.Parameters):
    """dls.py:13-24."""

    regularization_weight: float
    """Damping factor used to regularize the pseudoinverse."""

    def _validate_parameters(self) -> None:
        super()._validate_parameters()

        # dls.py:20-24 (a NaN weight is refused too: the device would refuse it)
        if not self.regularization_weight >= 0 or not np.isfinite(self.regularization_weight):
            raise ValueError(
                f"`regularization_weight` must be non-negative, but was {self.regularization_weight}.")


def _address(a) -> int:
    return int(a.ctypes.data) if isinstance(a, np.ndarray) else int(a)


@dataclasses.dataclass(frozen=True)
class DampedLeastSquaresMapper(mapper.CartesianVelocitytoJointVelocityMapper):
    """A `CartesianVelocitytoJointVelocityMapper` that uses damped least-squares to solve
    for the joint velocities (dls.py:27-77): with J the stacked translational Jacobians of
    the controlled objects (the rotational halves are dropped, dls.py:62), V the stacked
    target velocities and lambda the regularization weight,

    `[J^T @ J + lambda I] @ v = J^T @ V`          (dls.py:69-74)

    which the device solves in its equivalent form `v = J^T @ [J @ J^T + lambda I]^-1 @ V`.
    With lambda = 0 (dls.py:75-77, np.linalg.lstsq) that is the minimum-norm solution for a
    J of full row rank; a numerically rank-deficient `J @ J^T + lambda I` is reported
    instead of solved (include/dx.h dx_dls_map, the rank guard).
    """

    params: DampedLeastSquaresParameters

    def compute_joint_velocities_batch(
        self,
        physics: "dx_physics.BatchedPhysics",
        targets: Union[np.ndarray, int],
        out: Union[np.ndarray, int, None] = None,
        status: Union[np.ndarray, int, None] = None,
    ) -> Tuple[Union[np.ndarray, int], Union[np.ndarray, int]]:
        """One target set per env at the env's current qpos.  `targets` is [B, nobj, 3]
        float32: a host array (anything else array-like is converted) or the address of
        device memory; `out` [B, nv] float32 and `status` [B] int32 likewise, allocated on
        the host when None.  Returns (out, status): status 0 ok, 1 rank-deficient (the row
        is zero).  With every array in device memory the call is only enqueued on the
        batch's stream; with a host array it has completed on return."""
        B, nv = physics.nenv, physics.model.nv
        types, ids = self.params.objects()
        if not isinstance(targets, (int, np.integer)):
            t = np.asarray(targets, dtype=np.float32)
            if t.size != B * len(ids) * 3:
                raise ValueError(
                    "The number of target velocities must be equal to the number of controlled objects.")
            targets = np.ascontiguousarray(t.reshape(B, len(ids), 3))
        if out is None:
            out = np.zeros((B, nv), np.float32)
        if status is None:
            status = np.zeros(B, np.int32)
        for a, shape, dt in ((out, (B, nv), np.float32), (status, (B,), np.int32)):
            if isinstance(a, np.ndarray) and (a.shape != shape or a.dtype != dt or not a.flags.c_contiguous):
                raise ValueError(f"expected a C-contiguous {np.dtype(dt).name} array of shape {shape}")
        _lib.check(_lib.load().dx_dls_map(
            physics.ptr, types.ctypes.data, ids.ctypes.data, len(ids),
            ctypes.c_float(self.params.regularization_weight), _address(targets), _address(out), _address(status)))
        return out, status

    def compute_joint_velocities(
        self,
        physics: "dx_physics.BatchedPhysics",
        target_velocities: Sequence[np.ndarray],
        nullspace_bias: Optional[np.ndarray] = None,
    ) -> np.ndarray:
        """dls.py:43-77 on a 1-env batch: `target_velocities` is one [3] linear velocity
        per controlled object; returns the joint velocities [nv], float64."""
        del nullspace_bias  # dls.py:49
        if physics.nenv != 1:
            raise ValueError("compute_joint_velocities maps one environment; use compute_joint_velocities_batch.")
        twist = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in target_velocities], axis=0)
        if twist.size != 3 * len(self.params.object_names):
            raise ValueError(
                "The number of target velocities must be equal to the number of controlled objects.")
        out, status = self.compute_joint_velocities_batch(physics, twist.reshape(1, -1, 3))
        if status[0] != 0:
            raise ValueError(
                "The Jacobian of the controlled objects is rank-deficient at this configuration: "
                "use regularization_weight > 0.")
        return out[0].astype(np.float64)
