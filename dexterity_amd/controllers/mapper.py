"""Cartesian velocity to joint velocity mappers: the counterpart of
`dexterity/controllers/mapper.py` (the abstract mapper, :12-41, and its `Parameters`,
:44-81).

The reference names a controlled object by MuJoCo type and name and validates both
against the `MjModel`; here the model is a `physics.Model`, whose compiled scene carries
the name tables, and the types are MuJoCo's `mjtObj` values for bodies, geoms and sites
(`_lib.OBJ_BODY` / `OBJ_GEOM` / `OBJ_SITE`, include/dx.h `dx_obj_type`) or their names.
"""

from __future__ import annotations

import abc
import dataclasses
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from dexterity_amd import _lib, physics

ObjectType = Union[int, str]

# mapper.py:60-64: only bodies, geoms and sites are supported
_TYPE_NAMES = {_lib.OBJ_BODY: "body", _lib.OBJ_GEOM: "geom", _lib.OBJ_SITE: "site"}
_TYPE_CODES = {v: k for k, v in _TYPE_NAMES.items()}


def object_type_code(object_type: ObjectType) -> int:
    """The `dx_obj_type` of "body" / "geom" / "site" or of an `mjtObj` int; anything else
    (e.g. "joint", mjOBJ_JOINT = 3) raises ValueError (mapper.py:59-69)."""
    code = _TYPE_CODES.get(object_type) if isinstance(object_type, str) else object_type
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or int(code) not in _TYPE_NAMES:
        raise ValueError(
            f"Objects of type {object_type} are not supported. Only bodies, geoms and sites are supported.")
    return int(code)


class CartesianVelocitytoJointVelocityMapper(abc.ABC):
    """Abstract base class for a Cartesian velocity to joint velocity mapper
    (mapper.py:12-41).

    Subclasses implement `compute_joint_velocities`, which maps target Cartesian
    velocities of the controlled MuJoCo objects, expressed about each object's origin in
    world orientation, to joint velocities.  Where the reference takes an up-to-date
    `MjData`, this takes a `BatchedPhysics` whose qpos is current; kinematics are
    recomputed on the device.
    """

    @abc.abstractmethod
    def compute_joint_velocities(
        self,
        physics: "physics.BatchedPhysics",
        target_velocities: Sequence[np.ndarray],
        nullspace_bias: Optional[np.ndarray] = None,
    ) -> np.ndarray:
        """Maps the Cartesian target velocity to joint velocities."""


@dataclasses.dataclass(frozen=True)
class Parameters:
    """Container for `CartesianVelocitytoJointVelocityMapper` parameters (mapper.py:44-81)."""

    model: "physics.Model"
    """The scene, loaded into libdx (the reference's `MjModel`)."""

    object_types: Sequence[ObjectType]
    """Type of each controlled object: "body", "geom" or "site", or the `mjtObj` int."""

    object_names: Sequence[str]
    """Name of each controlled object, as in `model.compiled.names[type]`."""

    def __post_init__(self) -> None:
        self._validate_parameters()

    def _validate_parameters(self) -> None:
        # mapper.py:58-69
        codes = [object_type_code(t) for t in self.object_types]
        # mapper.py:71-81: name2id raises for a name of another type too
        names = self.model.compiled.names
        for object_name, code in zip(self.object_names, codes):
            kind = _TYPE_NAMES[code]
            if not object_name or object_name not in names[kind]:
                raise ValueError(
                    f"Could not find MuJoCo object with name {object_name} and type {kind} in the provided model.")

    def objects(self) -> Tuple[np.ndarray, np.ndarray]:
        """(types, ids) as the int32 arrays dx_jac_object / dx_dls_map take."""
        codes = [object_type_code(t) for t in self.object_types]
        names = self.model.compiled.names
        ids = [names[_TYPE_NAMES[c]].index(n) for c, n in zip(codes, self.object_names)]
        return np.asarray(codes, dtype=np.int32), np.asarray(ids, dtype=np.int32)

    def points(self) -> Tuple[np.ndarray, np.ndarray]:
        """The points the device controls (dx_dls.hip): (body id [nobj], offset in the body
        frame [nobj, 3]) -- (site_bodyid, site_pos) for a site (mj_jacSite), (geom_bodyid,
        geom_pos) for a geom (mj_jacGeom), (b, 0) for a body (mj_jacBody, at xpos)."""
        cm = self.model.compiled
        types, ids = self.objects()
        body = np.zeros(len(ids), np.int32)
        off = np.zeros((len(ids), 3))
        for k, (t, i) in enumerate(zip(types, ids)):
            if t == _lib.OBJ_SITE:
                body[k], off[k] = np.asarray(cm.site_bodyid).ravel()[i], np.asarray(cm.site_pos).reshape(-1, 3)[i]
            elif t == _lib.OBJ_GEOM:
                body[k], off[k] = np.asarray(cm.geom_bodyid).ravel()[i], np.asarray(cm.geom_pos).reshape(-1, 3)[i]
            else:
                body[k] = i
        return body, off
