"""Cartesian-to-joint velocity controllers: the counterpart of `dexterity/controllers/`
(controllers/__init__.py:1-9), batched over the environments of a `BatchedPhysics`."""

from dexterity_amd.controllers import dls
from dexterity_amd.controllers.mapper import CartesianVelocitytoJointVelocityMapper
from dexterity_amd.controllers.mapper import Parameters

__all__ = [
    "CartesianVelocitytoJointVelocityMapper",
    "Parameters",
    "dls",
]
