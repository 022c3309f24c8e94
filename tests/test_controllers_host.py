"""dexterity_amd.controllers on the host (no GPU): parameter validation and the resolution
of controlled objects to points.

The reference's own tests pin (controllers/mapper_test.py:11-32, dls/dls_test.py:11-22):
  * an unsupported object type (mjOBJ_JOINT) with a valid name raises ValueError;
  * an unknown object name with a supported type raises ValueError;
  * a negative regularization weight raises ValueError.
They are restated against assets/shadow_reorient.npz, whose hand is the reference tests'
ShadowHandSeriesE.  Nothing here launches a kernel; the device half is tests/test_gpu_dls.py.
"""

import numpy as np
import pytest

from dexterity_amd import _lib, build


@pytest.fixture(scope="module")
def model(reorient_compiled):
    from dexterity_amd import physics

    build.build()
    return physics.Model(reorient_compiled)


_SITE = "shadow_hand_e/fftip_site"
_BODY = "shadow_hand_e/palm"
_GEOM = "prop/geom"


def test_negative_regularization_raises(model):
    """dls_test.py:11-22."""
    from dexterity_amd.controllers import dls

    with pytest.raises(ValueError):
        dls.DampedLeastSquaresParameters(model=model, regularization_weight=-1, object_types=(_lib.OBJ_SITE,),
                                         object_names=(_SITE,))
    with pytest.raises(ValueError):
        dls.DampedLeastSquaresParameters(model=model, regularization_weight=float("nan"), object_types=("site",),
                                         object_names=(_SITE,))
    # zero is the undamped case (dls.py:75-77), not an error
    p = dls.DampedLeastSquaresParameters(model=model, regularization_weight=0.0, object_types=("site",),
                                         object_names=(_SITE,))
    assert p.regularization_weight == 0.0


@pytest.mark.parametrize("bad_type", ["joint", 3, "tendon", 0, None, 6.5])
def test_unsupported_object_type_raises(model, bad_type):
    """mapper_test.py:11-20 (mjOBJ_JOINT = 3)."""
    from dexterity_amd.controllers import mapper

    with pytest.raises(ValueError):
        mapper.Parameters(model=model, object_types=(bad_type,), object_names=(_SITE,))


@pytest.mark.parametrize("object_type,name", [
    ("site", "nonexistent_site_name"),   # mapper_test.py:22-31
    ("body", _SITE),                     # a name of another type
    ("geom", ""),                        # unnamed geoms cannot be addressed by name
    (_lib.OBJ_SITE, "fftip_site"),       # the scene's names carry the hand's prefix
])
def test_unknown_object_name_raises(model, object_type, name):
    from dexterity_amd.controllers import mapper

    with pytest.raises(ValueError):
        mapper.Parameters(model=model, object_types=(object_type,), object_names=(name,))


def test_valid_triple_constructs_and_resolves_to_points(model):
    """A body / geom / site triple, by name and by mjtObj value; the points are the
    compiled arrays' (mj_jacBody at xpos, mj_jacGeom, mj_jacSite)."""
    from dexterity_amd.controllers import dls, mapper

    cm = model.compiled
    p = dls.DampedLeastSquaresParameters(model=model, object_types=("body", _lib.OBJ_GEOM, "site"),
                                         object_names=(_BODY, _GEOM, _SITE), regularization_weight=1e-5)
    assert isinstance(p, mapper.Parameters)
    types, ids = p.objects()
    assert types.dtype == np.int32 and ids.dtype == np.int32
    assert list(types) == [1, 5, 6]  # MuJoCo's mjOBJ_BODY, mjOBJ_GEOM, mjOBJ_SITE
    b, g, s = cm.names["body"].index(_BODY), cm.names["geom"].index(_GEOM), cm.names["site"].index(_SITE)
    assert list(ids) == [b, g, s]
    body, off = p.points()
    gb, gp = np.asarray(cm.geom_bodyid).ravel(), np.asarray(cm.geom_pos).reshape(-1, 3)
    sb, sp = np.asarray(cm.site_bodyid).ravel(), np.asarray(cm.site_pos).reshape(-1, 3)
    assert list(body) == [b, gb[g], sb[s]]
    np.testing.assert_array_equal(off[0], 0.0)
    np.testing.assert_array_equal(off[1], gp[g])
    np.testing.assert_array_equal(off[2], sp[s])
    assert body[1] == cm.names["body"].index("prop/") and body[2] == cm.names["body"].index("shadow_hand_e/fftip")


def test_offset_site_and_geom_points(adroit_compiled):
    """The Adroit hand's fingertip sites and collision geoms sit off their bodies' origins."""
    from dexterity_amd import physics
    from dexterity_amd.controllers import mapper

    cm = adroit_compiled
    p = mapper.Parameters(model=physics.Model(cm), object_types=("site", "geom"),
                          object_names=("adroit_hand/S_fftip", "adroit_hand/C_thdistal"))
    body, off = p.points()
    s, g = cm.names["site"].index("adroit_hand/S_fftip"), cm.names["geom"].index("adroit_hand/C_thdistal")
    assert cm.names["body"][body[0]] == "adroit_hand/ffdistal" and cm.names["body"][body[1]] == "adroit_hand/thdistal"
    np.testing.assert_array_equal(off[0], np.asarray(cm.site_pos).reshape(-1, 3)[s])
    np.testing.assert_array_equal(off[1], np.asarray(cm.geom_pos).reshape(-1, 3)[g])
    assert np.any(off[0] != 0.0) and np.any(off[1] != 0.0)


def test_mapper_is_abstract_and_dls_implements_it(model):
    from dexterity_amd.controllers import CartesianVelocitytoJointVelocityMapper, dls

    with pytest.raises(TypeError):
        CartesianVelocitytoJointVelocityMapper()
    p = dls.DampedLeastSquaresParameters(model=model, object_types=("site",), object_names=(_SITE,),
                                         regularization_weight=1e-2)
    m = dls.DampedLeastSquaresMapper(p)
    assert isinstance(m, CartesianVelocitytoJointVelocityMapper) and m.params is p


def test_null_batch_is_rejected_before_any_launch():
    """The only argument error of dx_jac_object / dx_dls_map reachable without a device
    batch; the others are in tests/test_gpu_dls.py."""
    build.build()
    L = _lib.load()
    t = np.array([_lib.OBJ_SITE], np.int32)
    i = np.zeros(1, np.int32)
    v = np.zeros(3, np.float32)
    out = np.zeros(64, np.float32)
    assert L.dx_jac_object(None, t.ctypes.data, i.ctypes.data, 1, out.ctypes.data, None) == -1  # DX_EINVAL
    assert b"null batch" in L.dx_last_error()
    assert L.dx_dls_map(None, t.ctypes.data, i.ctypes.data, 1, 1e-5, v.ctypes.data, out.ctypes.data, None) == -1
    assert b"null batch" in L.dx_last_error()
