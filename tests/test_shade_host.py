"""The shading model of the RGB cameras on the CPU (include/dx.h "Shaded RGB"): the fp64
reference of tests/shade_ref.py against closed forms, the inputs of tests/test_gpu_rgb.py
within their own conditions (unstable share, e32c, not vacuous), and the refusals of the
shading settings' validation.
"""

import types

import numpy as np
import pytest

import camera_ref as cr
import shade_ref as sr
from dexterity_amd import cameras as cameras_lib
from dexterity_amd import physics as physics_lib

# straight down; off the sphere's axis, so that the sphere does not hide its own shadow
TOP = cameras_lib.CameraConfig("top", (0.6, 0.0, 2.0), (1, 0, 0, 0, 1, 0), fovy=50.0)
ALBEDO = np.array([[0.5, 0.6, 0.7], [0.9, 0.4, 0.2]])
PLAIN = cameras_lib.Shading(headlight=(0.0, 0.0, 0.0))


def _scene(types_, sizes):
    """A model of primitives only, as far as camera_ref.cast and shade_ref.shade read one."""
    return types.SimpleNamespace(ngeom=len(types_), geom_type=np.array(types_), geom_size=np.array(sizes, dtype=np.float64),
                                 geom_dataid=np.full(len(types_), -1), mesh_vert=np.zeros((0, 3)), mesh_vertadr=[],
                                 mesh_vertnum=[])


def _shade(cm, gpos, gmat, st, width=81, height=81, config=TOP):
    o, d = cr.world_rays(config, width, height)
    return sr.shade(cm, np.array(gpos, dtype=np.float64), np.array(gmat, dtype=np.float64), o, d, cr.NEAR, cr.FAR, st,
                    sr.camera_z(config)), o, d


# --------------------------------------------------------------------------- #
# closed forms
# --------------------------------------------------------------------------- #
def test_sphere_over_plane_under_the_vertical_light():
    r, z = 0.1, 0.4
    cm = _scene([cr.PLANE, cr.SPHERE], [[0, 0, 0], [r, 0, 0]])
    st = sr.Settings(ALBEDO.astype(np.float32), {}, cameras_lib.DEFAULT_LIGHTS, PLAIN)
    res, o, d = _shade(cm, [[0, 0, 0], [0, 0, z]], [np.eye(3), np.eye(3)], st)
    amb, dif = np.float32(0.2).astype(np.float64), np.float32(0.5).astype(np.float64)
    alb = ALBEDO.astype(np.float32).astype(np.float64)
    plane, ball = res.g == 0, res.g == 1
    assert plane.sum() > 100 and ball.sum() > 50
    # the plane's shadow: exactly the hit points within r of the sphere's axis
    rho = np.linalg.norm(res.P[plane, :2], axis=1)
    assert np.array_equal(res.occ[0][plane], rho < r)
    assert (rho < r).any() and (rho > r).any()
    assert np.abs(res.c[plane] - alb[0] * (amb + dif * ~res.occ[0][plane][:, None])).max() < 1e-12
    # the sphere: albedo (ambient + diffuse n_z), n from the hit point
    nz = (res.P[ball, 2] - z) / r
    assert not res.occ[0][ball].any() and nz.max() > 0.9 and nz.min() < 0  # (below the equator: it shadows itself)
    assert np.abs(res.c[ball] - alb[1] * (amb + dif * np.maximum(nz, 0)[:, None])).max() < 1e-12
    assert np.array_equal(res.byte[ball], np.floor(255 * res.c[ball] + 0.5).astype(np.uint8))
    # and with a background: a miss is the background, exactly
    sky = cameras_lib.CameraConfig("sky", (0.0, 0.0, 2.0), (1, 0, 0, 0, 0, 1), fovy=30.0)  # looks along -y
    bg = sr.Settings(st.geom_rgb, {}, st.lights, cameras_lib.Shading(background=(0.25, 0.5, 0.75)))
    res2, _, _ = _shade(cm, [[0, 0, 0], [0, 0, z]], [np.eye(3), np.eye(3)], bg, 9, 9, sky)
    up = res2.g < 0
    assert up.any() and np.array_equal(np.unique(res2.byte[up], axis=0), [[64, 128, 191]])


@pytest.mark.parametrize("face", range(6))
def test_box_turned_to_each_face_shows_its_colour(face):
    cm = _scene([cr.BOX], [[0.05, 0.07, 0.09]])
    k, neg = face // 2, face % 2
    # the rotation that turns the face's outward normal to world +z (towards the camera)
    nrm = np.zeros(3)
    nrm[k] = -1.0 if neg else 1.0
    a = np.zeros(3)
    a[(k + 1) % 3] = 1.0
    R = np.stack([a, np.cross(nrm, a), nrm])  # rows: world x, y, z in the box frame
    cols = np.asarray(cameras_lib.PALETTE_FACES, np.float32)
    st = sr.Settings(np.full((1, 3), 0.5, np.float32), {0: cols}, cameras_lib.DEFAULT_LIGHTS, PLAIN)
    res, _, _ = _shade(cm, [[0.6, 0, 1.5]], [R], st, 31, 31)
    seen = res.g == 0
    assert seen.sum() > 20
    assert np.all(res.face[seen] == face)
    assert np.abs(res.alb[seen] - cols[face].astype(np.float64)).max() == 0
    assert np.abs(res.c[seen] - cols[face].astype(np.float64) * (0.2 + 0.5)).max() < 1e-7


def test_checker_parity_on_both_sides_of_a_cell_edge():
    cm = _scene([cr.PLANE], [[0, 0, 0]])
    cell = 0.25
    sh = cameras_lib.Shading(checker_rgb=((0.1, 0.1, 0.1), (0.9, 0.9, 0.9)), checker_cell=cell, headlight=(0, 0, 0))
    st = sr.Settings(np.zeros((1, 3), np.float32), {}, (), sh)
    res, _, _ = _shade(cm, [[0, 0, 0]], [np.eye(3)], st, 64, 64)
    assert res.hit.all()
    par = (np.floor(res.P[:, 0] / cell) + np.floor(res.P[:, 1] / cell)).astype(np.int64) & 1
    want = np.where(par[:, None] == 1, np.float32(0.9), np.float32(0.1)).astype(np.float64) * np.float32(0.2).astype(np.float64)
    assert np.abs(res.c - want).max() < 1e-12
    # two pixels either side of the edge x = 0, and of y = -cell (negative cells too)
    img = res.byte[:, 0].reshape(64, 64)
    x = res.P[:, 0].reshape(64, 64)[40]
    k = int(np.searchsorted(x, 0.0))
    assert x[k - 1] < 0 < x[k] and img[40, k - 1] != img[40, k] and len(np.unique(img)) == 2


# --------------------------------------------------------------------------- #
# the inputs of the GPU tests stay within their own conditions
# --------------------------------------------------------------------------- #
def gpu_cases():
    """(scene, config, width, height, env) of tests/test_gpu_rgb.py's parity tests."""
    import test_gpu_camera as tg

    scene = tg.reorient_scene()
    out = [(scene, cfg, w, h, e) for (w, h) in cr.SIZES for cfg in sr.CAMERAS for e in range(scene.nenv)]
    out.append((tg.adroit_scene(), tg.ADROIT_TOP, 19, 13, 0))
    return out


def test_gpu_test_inputs(oracle_mod):
    worst, shares = 0.0, []
    tot = dict(stable=0, obj=0, shadow=0, lit=0)
    for scene, cfg, w, h, e in gpu_cases():
        ref = sr.reference(oracle_mod, scene, cfg, w, h, e)
        st = ~ref.unstable
        share = float(ref.unstable.mean())
        need, occ = ref.base.need[0], ref.base.occ[0]
        print(f"{scene.name} env {e} {cfg.name} {w}x{h}: unstable {int(ref.unstable.sum())} ({100 * share:.2f} %) e32c {ref.e32c:.3g} "
              f"objects {int((st & (ref.base.g > 0)).sum())} shadowed {int((st & need & occ).sum())} lit {int((st & need & ~occ).sum())} "
              f"g32 differs on {int((st & (ref.g32 != ref.base.g)).sum())} stable pixels")
        assert share <= sr.UNSTABLE_CAP, (scene.name, cfg.name, w, h, e, share)
        assert not (st & (ref.g32 != ref.base.g)).any()
        worst = max(worst, ref.e32c)
        shares.append(share)
        if scene.name == "reorient":
            tot["stable"] += int(st.sum())
            tot["obj"] += int((st & (ref.base.g > 0)).sum())
            tot["shadow"] += int((st & need & occ).sum())
            tot["lit"] += int((st & need & ~occ).sum())
    b = sr.colour_bound(worst)
    print(f"e32c {worst:.3g}; b {b:.3g}; 255 b {255 * b:.3g}; worst unstable share {100 * max(shares):.2f} %; {tot}")
    assert 255.0 * 4.0 * max(worst, 16 * cr.EPS32) < 0.5
    assert worst <= sr.MEASURED_E32C  # (the constant the GPU tests use covers these cases)
    # not vacuous: objects, pixels in shadow of the light they face, pixels lit by it
    assert tot["obj"] >= 0.05 * tot["stable"]
    assert tot["shadow"] >= 0.01 * tot["stable"]
    assert tot["lit"] >= 0.01 * tot["stable"]


# --------------------------------------------------------------------------- #
# validation
# --------------------------------------------------------------------------- #
TYPES = np.array([cr.PLANE, cr.BOX, cr.MESH, cr.SPHERE])


def _validate(**kw):
    args = dict(geom_rgb=np.zeros((4, 3)), box_faces={1: np.zeros((6, 3))}, lights=cameras_lib.DEFAULT_LIGHTS,
                shading=cameras_lib.DEFAULT_SHADING, geom_types=TYPES)
    args.update(kw)
    return cameras_lib.validate_shading(**args)


def test_validate_shading_accepts():
    rgb, fg, frgb, lights, sh = _validate()
    assert rgb.shape == (4, 3) and rgb.dtype == np.float32 and fg.tolist() == [1] and frgb.shape == (1, 6, 3)
    assert lights == cameras_lib.DEFAULT_LIGHTS and sh == cameras_lib.DEFAULT_SHADING
    d = cameras_lib.DEFAULT_LIGHTS[0]
    assert d.directional and d.castshadow and tuple(d.dir) == (0.0, 0.0, -1.0)  # the arena's light


@pytest.mark.parametrize("kw, word", [
    (dict(lights=[cameras_lib.Light()] * 5), "at most 4"),
    (dict(box_faces={2: np.zeros((6, 3))}), "not a box geom"),
    (dict(box_faces={7: np.zeros((6, 3))}), "not a box geom"),
    (dict(box_faces={1: np.zeros((5, 3))}), "six finite RGB"),
    (dict(geom_rgb=np.zeros((3, 3))), r"shape \[ngeom, 3\]"),
    (dict(geom_rgb=np.zeros((4, 4))), r"shape \[ngeom, 3\]"),
    (dict(geom_rgb=np.full((4, 3), np.nan)), "non-finite"),
    (dict(lights=[cameras_lib.Light(dir=(0.0, 0.0, 0.0))]), "dir that is not zero"),
    (dict(lights=[cameras_lib.Light(diffuse=(0.0, np.inf, 0.0))]), "diffuse"),
    (dict(shading=cameras_lib.Shading(checker_cell=-1.0)), "checker_cell"),
    (dict(shading=cameras_lib.Shading(ambient=(0.1, 0.2))), "ambient"),
])
def test_validate_shading_refuses(kw, word):
    with pytest.raises(ValueError, match=word):
        _validate(**kw)


def test_a_positional_light_may_have_a_zero_dir():
    _validate(lights=[cameras_lib.Light(pos=(0, 0, 1), dir=(0, 0, 0), directional=False)])


def test_validate_rgb_keyword():
    good = dict(width=84, height=84, near=0.01, far=10.0, num_envs=4, body_names=["world"])
    cfgs = cameras_lib.resolve(["top_down"])
    assert cameras_lib.validate(cfgs, depth=False, segmentation=False, rgb=True, **good) == [-1]
    with pytest.raises(ValueError, match="nothing to render"):
        cameras_lib.validate(cfgs, depth=False, segmentation=False, rgb=False, **good)
    with pytest.raises(ValueError, match="nothing to render"):
        cameras_lib.validate(cfgs, depth=False, segmentation=False, **good)


def test_methods_refuse_before_any_library_call():
    """set_shading validates first: a handle without a library raises ValueError."""
    from dexterity_amd import manipulation
    from dexterity_amd.mjcf.compiler import CompiledModel
    import test_gpu_camera as tg

    cm = tg.reorient_scene().cm
    phys = physics_lib.BatchedPhysics.__new__(physics_lib.BatchedPhysics)
    phys.ptr, phys.nenv, phys._owned = None, 4, False
    phys.model = types.SimpleNamespace(compiled=cm)
    with pytest.raises(ValueError, match="at most 4"):
        phys.set_shading(lights=[cameras_lib.Light()] * 5)
    with pytest.raises(ValueError, match="not a box geom"):
        phys.set_shading(box_faces={0: np.zeros((6, 3))})
    with pytest.raises(ValueError, match="nothing to render"):
        phys.set_cameras(["top_down"], 32, 24, depth=False, segmentation=False, rgb=False)
    env = manipulation.GoalEnvironment.__new__(manipulation.GoalEnvironment)
    env.ptr, env.physics, env.num_envs = None, None, 4
    env.task = types.SimpleNamespace(compiled=cm)
    with pytest.raises(ValueError, match=r"shape \[ngeom, 3\]"):
        env.enable_cameras(["top_down"], rgb=True, shading=dict(geom_rgb=np.zeros((2, 3))))
    assert isinstance(cm, CompiledModel)


def test_default_palette():
    import test_gpu_camera as tg

    cm = tg.reorient_scene().cm
    rgb, faces = cameras_lib.default_palette(cm)
    assert rgb.shape == (int(cm.ngeom), 3) and rgb.dtype == np.float32
    body = np.asarray(cm.geom_bodyid)
    assert np.all(rgb[body == 0] == np.float32(cameras_lib.PALETTE_WORLD))
    (g, cols), = faces.items()
    assert int(cm.geom_type[g]) == cr.BOX and cols.shape == (6, 3) and len(np.unique(cols, axis=0)) == 6
    hand = (body != 0) & (np.arange(len(body)) != g)
    assert np.all(rgb[hand] == np.float32(cameras_lib.PALETTE_HANDS[0]))
    # the exports of the C ABI
    from dexterity_amd import _lib

    assert {"dx_render_set_shading", "dx_env_set_shading"} <= set(_lib.EXPORTS)
    assert (_lib.RENDER_RGB, _lib.OUT_RGB, _lib.RENDER_MAX_LIGHTS, _lib.RENDER_MAX_FACE_GEOMS) == (8, 15, 4, 8)
