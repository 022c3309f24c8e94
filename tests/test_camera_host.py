"""Depth / segmentation cameras, the host side (no GPU): the hull face planes the library
derives (include/dx.h dx_model_hull_planes) against scipy's ConvexHull, the fp64 reference
ray cast of tests/camera_ref.py against analytic answers, the pinhole model of
dexterity_amd.cameras.camera_rays, the option validation of set_cameras / enable_cameras,
and the inputs of tests/test_gpu_camera.py against their own cap on unstable pixels.
"""

import math
import os

import numpy as np
import pytest

import camera_ref as cr
from dexterity_amd import cameras as cameras_lib
from dexterity_amd import physics as physics_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def asset(name):
    return os.path.join(ROOT, "assets", f"{name}.npz")


# --------------------------------------------------------------------------- #
# hull planes
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", ["shadow_reorient", "adroit_reach"])
def test_hull_planes_match_scipy(name):
    model = physics_lib.Model.from_file(asset(name))
    cm = model.compiled
    V = np.asarray(cm.mesh_vert, dtype=np.float64).reshape(-1, 3)
    eqs = cr.hull_equations(cm)
    total = 0
    for k, (a, n) in enumerate(zip(cm.mesh_vertadr, cm.mesh_vertnum)):
        P = model.hull_planes(k).astype(np.float64)
        v = V[a:a + n]
        R = np.abs(v).max()
        assert len(P) >= 4, (k, len(P))
        # every hull vertex inside every plane
        assert (v @ P[:, :3].T + P[:, 3]).max() <= 1e-6 * R, k
        # unit normals
        assert np.abs(np.linalg.norm(P[:, :3], axis=1) - 1.0).max() <= 1e-6, k
        # every scipy facet has a library plane
        gap = np.abs(eqs[k][:, None, :] - P[None, :, :]).max(axis=2).min(axis=1)
        assert gap.max() <= 1e-5, (k, gap.max())
        # coplanar triangles merged, nothing invented
        assert len(P) <= len(eqs[k]), (k, len(P), len(eqs[k]))
        total += len(P)
    assert total <= sum(len(e) for e in eqs)
    # a short destination gets the first planes and the full count
    L = physics_lib._lib.load()
    buf = np.zeros((2, 4), np.float32)
    assert L.dx_model_hull_planes(model.ptr, 0, buf.ctypes.data, 2) == len(model.hull_planes(0))
    assert np.array_equal(buf, model.hull_planes(0)[:2])
    assert L.dx_model_hull_planes(model.ptr, len(cm.mesh_vertnum), None, 0) < 0


# --------------------------------------------------------------------------- #
# the reference against analytic answers
# --------------------------------------------------------------------------- #
def test_reference_top_down_analytic(reorient_compiled, oracle_mod):
    cm = reorient_compiled
    gpos, gmat, _, _ = cr.oracle_state(oracle_mod, cm, cm.qpos0)
    W, H = 33, 25
    o, d = cr.world_rays(cameras_lib.TOP_DOWN, W, H)
    t, g = cr.cast(cm, gpos, gmat, o, d, cr.NEAR, cr.FAR)
    ground = int(np.nonzero(np.asarray(cm.geom_type) == cr.PLANE)[0][0])
    assert np.all(g >= 0)
    assert (g == ground).sum() > 0.9 * W * H
    assert np.abs(t[g == ground] - 2.5).max() < 1e-12
    # the cube (the prop's box, centre z = 0.16, half-size 0.02): its top face
    box = [i for i in range(int(cm.ngeom)) if int(cm.geom_type[i]) == cr.BOX]
    assert len(box) == 1
    assert abs(gpos[box[0]][2] - 0.16) < 1e-12 and np.allclose(np.asarray(cm.geom_size).reshape(-1, 3)[box[0]], 0.02)
    # a finer image over the cube: a narrow camera straight above it
    above = cameras_lib.CameraConfig("above", (gpos[box[0]][0], gpos[box[0]][1], 2.5), (1, 0, 0, 0, 1, 0), fovy=0.8)
    o, d = cr.world_rays(above, 21, 21)
    t, g = cr.cast(cm, gpos, gmat, o, d, cr.NEAR, cr.FAR)
    assert (g == box[0]).sum() > 50
    assert np.abs(t[g == box[0]] - (2.5 - 0.18)).max() < 1e-12


def test_reference_all_misses_when_facing_away(reorient_compiled, oracle_mod):
    cm = reorient_compiled
    gpos, gmat, _, _ = cr.oracle_state(oracle_mod, cm, cm.qpos0)
    up = cameras_lib.CameraConfig("up", (0.0, 0.0, 2.5), (1, 0, 0, 0, -1, 0))  # z = -world z: looks up
    o, d = cr.world_rays(up, 16, 12)
    assert np.all(d[:, 2] > 0)
    t, g = cr.cast(cm, gpos, gmat, o, d, cr.NEAR, cr.FAR)
    assert np.all(g == -1) and np.all(np.isinf(t))


def test_reference_float32_restatement_agrees(reorient_compiled, oracle_mod):
    """The float32 restatement of the kernel's arithmetic sees what the fp64 reference sees."""
    cm = reorient_compiled
    planes = cr.library_planes(asset("shadow_reorient"))
    gpos, gmat, xpos, xquat = cr.oracle_state(oracle_mod, cm, cm.qpos0)
    W, H = 19, 13
    o, d = cr.world_rays(cr.NEAR_TOP, W, H)
    t, g = cr.cast(cm, gpos, gmat, o, d, cr.NEAR, cr.FAR)
    bad = cr.unstable(cm, gpos, gmat, o, d, cr.NEAR, cr.FAR, g)
    t32, g32 = cr.cast32(cm, planes, xpos, xquat, cr.NEAR, cr.FAR, cr.NEAR_TOP, W, H)
    assert np.array_equal(g32[~bad], g[~bad])
    hit = ~bad & (g >= 0)
    assert np.all(np.abs(t32[hit] - t[hit]) <= cr.depth_bound(0.0, t[hit]))


# --------------------------------------------------------------------------- #
# camera_rays
# --------------------------------------------------------------------------- #
def test_camera_frame_from_skewed_axes():
    F = cameras_lib.camera_frame((2.0, 0.0, 0.0, 1.0, 0.5, 0.87))
    assert np.allclose(F @ F.T, np.eye(3), atol=1e-15)
    assert np.allclose(F[0], (1, 0, 0))
    assert np.allclose(F[2], np.cross(F[0], F[1]))
    assert F[1] @ np.array([1.0, 0.5, 0.87]) > 0


def test_camera_rays_pinhole():
    cfg = cameras_lib.CameraConfig("c", (0.1, 0.2, 0.3), (0.0, 1.0, 0.0, -0.7, 0.0, 0.75), fovy=50.0)
    W, H = 9, 7
    o, d = cameras_lib.camera_rays(cfg, W, H)
    x, y, z = cameras_lib.camera_frame(cfg.xyaxes)
    assert np.allclose(o, cfg.pos) and d.shape == (H, W, 3)
    # the centre pixel of an odd-sized image looks along -z
    assert np.allclose(d[H // 2, W // 2], -z, atol=1e-15)
    # depth along the optical axis: every direction has -z component 1
    assert np.allclose(d @ -z, 1.0, atol=1e-15)
    # the top row's centre ray: atan((H/2 - 0.5) / f) above the optical axis
    f = 0.5 * H / math.tan(math.radians(25.0))
    top = d[0, W // 2]
    ang = math.atan2(np.linalg.norm(np.cross(top, -z)), top @ -z)
    assert abs(ang - math.atan((H / 2 - 0.5) / f)) < 1e-14
    assert top @ y > 0  # row 0 is on top
    assert d[H // 2, W - 1] @ x > 0  # the last column is on the right
    assert abs(cameras_lib.focal_length(50.0, H) - f) < 1e-12


def test_named_cameras():
    assert sorted(cameras_lib.CAMERAS) == ["front_close", "front_far", "left_close", "right_close", "top_down"]
    assert cameras_lib.TOP_DOWN.pos == (0.0, 0.0, 2.5) and cameras_lib.TOP_DOWN.fovy == 45.0
    assert cameras_lib.resolve(["front_close", cr.NEAR_TOP]) == [cameras_lib.FRONT_CLOSE, cr.NEAR_TOP]
    assert cameras_lib.resolve("top_down") == [cameras_lib.TOP_DOWN]


# --------------------------------------------------------------------------- #
# option validation (before any library call: no GPU here)
# --------------------------------------------------------------------------- #
BODIES = ["world", "hand/forearm", "hand/palm"]
GOOD = dict(width=84, height=84, depth=True, segmentation=False, near=0.01, far=10.0, num_envs=4, body_names=BODIES)


def _validate(configs, **kw):
    return cameras_lib.validate(cameras_lib.resolve(configs), **{**GOOD, **kw})


def test_validate_accepts_and_resolves_bodies():
    palm = cameras_lib.CameraConfig("palm", (0, 0, 0.05), (1, 0, 0, 0, 1, 0), body="hand/palm")
    byid = cameras_lib.CameraConfig("byid", (0, 0, 0.05), (1, 0, 0, 0, 1, 0), body=1)
    assert _validate(["front_close", palm, byid]) == [-1, 2, 1]


@pytest.mark.parametrize("configs, kw, word", [
    (["no_such_camera"], {}, "unknown camera"),
    ([cameras_lib.CameraConfig("c", (0, 0, 1), (1, 0, 0, 2, 0, 0))], {}, "degenerate"),
    ([cameras_lib.CameraConfig("c", (0, 0, 1), (0, 0, 0, 0, 1, 0))], {}, "degenerate"),
    ([cameras_lib.CameraConfig("c", (0, 0, 1), (1, 0, 0, 0, 1, 0), fovy=0.0)], {}, "fovy"),
    ([cameras_lib.CameraConfig("c", (0, 0, 1), (1, 0, 0, 0, 1, 0), fovy=180.0)], {}, "fovy"),
    ([cameras_lib.CameraConfig("c", (0, 0, 1), (1, 0, 0, 0, 1, 0), body="hand/thumb")], {}, "no body named"),
    ([cameras_lib.CameraConfig("c", (0, 0, 1), (1, 0, 0, 0, 1, 0), body=3)], {}, "outside"),
    ([cameras_lib.CameraConfig("c", (0, 0, float("nan")), (1, 0, 0, 0, 1, 0))], {}, "pos"),
    (["top_down", "top_down"], {}, "names must differ"),
    (["top_down"], dict(near=0.0), "near"),
    (["top_down"], dict(near=1.0, far=1.0), "near"),
    (["top_down"], dict(depth=False, segmentation=False), "nothing to render"),
    (["top_down"], dict(width=513), "width and height"),
    (["top_down"], dict(height=0), "width and height"),
    (["top_down"], dict(num_envs=2**20, width=64, height=64), "reaches 2.31"),
    ([cameras_lib.CameraConfig(f"c{i}", (0, 0, 1), (1, 0, 0, 0, 1, 0)) for i in range(9)], {}, "at most 8"),
])
def test_validate_refuses(configs, kw, word):
    with pytest.raises(ValueError, match=word):
        _validate(configs, **kw)


def test_methods_refuse_before_any_library_call():
    """set_cameras / enable_cameras validate first: a handle without a library raises ValueError."""
    from dexterity_amd import manipulation

    class Compiled:
        names = {"body": BODIES}

    phys = physics_lib.BatchedPhysics.__new__(physics_lib.BatchedPhysics)
    phys.ptr, phys.nenv, phys._owned = None, 4, False
    phys.model = type("M", (), {"compiled": Compiled})()
    with pytest.raises(ValueError, match="near"):
        phys.set_cameras(["top_down"], 32, 24, near=-1.0)
    env = manipulation.GoalEnvironment.__new__(manipulation.GoalEnvironment)
    env.ptr, env.physics, env.num_envs = None, None, 4
    env.task = type("T", (), {"compiled": Compiled})()
    with pytest.raises(ValueError, match="fovy"):
        env.enable_cameras([cameras_lib.CameraConfig("c", (0, 0, 1), (1, 0, 0, 0, 1, 0), fovy=200.0)])
    with pytest.raises(ValueError, match="unknown camera"):
        env.enable_cameras(["behind"])


def test_wrappers_pass_enable_cameras_through():
    from dexterity_amd import wrappers

    calls = []

    class Env:
        def enable_cameras(self, *a, **kw):
            calls.append((a, kw))

    wrappers.Wrapper(wrappers.Wrapper(Env())).enable_cameras(["top_down"], height=32)
    assert calls == [((["top_down"],), {"height": 32})]


# --------------------------------------------------------------------------- #
# the inputs of the GPU tests stay within their own cap
# --------------------------------------------------------------------------- #
def test_gpu_test_inputs_are_stable(oracle_mod):
    """At most 1 % of each image of tests/test_gpu_camera.py is unstable in the reference
    (the one image outside the rule, test_gpu_camera.NO_PARITY, is 1.2 %)."""
    import test_gpu_camera as tg

    for scene in (tg.reorient_scene(), tg.adroit_scene()):
        for case in scene.cases:
            for e in tg.parity_envs(scene, case):
                ref = scene.reference(oracle_mod, case, e)
                assert ref.unstable.mean() <= 0.01, (scene.name, case.config.name, case.width, case.height, e,
                                                     int(ref.unstable.sum()))
    scene = tg.reorient_scene()
    for name, w, h, e in tg.NO_PARITY:  # what is left out really is over the cap, and nothing else is
        case = [c for c in scene.cases if (c.config.name, c.width, c.height) == (name, w, h)][0]
        assert scene.reference(oracle_mod, case, e).unstable.mean() > 0.01
