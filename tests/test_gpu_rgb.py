"""Shaded RGB cameras on the device (include/dx.h "Shaded RGB", dx_render_set_shading,
DX_RENDER_RGB, DX_OUT_RGB; dx_render.hip dx_shade_kernel) against the fp64 reference of
tests/shade_ref.py.

Byte rule, on every pixel the reference calls stable (shade_ref.unstable_rgb; at most 2 % of
an image are not, tests/test_shade_host.py checks the same inputs on the CPU): the byte equals
the reference's floor(255 c + 0.5), unless the reference's 255 c lies within 255 b of a
half-integer, b = 4 max(e32c, 16 eps32) -- then it may differ by 1.  A miss is the background,
exactly.  The exact contracts are bit for bit.
"""

import ctypes
import functools

import numpy as np
import pytest

import camera_ref as cr
import shade_ref as sr
import test_gpu_camera as tg
from dexterity_amd import _lib
from dexterity_amd import cameras as cameras_lib

pytestmark = pytest.mark.gpu

B = sr.colour_bound(sr.MEASURED_E32C)
FIRST = 0
NO_SHADOW = (cameras_lib.Light(castshadow=False),)
FACES = np.asarray(cameras_lib.PALETTE_FACES[::-1], np.float32)  # (not the default order)


def _apply(phys, st):
    phys.set_shading(geom_rgb=st.geom_rgb, box_faces=st.box_faces, lights=st.lights, shading=st.shading)


def _cameras(scene):
    return list(sr.CAMERAS) + [tg.PALM] if scene.name == "reorient" else [tg.ADROIT_TOP]


@functools.lru_cache(maxsize=None)
def rendered(scene_fn, width, height, cull=True, variant="default"):
    """(rgb [nenv, ncam, H, W, 3], depth, segmentation, camera names) of the scene's cameras."""
    scene, phys = scene_fn(), tg.batch_of(scene_fn)
    st = sr.default_settings(scene.cm)
    if variant == "no_shadow":
        st = st._replace(lights=NO_SHADOW)
    elif variant == "faces":
        st = st._replace(box_faces={g: FACES for g in st.box_faces})
    _apply(phys, st)
    cfgs = _cameras(scene)
    phys.set_cameras(cfgs, width, height, depth=True, segmentation=True, rgb=True, near=cr.NEAR, far=cr.FAR, cull=cull)
    phys.render()
    return phys.rgb(), phys.depth(), phys.segmentation(), tuple(c.name for c in cfgs)


# --------------------------------------------------------------------------- #
# parity
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("k", range(4))
def test_reorient_parity(k, oracle_mod):
    scene = tg.reorient_scene()
    (w, h), cfg = cr.SIZES[k // 2], sr.CAMERAS[k % 2]
    rgb, _, seg, names = rendered(tg.reorient_scene, w, h)
    assert rgb.shape == (scene.nenv, 3, h, w, 3) and rgb.dtype == np.uint8
    c = names.index(cfg.name)
    assert 255.0 * B < 0.5
    for e in range(scene.nenv):
        ref = sr.reference(oracle_mod, scene, cfg, w, h, e)
        sr.check_bytes(ref, rgb[e, c], B, label=f"reorient env {e} {cfg.name} {w}x{h}")
        assert np.array_equal(seg[e, c].reshape(-1)[~ref.unstable], ref.base.g[~ref.unstable])


def test_adroit_parity(oracle_mod):
    scene = tg.adroit_scene()
    rgb, _, seg, _ = rendered(tg.adroit_scene, 19, 13)
    ref = sr.reference(oracle_mod, scene, tg.ADROIT_TOP, 19, 13, 0)
    sr.check_bytes(ref, rgb[0, 0], B, label="adroit env 0")
    # no ground: the misses are the background (black by default), exactly
    assert (seg[0, 0] == -1).any() and np.all(rgb[0, 0][seg[0, 0] == -1] == 0)


# --------------------------------------------------------------------------- #
# shadows and faces are exercised
# --------------------------------------------------------------------------- #
def test_castshadow_off_only_brightens(oracle_mod):
    scene = tg.reorient_scene()
    w, h = cr.SIZES[0]
    on, _, _, names = rendered(tg.reorient_scene, w, h)
    off, _, _, _ = rendered(tg.reorient_scene, w, h, variant="no_shadow")
    stable = brighter = 0
    for cfg in sr.CAMERAS:
        c = names.index(cfg.name)
        for e in range(scene.nenv):
            st = ~sr.reference(oracle_mod, scene, cfg, w, h, e).unstable
            a, b = on[e, c].reshape(-1, 3)[st].astype(int), off[e, c].reshape(-1, 3)[st].astype(int)
            assert np.all(b >= a), (cfg.name, e)
            stable += int(st.sum())
            brighter += int(np.any(b > a, axis=1).sum())
    print(f"castshadow off: {brighter} of {stable} stable pixels brighter")
    assert brighter >= 0.01 * stable


def test_box_faces(oracle_mod):
    scene = tg.reorient_scene()
    w, h = cr.SIZES[0]
    rgb, _, _, names = rendered(tg.reorient_scene, w, h, variant="faces")
    (cube,) = sr.default_settings(scene.cm).box_faces
    seen, pixels = set(), 0
    for cfg in sr.CAMERAS:
        c = names.index(cfg.name)
        for e in range(scene.nenv):
            ref = sr.reference(oracle_mod, scene, cfg, w, h, e)  # (face and irradiance do not depend on the colours)
            s = ~ref.unstable & (ref.base.g == cube)
            irr = np.minimum(1.0, ref.base.E[s])
            alb = rgb[e, c].reshape(-1, 3)[s] / 255.0 / irr
            want = FACES[ref.base.face[s]].astype(np.float64)
            # a byte is within half a step, and b, of 255 albedo irradiance
            assert np.all(np.abs(alb - want) <= (0.5 / 255.0 + B) / irr + 1e-12), (cfg.name, e)
            seen |= set(ref.base.face[s].tolist())
            pixels += int(s.sum())
    print(f"cube pixels {pixels}, faces seen {sorted(seen)}")
    assert pixels > 20 and len(seen) >= 2


# --------------------------------------------------------------------------- #
# exact contracts
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("size", cr.SIZES)
def test_no_cull_is_bit_identical(size):
    r0, d0, s0, _ = rendered(tg.reorient_scene, *size)
    r1, d1, s1, _ = rendered(tg.reorient_scene, *size, cull=False)
    assert np.array_equal(r0, r1)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(s0, s1)
    assert len(np.unique(r0.reshape(-1, 3), axis=0)) > 20


def test_two_renders_are_bit_identical():
    scene, phys = tg.reorient_scene(), tg.batch_of(tg.reorient_scene)
    _apply(phys, sr.default_settings(scene.cm))
    phys.set_cameras([cr.NEAR_TOP, tg.PALM], 32, 24, depth=False, segmentation=False, rgb=True, near=cr.NEAR, far=cr.FAR)
    phys.render()
    r0 = phys.rgb()
    phys.render()
    assert np.array_equal(r0, phys.rgb())


@pytest.mark.parametrize("size", cr.SIZES)
def test_camera_alone_equals_its_slice(size):
    scene, phys = tg.reorient_scene(), tg.batch_of(tg.reorient_scene)
    r3, _, _, names = rendered(tg.reorient_scene, *size)
    _apply(phys, sr.default_settings(scene.cm))
    for cfg in _cameras(scene):
        phys.set_cameras([cfg], size[0], size[1], depth=False, segmentation=False, rgb=True, near=cr.NEAR, far=cr.FAR)
        phys.render()
        assert np.array_equal(phys.rgb()[:, 0], r3[:, names.index(cfg.name)]), cfg.name


@pytest.mark.parametrize("size", cr.SIZES)
def test_depth_and_segmentation_do_not_change_beside_rgb(size):
    scene, phys = tg.reorient_scene(), tg.batch_of(tg.reorient_scene)
    _, d1, s1, _ = rendered(tg.reorient_scene, *size)
    phys.set_cameras(_cameras(scene), size[0], size[1], depth=True, segmentation=True, near=cr.NEAR, far=cr.FAR)
    phys.render()
    assert np.array_equal(phys.depth().view(np.uint32), d1.view(np.uint32)) and np.array_equal(phys.segmentation(), s1)
    with pytest.raises(_lib.DxError):
        phys.rgb()  # not enabled


# --------------------------------------------------------------------------- #
# the C ABI
# --------------------------------------------------------------------------- #
def test_abi():
    from dexterity_amd import physics as physics_lib

    scene = tg.reorient_scene()
    phys = physics_lib.BatchedPhysics(tg.batch_of(tg.reorient_scene).model, 2)
    phys.set(_lib.QPOS, scene.qpos[:2].astype(np.float32))
    phys.forward()
    L = _lib.load()
    ngeom = int(scene.cm.ngeom)
    (cube,) = sr.default_settings(scene.cm).box_faces
    # settings given before the cameras hold after them: one flat colour, ambient 1, no light
    flat = np.tile(np.float32([0.2, 0.4, 0.6]), (ngeom, 1))
    phys.set_shading(geom_rgb=flat, box_faces={}, lights=(), shading=cameras_lib.Shading(
        ambient=(1, 1, 1), headlight=(0, 0, 0), background=(0.25, 0.5, 0.75)))
    cam = (_lib.Camera * 1)()
    cam[0].pos[:] = [-0.02, -0.02, 0.55]
    cam[0].xyaxes[:] = [1, 0, 0, 0, 1, 0]
    cam[0].fovy, cam[0].near_, cam[0].far_, cam[0].body = 45.0, 0.01, 10.0, -1
    for flags in (16, _lib.RENDER_RGB | 16, _lib.RENDER_DEPTH | 32):
        assert L.dx_render_set_cameras(phys.ptr, cam, 1, 19, 13, flags) == -1  # unknown flag bits
    assert L.dx_render_set_cameras(phys.ptr, cam, 1, 19, 13, 0) == -1
    assert L.dx_render_set_cameras(phys.ptr, cam, 1, 19, 13, _lib.RENDER_NO_CULL) == -1
    # RGB alone: the cast's buffers stay the library's own
    for size in ((19, 13), (32, 24)):
        assert L.dx_render_set_cameras(phys.ptr, cam, 1, size[0], size[1], _lib.RENDER_RGB) == 0
        assert L.dx_render(phys.ptr) == 0
        p = ctypes.c_void_p()
        assert L.dx_render_output(phys.ptr, _lib.RENDER_RGB, ctypes.byref(p)) == 0 and p.value
        assert L.dx_render_output(phys.ptr, _lib.RENDER_DEPTH, ctypes.byref(p)) == -1
        assert L.dx_render_output(phys.ptr, _lib.RENDER_SEGMENTATION, ctypes.byref(p)) == -1
        img = np.zeros((2, 1, size[1], size[0], 3), np.uint8)
        assert L.dx_render_get(phys.ptr, _lib.RENDER_RGB, img.ctypes.data, 0, 2) == 0
        assert np.array_equal(np.unique(img.reshape(-1, 3), axis=0), [[51, 102, 153]])  # (the ground fills the view)
    # the refusals and their codes; a refused call changes nothing
    rgb = np.ascontiguousarray(flat)
    faces = np.zeros((9, 6, 3), np.float32)
    lights = (_lib.Light * 5)()
    for l in lights:
        l.dir[:] = [0, 0, -1]
        l.directional = 1

    def call(geom_rgb=rgb, fg=(), nface=None, lt=lights, nlight=0):
        arr = (ctypes.c_int32 * max(len(fg), 1))(*fg)
        return L.dx_render_set_shading(phys.ptr, geom_rgb.ctypes.data, arr, faces.ctypes.data,
                                       len(fg) if nface is None else nface, lt, nlight, None)

    assert call(nlight=5) == -5 and call(fg=[cube] * 9) == -5           # DX_ELIMIT
    assert call(fg=[0]) == -1 and call(fg=[cube - 1]) == -1             # the plane, a hull: no box geoms
    assert call(fg=[cube, cube]) == -1 and call(fg=[ngeom]) == -1
    bad = rgb.copy()
    bad[3, 1] = np.nan
    assert call(geom_rgb=bad) == -1
    lights[0].dir[:] = [0, 0, 0]
    assert call(nlight=1) == -1                                         # a zero dir on a directional light
    assert L.dx_render(phys.ptr) == 0
    assert L.dx_render_get(phys.ptr, _lib.RENDER_RGB, img.ctypes.data, 0, 2) == 0
    assert np.array_equal(np.unique(img.reshape(-1, 3), axis=0), [[51, 102, 153]])
    # ncam = 0 switches everything off
    assert L.dx_render_set_cameras(phys.ptr, None, 0, 0, 0, 0) == 0
    assert L.dx_render(phys.ptr) == -1
    assert L.dx_render_output(phys.ptr, _lib.RENDER_RGB, ctypes.byref(p)) == -1
    phys.close()


def test_positional_light_and_tilings_agree():
    """A positional shadow-casting light beside the default one: its cull (the segment sweep)
    does not change the bytes at either size, nor does rendering the camera alone."""
    scene, phys = tg.reorient_scene(), tg.batch_of(tg.reorient_scene)
    st = sr.default_settings(scene.cm)
    lamp = cameras_lib.Light(pos=(0.15, -0.1, 0.5), directional=False, diffuse=(0.4, 0.3, 0.2))
    _apply(phys, st._replace(lights=st.lights + (lamp,)))
    for w, h in cr.SIZES:
        out = []
        for cull in (True, False):
            phys.set_cameras(list(sr.CAMERAS), w, h, depth=False, segmentation=False, rgb=True, near=cr.NEAR, far=cr.FAR,
                             cull=cull)
            phys.render()
            out.append(phys.rgb())
        assert np.array_equal(out[0], out[1])
        phys.set_cameras([sr.NEAR_FRONT], w, h, depth=False, segmentation=False, rgb=True, near=cr.NEAR, far=cr.FAR)
        phys.render()
        assert np.array_equal(phys.rgb()[:, 0], out[0][:, 1])
    base, _, _, _ = rendered(tg.reorient_scene, *cr.SIZES[1])
    assert not np.array_equal(base[:, :2], out[0])  # the lamp shows


# --------------------------------------------------------------------------- #
# env level
# --------------------------------------------------------------------------- #
def test_env_rgb(oracle_mod):
    from dexterity_amd import manipulation

    task = manipulation.ReOrient()
    dt = float(task.compiled.timestep) * int(task.params()[0])
    W, H = 19, 13
    opts = dict(height=H, width=W, depth=True, segmentation=True, rgb=True, near=cr.NEAR, far=cr.FAR,
                shading=dict(shading=sr.CHECKER))
    kw = dict(seed=5, num_envs=4, time_limit=1.5 * dt)  # LAST on step 2, FIRST again on step 3
    env = manipulation.load("reorient", "state_dense", cameras=[sr.NEAR_FRONT, tg.PALM], camera_options=opts, **kw)
    plain = manipulation.load("reorient", "state_dense", **kw)
    scene = tg.reorient_scene()
    st = sr.default_settings(scene.cm)
    rng = np.random.RandomState(3)
    spec = env.action_spec()
    ts, tp = env.reset(), plain.reset()
    assert env.rgb_ptr()
    seen_first_after_step = False
    prev, checked = None, 0
    for step in range(4):
        keys = list(ts.observation)
        assert keys[: len(tp.observation)] == list(tp.observation)
        assert keys[len(tp.observation):] == [f"{n}_{k}" for n in (sr.NEAR_FRONT.name, "palm") for k in ("depth", "segmentation", "rgb")]
        ospec = env.observation_spec()
        assert list(ospec) == keys
        for name in (sr.NEAR_FRONT.name, "palm"):
            img, sp = ts.observation[f"{name}_rgb"], ospec[f"{name}_rgb"]
            assert img.shape == (4, H, W, 3) and img.dtype == np.uint8
            assert sp.shape == (H, W, 3) and sp.dtype == np.uint8 and sp.minimum.min() == 0 and sp.maximum.max() == 255
        # everything else is what an env without cameras yields, bit for bit
        for k in tp.observation:
            assert np.array_equal(ts.observation[k], tp.observation[k]), (step, k)
        assert np.array_equal(ts.reward, tp.reward) and np.array_equal(ts.discount, tp.discount)
        assert np.array_equal(ts.step_type, tp.step_type)
        assert np.array_equal(env._read(_lib.OUT_OBS, np.float32, env.obs_dim).view(np.uint32),
                              plain._read(_lib.OUT_OBS, np.float32, plain.obs_dim).view(np.uint32))
        # the env's image equals a batch-level render of the same state
        rgb = env.physics.rgb()
        assert np.array_equal(ts.observation[f"{sr.NEAR_FRONT.name}_rgb"], rgb[:, 0])
        assert np.array_equal(ts.observation["palm_rgb"], rgb[:, 1])
        env.physics.render()
        assert np.array_equal(env.physics.rgb(), rgb)
        # an env that returned FIRST shows its reset state
        qpos = env.physics.get(_lib.QPOS).astype(np.float64)
        for e in (np.nonzero(ts.step_type == FIRST)[0][:2] if step else [0]):
            ref = sr.reference(oracle_mod, scene, sr.NEAR_FRONT, W, H, int(e), st=st, qpos=qpos[e])
            if ref.unstable.mean() <= sr.UNSTABLE_CAP:  # (a random reset state: the cap is a condition on inputs)
                sr.check_bytes(ref, rgb[e, 0], sr.colour_bound(max(ref.e32c, sr.MEASURED_E32C)), label=f"env step {step} env {e}")
                checked += 1
            if step:
                seen_first_after_step = True
                assert not np.array_equal(rgb[e], prev[e])  # not the pre-reset image
        prev = rgb
        a = rng.uniform(spec.minimum, spec.maximum, size=(4, env.model.nu)).astype(np.float32)
        ts, tp = env.step(a), plain.step(a)
    assert seen_first_after_step and checked >= 2
    ts = env.timestep()
    assert f"{sr.NEAR_FRONT.name}_rgb" in ts.observation
    env.enable_cameras([])
    ts = env.step(a)
    assert list(ts.observation) == list(tp.observation)
    with pytest.raises(_lib.DxError):
        env.rgb_ptr()
    env.close()
    plain.close()
