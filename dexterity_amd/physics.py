"""Batched physics handle: the MI355X counterpart of dm_control's `mjcf.Physics`.

One `BatchedPhysics` owns B environments that share a compiled model and live in
HBM.  The methods mirror the parts of `mjcf.Physics` the reference uses on its hot
path: `step()` (composer substep loop, reorient.py:168 /
reach.py:139), `forward()`, and reads/writes of qpos / qvel / ctrl /
xfrc_applied / site xpos / contacts -- every one batched over environments.
"""

from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from dexterity_amd import _lib
from dexterity_amd import blob as blob_lib
from dexterity_amd import cameras as cameras_lib
from dexterity_amd.mjcf.compiler import CompiledModel


class Model:
    """A compiled scene loaded into libdx (shared by any number of batches)."""

    def __init__(self, compiled: CompiledModel):
        self.compiled = compiled
        self.blob = blob_lib.pack(compiled.arrays)
        L = _lib.load()
        self.ptr = L.dx_model_load(self.blob, len(self.blob))
        if not self.ptr:
            raise _lib.DxError(f"dx_model_load failed: {L.dx_last_error().decode()}")
        sizes = (ctypes.c_int32 * 12)()
        _lib.check(L.dx_model_sizes(self.ptr, sizes))
        (self.nq, self.nv, self.nbody, self.njnt, self.ngeom, self.nsite, self.nu,
         self.ntendon, self.nbpair, self.ngpair, self.ncon_max, self.nefc_max) = list(sizes)
        self.lds_bytes = _lib.check(L.dx_model_lds_bytes(self.ptr))

    @staticmethod
    def from_file(path: str) -> "Model":
        return Model(CompiledModel.load(path))

    def width(self, field: int) -> int:
        return _lib.check(_lib.load().dx_field_width(self.ptr, field))

    def hull_planes(self, mesh: int) -> np.ndarray:
        """[n, 4] float32 face planes (unit n, d; n.x + d <= 0 inside, geom frame) the library
        derives for hull `mesh` (include/dx.h dx_model_hull_planes; no GPU needed)."""
        L = _lib.load()
        n = _lib.check(L.dx_model_hull_planes(self.ptr, int(mesh), None, 0))
        out = np.zeros((n, 4), np.float32)
        _lib.check(L.dx_model_hull_planes(self.ptr, int(mesh), out.ctypes.data, n))
        return out

    def __del__(self):
        if getattr(self, "ptr", None) and _lib._lib is not None:
            _lib._lib.dx_model_free(self.ptr)
            self.ptr = None


class BatchedPhysics:
    """B environments on one GPU; state resident in HBM."""

    def __init__(self, model: Model, nenv: int, device: int = 0):
        L = _lib.load()
        self.model = model
        self.nenv = int(nenv)
        self.device = device
        self.ptr = L.dx_batch_create(model.ptr, self.nenv, device)
        self._owned = True
        if not self.ptr:
            raise _lib.DxError(f"dx_batch_create failed: {L.dx_last_error().decode()}")

    @classmethod
    def borrowed(cls, model: Model, ptr: int, nenv: int, device: int) -> "BatchedPhysics":
        """A view of a batch owned elsewhere (e.g. by a dx_env); never destroyed here."""
        self = cls.__new__(cls)
        self.model, self.ptr, self.nenv, self.device, self._owned = model, ptr, int(nenv), device, False
        return self

    def close(self):
        if getattr(self, "ptr", None) and getattr(self, "_owned", False) and _lib._lib is not None:
            _lib._lib.dx_batch_destroy(self.ptr)
        self.ptr = None

    def __del__(self):
        self.close()

    # ------------------------------------------------------------------ #
    def step(self, nsubstep: int = 1) -> None:
        _lib.check(_lib.load().dx_step(self.ptr, nsubstep))

    def forward(self) -> None:
        _lib.check(_lib.load().dx_forward(self.ptr))

    def sync(self) -> None:
        _lib.check(_lib.load().dx_sync(self.ptr))

    def reset(self, env0: int = 0, n: Optional[int] = None) -> None:
        n = self.nenv - env0 if n is None else n
        _lib.check(_lib.load().dx_reset(self.ptr, env0, n))

    # ------------------------------------------------------------------ #
    def set(self, field: int, values, env0: int = 0) -> None:
        w = self.model.width(field)
        a = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, w)
        _lib.check(_lib.load().dx_set_field(self.ptr, field, a.ctypes.data, env0, a.shape[0]))
        self.sync()  # host buffer must outlive the async copy

    def set_device(self, field: int, devptr: int, env0: int, n: int) -> None:
        """Device-to-device copy from a raw device pointer (no host sync)."""
        _lib.check(_lib.load().dx_set_field(self.ptr, field, ctypes.c_void_p(devptr), env0, n))

    def get(self, field: int, env0: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.nenv - env0 if n is None else n
        w = self.model.width(field)
        dt = np.int32 if field in _lib.INT_FIELDS else np.float32
        out = np.empty((n, w), dtype=dt)
        _lib.check(_lib.load().dx_get_field(self.ptr, field, out.ctypes.data, env0, n))
        return out

    def field_ptr(self, field: int) -> int:
        p = ctypes.c_void_p()
        _lib.check(_lib.load().dx_field_ptr(self.ptr, field, ctypes.byref(p)))
        return p.value

    def set_xfrc(self, xfrc, env0: int = 0) -> None:
        """xfrc_applied: None (none) or [nbody, 6] -- one array shared by every env -- or
        [n, nbody, 6], every env its own rows as in MjData (envs env0 .. env0+n-1; the batch
        then stays in per-env mode until a shared array or None is set again)."""
        nbody = self.model.nbody
        if xfrc is None:
            _lib.check(_lib.load().dx_set_xfrc(self.ptr, None, 0))
            self.sync()
            return
        a = np.ascontiguousarray(xfrc, dtype=np.float32)
        if a.shape == (nbody, 6):
            _lib.check(_lib.load().dx_set_xfrc(self.ptr, a.ctypes.data, nbody))
        elif a.ndim == 3 and a.shape[1:] == (nbody, 6) and 1 <= a.shape[0] and 0 <= env0 and env0 + a.shape[0] <= self.nenv:
            _lib.check(_lib.load().dx_set_xfrc_env(self.ptr, a.ctypes.data, env0, a.shape[0]))
        else:
            raise ValueError(f"xfrc must be [nbody, 6] = [{nbody}, 6] or [n, {nbody}, 6] with env0 + n <= nenv = "
                             f"{self.nenv}, got {a.shape} at env0 = {env0}")
        self.sync()  # host buffer must outlive the async copy

    @property
    def xfrc_applied(self) -> np.ndarray:
        """A host copy of the applied wrenches, shaped by the current mode: [nbody, 6] while
        one array is shared (zeros while none is set), [nenv, nbody, 6] in per-env mode."""
        per_env = self.xfrc_ptr() is not None
        n = self.nenv if per_env else 1
        out = np.empty((n, self.model.nbody, 6), np.float32)
        _lib.check(_lib.load().dx_get_xfrc_env(self.ptr, out.ctypes.data, 0, n))
        return out if per_env else out[0]

    def xfrc_ptr(self) -> Optional[int]:
        """Device address of the per-env rows [nenv, nbody, 6] f32 (write them on the batch's
        stream; no host trip), or None while the batch shares one array."""
        p, stride = ctypes.c_void_p(), ctypes.c_int32()
        if _lib.load().dx_xfrc_ptr(self.ptr, ctypes.byref(p), ctypes.byref(stride)) < 0:
            return None
        return p.value

    def set_watch(self, geom: int, body: int) -> None:
        _lib.check(_lib.load().dx_set_watch(self.ptr, geom, body))

    def jac_site(self, sites, rotational: bool = True):
        """mj_jacSite for every env at its current qpos (utils/mujoco_utils.py:38-73,
        compute_object_6d_jacobian): (jacp, jacr) of shape [B, nsite, 3, nv]."""
        s = np.ascontiguousarray(sites, dtype=np.int32).reshape(-1)
        shape = (self.nenv, len(s), 3, self.model.nv)
        jp = np.empty(shape, np.float32)
        jr = np.empty(shape, np.float32) if rotational else None
        _lib.check(_lib.load().dx_jac_site(self.ptr, s.ctypes.data, len(s), jp.ctypes.data,
                                           None if jr is None else jr.ctypes.data))
        return jp, jr

    def jac_object(self, types, ids, rotational: bool = True):
        """mj_jacBody / mj_jacGeom / mj_jacSite for every env at its current qpos
        (utils/mujoco_utils.py:38-73, compute_object_6d_jacobian, for the object types of
        controllers/mapper.py:60-64): types are `_lib.OBJ_BODY` / `OBJ_GEOM` / `OBJ_SITE`
        per object; (jacp, jacr) of shape [B, nobj, 3, nv]."""
        t = np.ascontiguousarray(types, dtype=np.int32).reshape(-1)
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if len(t) != len(i):
            raise ValueError("one object type per object id")
        shape = (self.nenv, len(i), 3, self.model.nv)
        jp = np.empty(shape, np.float32)
        jr = np.empty(shape, np.float32) if rotational else None
        _lib.check(_lib.load().dx_jac_object(self.ptr, t.ctypes.data, i.ctypes.data, len(i), jp.ctypes.data,
                                             None if jr is None else jr.ctypes.data))
        return jp, jr

    def enable_sensors(self, enable: bool = True) -> None:
        """Joint torque sensors (DX_SENSOR_TORQUE) computed by every step / forward."""
        _lib.check(_lib.load().dx_sensor_enable(self.ptr, int(enable)))

    def joint_torques(self, joints, axes) -> np.ndarray:
        """`DexterousHandObservables.joint_torques` (dexterous_hand.py:266-275): each
        joint's 3-axis torque sensor (a site at its body origin) projected on the
        joint axis; joints are (body id) per joint, axes [njoint, 3] in the body frame."""
        s = self.get(_lib.SENSOR_TORQUE).reshape(self.nenv, -1, 3)
        bodies = np.asarray(joints, dtype=int)
        return np.einsum("ejk,jk->ej", s[:, bodies, :], np.asarray(axes, dtype=np.float64))

    def enable_contact_forces(self, enable: bool = True) -> None:
        """Contact force sensing (include/dx.h dx_contact_enable): every step / forward then
        also writes DX_CFRC_EXT and, for the pads of `set_contact_pads`, DX_PAD_FORCE."""
        _lib.check(_lib.load().dx_contact_enable(self.ptr, int(enable)))

    def set_contact_pads(self, bodies, partners=-1) -> None:
        """The pads of DX_PAD_FORCE: pad k reports the force that contacts with body
        `partners[k]` (-1: any body; one value serves every pad) exert on `bodies[k]`, in
        that body's frame.  An empty list clears them; at most 64."""
        b = np.asarray(bodies, dtype=np.int32).reshape(-1)
        pads = np.empty((len(b), 2), dtype=np.int32)
        pads[:, 0] = b
        pads[:, 1] = np.broadcast_to(np.asarray(partners, dtype=np.int32), b.shape)
        _lib.check(_lib.load().dx_contact_set_pads(self.ptr, pads.ctypes.data if len(b) else None, len(b)))

    def cfrc_ext(self) -> np.ndarray:
        """MuJoCo's `cfrc_ext` of every env, [B, nbody, 6]: per body the torque about the
        subtree com of its tree root, then the force, world axes (DX_CFRC_EXT)."""
        return self.get(_lib.CFRC_EXT).reshape(self.nenv, -1, 6)

    def pad_forces(self) -> np.ndarray:
        """[B, npad, 3]: each pad's contact force in its body's frame (DX_PAD_FORCE)."""
        npad = _lib.check(_lib.load().dx_contact_npad(self.ptr))
        out = np.zeros((self.nenv, npad, 3), dtype=np.float32)
        if npad:
            _lib.check(_lib.load().dx_get_field(self.ptr, _lib.PAD_FORCE, out.ctypes.data, 0, self.nenv))
        return out

    # ------------------------------------------------------------------ #
    # depth / segmentation cameras and batched rays (include/dx.h dx_render_set_cameras)
    def set_cameras(self, configs, width: int, height: int, depth: bool = True, segmentation: bool = False,
                    near: float = 0.01, far: float = 10.0, cull: bool = True, rgb: bool = False) -> None:
        """The cameras `render()` casts: CameraConfigs or names of the five of
        `dexterity_amd.cameras` (an empty list switches them off).  Depth is the distance
        along the optical axis in metres, `far` on a miss; segmentation the geom id, -1 on a
        miss; rgb the shaded uint8 image (`set_shading`; include/dx.h "Shaded RGB").
        `cull=False` renders without the per-tile geom culls (the same images).  Bad
        options raise ValueError before any library call."""
        cfgs = cameras_lib.resolve(configs)
        L = _lib.load()
        if not cfgs:
            _lib.check(L.dx_render_set_cameras(self.ptr, None, 0, 0, 0, 0))
            self._cameras = ()
            return
        bodies = cameras_lib.validate(cfgs, width, height, depth, segmentation, near, far, self.nenv,
                                      self.model.compiled.names["body"], rgb=rgb)
        arr = (_lib.Camera * len(cfgs))()
        for c, cfg, body in zip(arr, cfgs, bodies):
            c.pos[:] = [float(v) for v in cfg.pos]
            c.xyaxes[:] = [float(v) for v in cfg.xyaxes]
            c.fovy, c.near_, c.far_, c.body = float(cfg.fovy), float(near), float(far), body
        flags = (_lib.RENDER_DEPTH if depth else 0) | (_lib.RENDER_SEGMENTATION if segmentation else 0) | \
            (0 if cull else _lib.RENDER_NO_CULL) | (_lib.RENDER_RGB if rgb else 0)
        _lib.check(L.dx_render_set_cameras(self.ptr, arr, len(cfgs), int(width), int(height), flags))
        self._cameras = tuple(cfgs)
        self._camera_shape = (self.nenv, len(cfgs), int(height), int(width))

    def render(self) -> None:
        """Renders the current poses (after `step()` or `forward()`) on the batch's stream."""
        _lib.check(_lib.load().dx_render(self.ptr))

    def _image(self, which: int, dtype) -> np.ndarray:
        if not getattr(self, "_cameras", ()):
            raise _lib.DxError("no cameras (set_cameras)")
        out = np.empty(self._camera_shape, dtype=dtype)
        _lib.check(_lib.load().dx_render_get(self.ptr, which, out.ctypes.data, 0, self.nenv))
        return out

    def depth(self) -> np.ndarray:
        """[B, ncam, H, W] float32 host copy of the last render's depth images."""
        return self._image(_lib.RENDER_DEPTH, np.float32)

    def segmentation(self) -> np.ndarray:
        """[B, ncam, H, W] int32 host copy of the last render's geom ids (-1: none)."""
        return self._image(_lib.RENDER_SEGMENTATION, np.int32)

    def set_shading(self, geom_rgb=None, box_faces=None, lights=None, shading=None) -> None:
        """The settings of the shaded RGB images (include/dx.h dx_render_set_shading); they
        persist across `set_cameras`.  geom_rgb [ngeom, 3] linear colours; box_faces {box geom
        id: [6, 3]} face colours in the order +x, -x, +y, -y, +z, -z; lights a sequence of
        `cameras.Light` (at most 4); shading a `cameras.Shading`.  None is that part's default
        (`cameras.default_palette`, `DEFAULT_LIGHTS`, `DEFAULT_SHADING`).  Bad settings raise
        ValueError before any library call."""
        cm = self.model.compiled
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
        _lib.check(_lib.load().dx_render_set_shading(self.ptr, *args))
        del keep

    def rgb(self) -> np.ndarray:
        """[B, ncam, H, W, 3] uint8 host copy of the last render's shaded images."""
        if not getattr(self, "_cameras", ()):
            raise _lib.DxError("no cameras (set_cameras)")
        out = np.empty(self._camera_shape + (3,), dtype=np.uint8)
        _lib.check(_lib.load().dx_render_get(self.ptr, _lib.RENDER_RGB, out.ctypes.data, 0, self.nenv))
        return out

    def shadow_stats(self):
        """(survivors summed, their maximum, passes) of the shading pass's shadow cull since the
        last call: the geoms per pixel tile and shadow-casting light that survive it
        (`render_stats` switches the counting on)."""
        out = (ctypes.c_uint64 * 3)()
        _lib.check(_lib.load().dx_render_stats2(self.ptr, out))
        return tuple(int(v) for v in out)

    def image_ptr(self, which: int) -> int:
        """Device address of the depth (`_lib.RENDER_DEPTH`), segmentation or RGB
        (`_lib.RENDER_RGB`) images."""
        p = ctypes.c_void_p()
        _lib.check(_lib.load().dx_render_output(self.ptr, which, ctypes.byref(p)))
        return p.value

    def render_stats(self, enable: bool = True):
        """(survivors summed, their maximum, tiles) of the renders since the last call: the
        geoms per pixel tile that survive the cull.  `enable` switches the counting."""
        out = (ctypes.c_uint64 * 3)()
        _lib.check(_lib.load().dx_render_stats(self.ptr, int(enable), out))
        return tuple(int(v) for v in out)

    def ray(self, origins, dirs):
        """A batched mj_ray at the current poses: origins / dirs [B, nray, 3] (world frame;
        dirs need not be normalised) -> (dist [B, nray] float32 along the normalised dir,
        geom [B, nray] int32); a miss is -1 / -1."""
        o = np.ascontiguousarray(origins, dtype=np.float32)
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        if o.ndim != 3 or o.shape[0] != self.nenv or o.shape[2] != 3 or d.shape != o.shape or o.shape[1] < 1:
            raise ValueError(f"origins and dirs must both be [{self.nenv}, nray, 3], got {o.shape} and {d.shape}")
        dist = np.empty(o.shape[:2], np.float32)
        geom = np.empty(o.shape[:2], np.int32)
        _lib.check(_lib.load().dx_ray(self.ptr, o.ctypes.data, d.ctypes.data, o.shape[1], dist.ctypes.data,
                                      geom.ctypes.data))
        return dist, geom

    def debug(self, enable: bool = True) -> None:
        _lib.check(_lib.load().dx_debug_enable(self.ptr, int(enable)))

    def health(self) -> dict:
        """The always-on health counters (include/dx.h dx_health): capacity overflows,
        diverged env-substeps, the most contacts one env-substep found and, when
        `ncon_histogram(True)` is on, the histogram of contacts per env-substep."""
        out = np.zeros(_lib.HEALTH_WORDS + _lib.NCON_HIST, dtype=np.uint32)
        _lib.check(_lib.load().dx_health(self.ptr, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out.size))
        h = {k: int(out[i]) for i, k in enumerate(_lib.HEALTH)}
        h["ncon_hist"] = out[_lib.HEALTH_WORDS:].astype(np.int64)
        return h

    def health_clear(self) -> None:
        _lib.check(_lib.load().dx_health_clear(self.ptr))

    def ncon_histogram(self, enable: bool = True) -> None:
        _lib.check(_lib.load().dx_ncon_histogram(self.ptr, int(enable)))

    def debug_get(self, name: str) -> np.ndarray:
        nv = self.model.nv
        sizes = {
            "qacc_smooth": (self.nenv, nv),
            "qfrc_smooth": (self.nenv, nv),
            "M": (self.nenv, nv, nv),
            "contact": (self.nenv, self.model.ncon_max, 16),
            "efc_count": (self.nenv, 2),
        }
        if name in ("queue_timeouts", "queue_slots"):
            out = np.zeros(1, dtype=np.int32)
            _lib.check(_lib.load().dx_debug_get(self.ptr, name.encode(), out.ctypes.data, 1))
            return out
        if name in ("bp_sizes", "bp_item", "bp_cull"):
            # the body-pair cull's host tables (dx_model.hip): {nbitem, nbplane, nbpair}, the
            # distinct planes and spheres [nbitem][8], a pair's items and margin [nbpair][2]
            out = np.zeros(3, dtype=np.int32)
            _lib.check(_lib.load().dx_debug_get(self.ptr, b"bp_sizes", out.ctypes.data, 3))
            if name == "bp_sizes":
                return out
            out = np.zeros((out[0], 8), np.float32) if name == "bp_item" else np.zeros((out[2], 2), np.int32)
            _lib.check(_lib.load().dx_debug_get(self.ptr, name.encode(), out.ctypes.data, out.size))
            return out
        shape = sizes[name]
        out = np.empty(shape, dtype=np.float32)
        _lib.check(_lib.load().dx_debug_get(self.ptr, name.encode(), out.ctypes.data, out.size))
        if name == "efc_count":
            return out.view(np.int32)
        return out

    # convenience views (host copies)
    @property
    def qpos(self) -> np.ndarray:
        return self.get(_lib.QPOS)

    @property
    def qvel(self) -> np.ndarray:
        return self.get(_lib.QVEL)

    @property
    def qacc(self) -> np.ndarray:
        return self.get(_lib.QACC)


def gravity_compensation(compiled: CompiledModel, prefix: str) -> np.ndarray:
    """xfrc_applied rows = -m_b g for bodies whose name starts with prefix.

    utils/mujoco_utils.py:91-99 (called from shadow_hand_e.py:35-41 and
    adroit_hand.py:30-36 in initialize_episode).
    """
    xfrc = np.zeros((compiled.nbody, 6))
    for i, n in enumerate(compiled.names["body"]):
        if n.startswith(prefix):
            xfrc[i, :3] = -compiled.gravity * compiled.body_mass[i]
    return xfrc
