"""Camera configurations and the pinhole model of the device ray cast (include/dx.h
dx_render_set_cameras; csrc/dx_render.hip).

The reference adds world-fixed cameras to the arena from five named configurations
(manipulation/shared/cameras.py:22-50) and observes them at 84 x 84 with optional `depth`
and `segmentation` (manipulation/shared/observations.py:62-74).  Here a camera may also be
attached to a body (`body`, a name or an id: a palm camera), `pos` / `xyaxes` then being
in that body's frame.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np

MAX_CAMERAS = 8      # DX_RENDER_MAX_CAMERAS
MAX_SIDE = 512       # DX_RENDER_MAX_SIDE
RENDER_DEPTH, RENDER_SEGMENTATION, RENDER_NO_CULL = 1, 2, 4  # dx_render_set_cameras flags
RENDER_RGB = 8
MAX_LIGHTS = 4       # DX_RENDER_MAX_LIGHTS
MAX_FACE_GEOMS = 8   # DX_RENDER_MAX_FACE_GEOMS
OBJ_GEOM = 5         # mjOBJ_GEOM, the object type of a segmentation pixel
GEOM_BOX = 6         # mjGEOM_BOX


@dataclasses.dataclass(frozen=True)
class CameraConfig:
    """cameras.py:13-17, plus MuJoCo's `fovy` (degrees, default 45) and an optional body."""

    name: str
    pos: Tuple[float, float, float]
    xyaxes: Tuple[float, float, float, float, float, float]
    fovy: float = 45.0
    body: Optional[Union[str, int]] = None


# manipulation/shared/cameras.py:22-50
FRONT_CLOSE = CameraConfig(name="front_close", pos=(0.0, -0.5, 0.5), xyaxes=(1.0, 0.0, 0.0, 0.0, 0.7, 0.75))
LEFT_CLOSE = CameraConfig(name="left_close", pos=(-0.6, 0.0, 0.5), xyaxes=(0.0, -1.0, 0.0, 0.7, 0.0, 0.75))
RIGHT_CLOSE = CameraConfig(name="right_close", pos=(0.6, 0.0, 0.5), xyaxes=(0.0, 1.0, 0.0, -0.7, 0.0, 0.75))
FRONT_FAR = CameraConfig(name="front_far", pos=(0.0, -1.0, 0.7), xyaxes=(1.0, 0.0, 0.0, 0.0, 0.7, 0.75))
TOP_DOWN = CameraConfig(name="top_down", pos=(0.0, 0.0, 2.5), xyaxes=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
CAMERAS = {c.name: c for c in (FRONT_CLOSE, LEFT_CLOSE, RIGHT_CLOSE, FRONT_FAR, TOP_DOWN)}


def camera_frame(xyaxes) -> np.ndarray:
    """[3, 3] rows x, y, z of the camera frame ([3P] MuJoCo's xyaxes): x normalised, y made
    orthogonal to x and normalised, z = x (x) y.  The camera looks along -z.  ValueError
    for degenerate axes."""
    a = np.asarray(xyaxes, dtype=np.float64).reshape(-1)
    if a.shape != (6,) or not np.all(np.isfinite(a)):
        raise ValueError(f"xyaxes must be six finite numbers, got {xyaxes!r}")
    x, y = a[:3].copy(), a[3:].copy()
    nx = np.linalg.norm(x)
    if not nx > 1e-10:
        raise ValueError(f"degenerate xyaxes {xyaxes!r}: the x axis has no length")
    x /= nx
    y -= np.dot(x, y) * x
    ny = np.linalg.norm(y)
    if not ny > 1e-10:
        raise ValueError(f"degenerate xyaxes {xyaxes!r}: the y axis is parallel to the x axis")
    y /= ny
    return np.stack([x, y, np.cross(x, y)])


def focal_length(fovy: float, height: int) -> float:
    """f = 0.5 H / tan(fovy / 2) in pixels, fovy the vertical field of view in degrees."""
    return 0.5 * height / math.tan(0.5 * math.radians(fovy))


def camera_rays(config: CameraConfig, width: int, height: int):
    """The pinhole model in numpy (fp64): (origin [3], directions [H, W, 3]) in the frame
    `pos` / `xyaxes` are given in.  Pixel (r, c), row 0 on top, has its centre at
    (c + 0.5, r + 0.5) and the direction
        x (c + 0.5 - W/2) / f - y (r + 0.5 - H/2) / f - z,
    not normalised: a hit's ray parameter is its depth along the optical axis."""
    x, y, z = camera_frame(config.xyaxes)
    f = focal_length(config.fovy, height)
    u = (np.arange(width) + 0.5 - 0.5 * width) / f
    v = (np.arange(height) + 0.5 - 0.5 * height) / f
    d = x[None, None, :] * u[None, :, None] - y[None, None, :] * v[:, None, None] - z[None, None, :]
    return np.asarray(config.pos, dtype=np.float64), d


def resolve(configs_or_names) -> list:
    """A list of CameraConfig from configs and / or the names of the five above."""
    if isinstance(configs_or_names, (str, CameraConfig)):
        configs_or_names = [configs_or_names]
    out = []
    for c in configs_or_names:
        if isinstance(c, str):
            if c not in CAMERAS:
                raise ValueError(f"unknown camera {c!r}; the named ones are {sorted(CAMERAS)}")
            c = CAMERAS[c]
        if not isinstance(c, CameraConfig):
            raise ValueError(f"a camera is a CameraConfig or one of the names {sorted(CAMERAS)}, got {c!r}")
        out.append(c)
    return out


# --------------------------------------------------------------------------- #
# shaded RGB (include/dx.h "Shaded RGB": the shading model; dx_render_set_shading)
# --------------------------------------------------------------------------- #
@dataclasses.dataclass(frozen=True)
class Light:
    """struct dx_light: a directional light shines along `dir` from infinitely far, a
    positional one from `pos`; `diffuse` is its linear RGB strength."""

    pos: Tuple[float, float, float] = (0.0, 0.0, 1.0)
    dir: Tuple[float, float, float] = (0.0, 0.0, -1.0)
    diffuse: Tuple[float, float, float] = (0.5, 0.5, 0.5)
    directional: bool = True
    castshadow: bool = True


@dataclasses.dataclass(frozen=True)
class Shading:
    """struct dx_shading.  `headlight` is the diffuse strength of a light along the camera's
    +z axis that casts no shadow (all 0: off); `checker_cell` (metres, 0: off) paints plane
    geoms with `checker_rgb` by the parity of the cell."""

    ambient: Tuple[float, float, float] = (0.2, 0.2, 0.2)
    background: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    headlight: Tuple[float, float, float] = (0.3, 0.3, 0.3)
    checker_rgb: Tuple[Tuple[float, float, float], Tuple[float, float, float]] = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    checker_cell: float = 0.0


# The library's defaults (dx_render_set_shading with NULLs; dx_query.hip mirrors the values).
# The reference arena declares one directional light straight down that casts shadows
# (models/arenas/arena.py:30-38), and MuJoCo's headlight is on by default.  Strengths: ambient
# 0.2 + light 0.5 + headlight 0.3 = 1, so a surface facing both is exactly white-limited and
# nothing saturates; the shadowed ground keeps 0.2 + 0.3 n.z of the headlight.
DEFAULT_LIGHTS = (Light(),)
DEFAULT_SHADING = Shading()
PALETTE_WORLD = (0.45, 0.45, 0.5)
PALETTE_HANDS = ((0.85, 0.65, 0.5), (0.5, 0.65, 0.85))
PALETTE_PROP = (0.8, 0.8, 0.8)
PALETTE_FACES = ((0.9, 0.1, 0.1), (0.1, 0.8, 0.1), (0.1, 0.2, 0.9),   # +x, -x, +y,
                 (0.9, 0.8, 0.1), (0.9, 0.1, 0.9), (0.1, 0.8, 0.8))   # -y, +z, -z


def default_palette(compiled):
    """(geom_rgb [ngeom, 3] float32, box_faces {geom id: [6, 3]}) from the compiled model's
    own tables: the world body's geoms PALETTE_WORLD; the geoms of each hand -- a kinematic
    tree whose root has no free joint, in the order the geoms meet them -- PALETTE_HANDS in
    turn; a free-jointed prop's geoms PALETTE_PROP, and the first box among them the six
    PALETTE_FACES."""
    gb = np.asarray(compiled.geom_bodyid, dtype=np.int64)
    gt = np.asarray(compiled.geom_type, dtype=np.int64)
    root = np.asarray(compiled.body_rootid, dtype=np.int64)
    free = {int(root[b]) for t, b in zip(np.asarray(compiled.jnt_type), np.asarray(compiled.jnt_bodyid)) if int(t) == 0}
    rgb = np.zeros((len(gb), 3), np.float32)
    hands, faces = [], {}
    for g, b in enumerate(gb):
        r = int(root[b])
        if b == 0:
            rgb[g] = PALETTE_WORLD
        elif r in free:
            rgb[g] = PALETTE_PROP
            if gt[g] == GEOM_BOX and not faces:
                faces[g] = np.asarray(PALETTE_FACES, np.float32)
        else:
            if r not in hands:
                hands.append(r)
            rgb[g] = PALETTE_HANDS[hands.index(r) % 2]
    return rgb, faces


def _triple(value, what):
    a = np.asarray(value, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.all(np.isfinite(a)):
        raise ValueError(f"{what} must be three finite numbers, got {value!r}")
    return a


def validate_shading(geom_rgb, box_faces, lights, shading, geom_types) -> tuple:
    """Checks the shading settings before any library call (ValueError with the reason) and
    returns them in the library's shapes: (geom_rgb [ngeom, 3] float32 or None, face geoms
    [nface] int32, face_rgb [nface, 6, 3] float32, lights tuple, shading).  None stands for
    the library's default of that part."""
    ngeom = len(geom_types)
    if geom_rgb is not None:
        a = np.asarray(geom_rgb, dtype=np.float32)
        if a.shape != (ngeom, 3):
            raise ValueError(f"geom_rgb must have the shape [ngeom, 3] = [{ngeom}, 3], got {list(a.shape)}")
        if not np.all(np.isfinite(a)):
            raise ValueError("geom_rgb holds a non-finite value")
        geom_rgb = np.ascontiguousarray(a)
    face_geom = face_rgb = None
    if box_faces is not None:
        if len(box_faces) > MAX_FACE_GEOMS:
            raise ValueError(f"{len(box_faces)} geoms with face colours: at most {MAX_FACE_GEOMS}")
        face_geom = np.zeros(len(box_faces), np.int32)
        face_rgb = np.zeros((len(box_faces), 6, 3), np.float32)
        for k, (g, c) in enumerate(box_faces.items()):
            if int(g) != g or not 0 <= int(g) < ngeom or int(geom_types[int(g)]) != GEOM_BOX:
                raise ValueError(f"box_faces: geom {g!r} is not a box geom")
            c = np.asarray(c, dtype=np.float32)
            if c.shape != (6, 3) or not np.all(np.isfinite(c)):
                raise ValueError(f"box_faces[{g}] must be six finite RGB triples [6, 3], got {list(c.shape)}")
            face_geom[k], face_rgb[k] = int(g), c
    if lights is not None:
        lights = tuple(lights)
        if len(lights) > MAX_LIGHTS:
            raise ValueError(f"{len(lights)} lights: at most {MAX_LIGHTS}")
        for i, l in enumerate(lights):
            if not isinstance(l, Light):
                raise ValueError(f"light {i} is not a cameras.Light: {l!r}")
            _triple(l.pos, f"light {i}: pos")
            _triple(l.diffuse, f"light {i}: diffuse")
            if l.directional and not np.linalg.norm(_triple(l.dir, f"light {i}: dir")) > 0.0:
                raise ValueError(f"light {i}: a directional light needs a dir that is not zero")
            _triple(l.dir, f"light {i}: dir")
    if shading is not None:
        if not isinstance(shading, Shading):
            raise ValueError(f"shading is not a cameras.Shading: {shading!r}")
        for name in ("ambient", "background", "headlight"):
            _triple(getattr(shading, name), f"shading.{name}")
        c = np.asarray(shading.checker_rgb, dtype=np.float64)
        if c.shape != (2, 3) or not np.all(np.isfinite(c)):
            raise ValueError(f"shading.checker_rgb must be two finite RGB triples, got {shading.checker_rgb!r}")
        if not (math.isfinite(shading.checker_cell) and shading.checker_cell >= 0.0):
            raise ValueError(f"shading.checker_cell must be finite and not negative, got {shading.checker_cell}")
    return geom_rgb, face_geom, face_rgb, lights, shading


def validate(configs: Sequence[CameraConfig], width: int, height: int, depth: bool, segmentation: bool,
             near: float, far: float, num_envs: int, body_names: Sequence[str], rgb: bool = False) -> list:
    """Checks every option before any library call (ValueError with the reason) and returns
    the body id of each camera (-1: world-fixed)."""
    if len(configs) > MAX_CAMERAS:
        raise ValueError(f"{len(configs)} cameras: at most {MAX_CAMERAS}")
    names = [c.name for c in configs]
    if len(set(names)) != len(names):
        raise ValueError(f"camera names must differ, got {names}")
    if int(width) != width or int(height) != height or not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"width and height must be integers in [1, {MAX_SIDE}], got {width} x {height}")
    if not (depth or segmentation or rgb):
        raise ValueError("nothing to render: depth and segmentation are both off")
    if not (math.isfinite(near) and math.isfinite(far) and 0.0 < near < far):
        raise ValueError(f"need 0 < near < far, got near = {near}, far = {far}")
    if num_envs * max(len(configs), 1) * width * height >= 2**31:
        raise ValueError("num_envs * cameras * height * width reaches 2^31")
    bodies = []
    for c in configs:
        camera_frame(c.xyaxes)
        if len(c.pos) != 3 or not all(math.isfinite(p) for p in c.pos):
            raise ValueError(f"camera {c.name!r}: pos must be three finite numbers, got {c.pos!r}")
        if not (math.isfinite(c.fovy) and 0.0 < c.fovy < 180.0):
            raise ValueError(f"camera {c.name!r}: fovy must be in (0, 180) degrees, got {c.fovy}")
        if c.body is None:
            bodies.append(-1)
        elif isinstance(c.body, str):
            if c.body not in body_names:
                raise ValueError(f"camera {c.name!r}: no body named {c.body!r}")
            bodies.append(list(body_names).index(c.body))
        else:
            if not 0 <= int(c.body) < len(body_names):
                raise ValueError(f"camera {c.name!r}: body {c.body} outside [0, {len(body_names)})")
            bodies.append(int(c.body))
    return bodies
