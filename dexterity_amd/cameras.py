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
OBJ_GEOM = 5         # mjOBJ_GEOM, the object type of a segmentation pixel


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


def validate(configs: Sequence[CameraConfig], width: int, height: int, depth: bool, segmentation: bool,
             near: float, far: float, num_envs: int, body_names: Sequence[str]) -> list:
    """Checks every option before any library call (ValueError with the reason) and returns
    the body id of each camera (-1: world-fixed)."""
    if len(configs) > MAX_CAMERAS:
        raise ValueError(f"{len(configs)} cameras: at most {MAX_CAMERAS}")
    names = [c.name for c in configs]
    if len(set(names)) != len(names):
        raise ValueError(f"camera names must differ, got {names}")
    if int(width) != width or int(height) != height or not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"width and height must be integers in [1, {MAX_SIDE}], got {width} x {height}")
    if not (depth or segmentation):
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
