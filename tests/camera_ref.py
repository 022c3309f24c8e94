"""Reference ray cast for the depth / segmentation cameras and dx_ray (include/dx.h
dx_render_set_cameras; dexterity_amd/csrc/dx_render.hip) -- TEST INFRASTRUCTURE ONLY.

`cast` is fp64 numpy, independent of the kernel's arithmetic: geom poses from the fp64
oracle (geom_xpos / geom_xmat after kinematics()), hulls as scipy's ConvexHull equations of
mesh_vert, rays from dexterity_amd.cameras.camera_rays, world-frame rays moved into each
geom's frame, the textbook quadratic for spheres.

`unstable` recasts with the ray directions, geom positions and rotation entries jittered
by +-16 eps32 (1.9e-6), four draws from a fixed seed: a pixel is unstable when the
reference's own geom id changes in any draw (a silhouette pixel: either answer is right).

`cast32` restates the kernel's arithmetic in float32 numpy (body pose -> geom pose, the
camera moved into the geom frame, closest-approach spheres, slabs, half-space clipping
against the LIBRARY's planes): its worst depth error against `cast` on stable pixels is the
e32 of the GPU tests' tolerance 4 max(e32, 16 eps32 depth).
"""

import functools

import numpy as np

from dexterity_amd import cameras as cameras_lib

PLANE, SPHERE, CAPSULE, BOX, MESH = 0, 2, 3, 6, 7
EPS32 = float(np.finfo(np.float32).eps)
JITTER = 16 * EPS32
INF = np.inf

# the GPU tests' cameras (the reorient scene: the hand near the origin, palm up, the cube
# above it)
NEAR_TOP = cameras_lib.CameraConfig("near_top", (-0.02, -0.02, 0.55), (1, 0, 0, 0, 1, 0))
NEAR_FRONT = cameras_lib.CameraConfig("near_front", (0.0, -0.42, 0.30), (1, 0, 0, 0, 0.5, 0.87))
SIZES = ((32, 24), (19, 13))  # (width, height): no multiples of the 16-pixel tile
NEAR, FAR = 0.01, 10.0


def hull_equations(cm):
    """Per hull [nfacet, 4] scipy ConvexHull equations (n, d; n x + d <= 0 inside)."""
    key = id(cm)
    if key not in _HULLS:
        from scipy.spatial import ConvexHull

        V = np.asarray(cm.mesh_vert, dtype=np.float64).reshape(-1, 3)
        out = []
        for a, n in zip(cm.mesh_vertadr, cm.mesh_vertnum):
            out.append(np.array(ConvexHull(V[a:a + n]).equations, dtype=np.float64))
        _HULLS[key] = (cm, out)
    return _HULLS[key][1]


_HULLS = {}


def oracle_state(oracle_mod, cm, qpos):
    """(geom_xpos [ngeom, 3], geom_xmat [ngeom, 3, 3], xpos [nbody, 3], xquat [nbody, 4]) of
    the fp64 oracle at qpos."""
    from dexterity_amd import blob as blob_lib

    om = _oracle_model(oracle_mod, cm)
    d = oracle_mod.OracleData(om)
    d.reset()
    d.qpos[:] = qpos
    d.kinematics()
    return (d.geom_xpos.reshape(-1, 3).copy(), d.geom_xmat.reshape(-1, 3, 3).copy(),
            d.xpos.reshape(-1, 3).copy(), d.xquat.reshape(-1, 4).copy())


def _oracle_model(oracle_mod, cm):
    from dexterity_amd import blob as blob_lib

    key = id(cm)
    if key not in _OMODELS:
        _OMODELS[key] = (cm, oracle_mod.OracleModel(blob_lib.pack(cm.arrays)))
    return _OMODELS[key][1]


_OMODELS = {}


def quat_to_mat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def world_rays(config, width, height, xpos=None, xquat=None, body=-1):
    """(origin [3], dirs [H*W, 3]) of a camera in the world; a body camera through the
    oracle's body pose."""
    o, d = cameras_lib.camera_rays(config, width, height)
    d = d.reshape(-1, 3)
    if body is not None and body >= 0:
        R = quat_to_mat(xquat[body])
        return xpos[body] + R @ o, d @ R.T
    return o, d


# --------------------------------------------------------------------------- #
# the fp64 reference
# --------------------------------------------------------------------------- #
def _entry(cm, hulls, g, o, d):
    """Entry parameter [n] of the lines o + t d (geom g's frame) into geom g; inf: a miss."""
    typ = int(cm.geom_type[g])
    size = np.asarray(cm.geom_size, dtype=np.float64).reshape(-1, 3)[g]
    n = len(d)
    if typ == PLANE:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[:, 2] / d[:, 2]
        return np.where((d[:, 2] < 0) & (o[:, 2] > 0), t, INF)
    if typ in (MESH, BOX):
        if typ == MESH:
            E = hulls[int(cm.geom_dataid[g])]
        else:
            E = np.zeros((6, 4))
            for k in range(3):
                E[2 * k, k], E[2 * k, 3] = 1.0, -size[k]
                E[2 * k + 1, k], E[2 * k + 1, 3] = -1.0, -size[k]
        den = d @ E[:, :3].T            # [n, nf]
        dist = o @ E[:, :3].T + E[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -dist / den
        tmin = np.max(np.where(den < 0, t, -INF), axis=1)
        tmax = np.min(np.where(den > 0, t, INF), axis=1)
        out = np.any((den == 0) & (dist > 0), axis=1)
        return np.where((tmin <= tmax) & ~out, tmin, INF)

    def sphere(c, r):
        oc = o - c
        a = np.sum(d * d, axis=1)
        b = np.sum(oc * d, axis=1)
        cc = np.sum(oc * oc, axis=1) - r * r
        disc = b * b - a * cc
        with np.errstate(invalid="ignore"):
            return np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, INF)

    if typ == SPHERE:
        return sphere(np.zeros(3), size[0])
    if typ == CAPSULE:
        r, h = size[0], size[1]
        t = np.minimum(sphere(np.array([0, 0, h]), r), sphere(np.array([0, 0, -h]), r))
        a = d[:, 0] ** 2 + d[:, 1] ** 2
        b = o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]
        cc = o[:, 0] ** 2 + o[:, 1] ** 2 - r * r
        disc = b * b - a * cc
        with np.errstate(divide="ignore", invalid="ignore"):
            ts = (-b - np.sqrt(np.maximum(disc, 0))) / a
            ok = (disc >= 0) & (a > 0) & (np.abs(o[:, 2] + ts * d[:, 2]) <= h)
        return np.minimum(t, np.where(ok, ts, INF))
    return np.full(n, INF)


def bound_radius(cm):
    """[ngeom] a radius about each geom's frame origin that holds the geom, from the hull
    vertices and the primitive sizes (the reference's own: not the model's geom_bsphere, which
    the kernel's cull trusts); 0 for the plane."""
    key = id(cm)
    if key not in _RADII:
        V = np.asarray(cm.mesh_vert, dtype=np.float64).reshape(-1, 3)
        size = np.asarray(cm.geom_size, dtype=np.float64).reshape(-1, 3)
        r = np.zeros(int(cm.ngeom))
        for g in range(int(cm.ngeom)):
            typ = int(cm.geom_type[g])
            if typ == MESH:
                k = int(cm.geom_dataid[g])
                a, n = int(cm.mesh_vertadr[k]), int(cm.mesh_vertnum[k])
                r[g] = np.linalg.norm(V[a:a + n], axis=1).max()
            elif typ == BOX:
                r[g] = np.linalg.norm(size[g])
            elif typ == SPHERE:
                r[g] = size[g, 0]
            elif typ == CAPSULE:
                r[g] = size[g, 0] + size[g, 1]
        _RADII[key] = (cm, r)
    return _RADII[key][1]


_RADII = {}


def cast(cm, gpos, gmat, origins, dirs, near, far, skip=()):
    """Nearest geom entered at t in [near, far] along each world ray: (t [n] with inf for a
    miss, geom [n] with -1).  origins [3] or [n, 3]; the lower geom id wins a tie; the geoms
    in `skip` are left out of the scene."""
    hulls = hull_equations(cm)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    origins = np.broadcast_to(np.asarray(origins, dtype=np.float64), dirs.shape)
    best = np.full(len(dirs), INF)
    geom = np.full(len(dirs), -1, dtype=np.int32)
    rad = bound_radius(cm)
    dn = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    for g in range(int(cm.ngeom)):
        if g in skip:
            continue
        R = gmat[g]
        sel = slice(None)
        if int(cm.geom_type[g]) != PLANE:
            # only the rays that pass within 1.05 r + 1 mm of the geom's frame origin, r from
            # the vertices and sizes (the reference's own shortcut, far wider than any rounding)
            v = gpos[g] - origins
            perp = np.linalg.norm(v - np.sum(v * dn, axis=1, keepdims=True) * dn, axis=1)
            sel = np.nonzero(perp <= 1.05 * rad[g] + 1e-3)[0]
            if not len(sel):
                continue
        t = _entry(cm, hulls, g, (origins[sel] - gpos[g]) @ R, dirs[sel] @ R)
        hit = (t >= near) & (t <= far) & (t < best[sel])
        best[sel] = np.where(hit, t, best[sel])
        geom[sel] = np.where(hit, g, geom[sel])
    return best, geom


def unstable(cm, gpos, gmat, origins, dirs, near, far, geom, seed=0, skip=()):
    """[n] bool: the reference's geom id changes under a +-16 eps32 jitter (four draws)."""
    rng = np.random.RandomState(seed)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    bad = np.zeros(len(dirs), dtype=bool)
    for _ in range(4):
        d2 = dirs + rng.uniform(-JITTER, JITTER, dirs.shape)
        p2 = gpos + rng.uniform(-JITTER, JITTER, gpos.shape)
        m2 = gmat + rng.uniform(-JITTER, JITTER, gmat.shape)
        _, g2 = cast(cm, p2, m2, origins, d2, near, far, skip)
        bad |= g2 != geom
    return bad


# --------------------------------------------------------------------------- #
# the kernel's arithmetic in float32
# --------------------------------------------------------------------------- #
F = np.float32


def _q2m32(q):
    w, x, y, z = [F(v) for v in q]
    one, two = F(1), F(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=F)


def _sphere32(o, d, inv_a, cz, r2):
    oz = o[:, 2] - F(cz)
    tc = -(o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1] + oz * d[:, 2]) * inv_a
    px, py, pz = o[:, 0] + tc * d[:, 0], o[:, 1] + tc * d[:, 1], oz + tc * d[:, 2]
    perp2 = px * px + py * py + pz * pz
    with np.errstate(invalid="ignore"):
        return np.where(perp2 <= r2, tc - np.sqrt(np.maximum((r2 - perp2) * inv_a, F(0))), F(INF)).astype(F)


def _entry32(cm, planes, g, o, d):
    typ = int(cm.geom_type[g])
    size = np.asarray(cm.geom_size, dtype=np.float64).reshape(-1, 3)[g].astype(F)
    n = len(d)
    a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(F)
    inv_a = (F(1) / a).astype(F)
    if typ == PLANE:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((d[:, 2] < 0) & (o[:, 2] > 0), -o[:, 2] / d[:, 2], F(INF)).astype(F)
    if typ == MESH:
        P = np.asarray(planes[int(cm.geom_dataid[g])], dtype=F)  # [np, 4]; rays x planes below
        den = (P[None, :, 0] * d[:, None, 0] + P[None, :, 1] * d[:, None, 1] + P[None, :, 2] * d[:, None, 2]).astype(F)
        dist = (P[None, :, 0] * o[:, None, 0] + P[None, :, 1] * o[:, None, 1] + P[None, :, 2] * o[:, None, 2]
                + P[None, :, 3]).astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (-dist / den).astype(F)
        tmin = np.max(np.where(den < 0, t, F(-INF)), axis=1, initial=F(-INF))
        tmin = np.where(np.any((den == 0) & (dist > 0), axis=1), F(INF), tmin).astype(F)
        tmax = np.min(np.where(den > 0, t, F(INF)), axis=1, initial=F(INF)).astype(F)
        with np.errstate(invalid="ignore"):
            thick = (tmax - tmin) > F(8) * F(EPS32) * np.maximum(np.abs(tmin), np.abs(tmax))
        return np.where(thick, tmin, F(INF)).astype(F)
    if typ == BOX:
        tmin, tmax = np.full(n, -INF, dtype=F), np.full(n, INF, dtype=F)
        for k in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = (F(1) / d[:, k]).astype(F)
                t1, t2 = ((-size[k] - o[:, k]) * inv).astype(F), ((size[k] - o[:, k]) * inv).astype(F)
            nz = d[:, k] != 0
            tmin = np.where(nz, np.maximum(tmin, np.minimum(t1, t2)),
                            np.where(np.abs(o[:, k]) > size[k], F(INF), tmin))
            tmax = np.where(nz, np.minimum(tmax, np.maximum(t1, t2)), tmax)
        return np.where(tmin <= tmax, tmin, F(INF)).astype(F)
    if typ == SPHERE:
        return _sphere32(o, d, inv_a, 0.0, size[0] * size[0])
    if typ == CAPSULE:
        r, h = size[0], size[1]
        r2 = r * r
        t = np.minimum(_sphere32(o, d, inv_a, h, r2), _sphere32(o, d, inv_a, -h, r2))
        a2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv_a2 = (F(1) / a2).astype(F)
            tc = -(o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]) * inv_a2
            px, py = o[:, 0] + tc * d[:, 0], o[:, 1] + tc * d[:, 1]
            perp2 = px * px + py * py
            ts = (tc - np.sqrt(np.maximum((r2 - perp2) * inv_a2, F(0)))).astype(F)
            ok = (a2 > F(1e-12) * a) & (perp2 <= r2) & (np.abs(o[:, 2] + ts * d[:, 2]) <= h)
        return np.minimum(t, np.where(ok, ts, F(INF))).astype(F)
    return np.full(n, INF, dtype=F)


def geom_poses32(cm, xpos, xquat):
    """The kernel's geom poses: fp32 body poses (the oracle's, rounded) times the model's
    geom_pos / geom_quat."""
    gq = np.asarray(cm.geom_quat, dtype=np.float64).reshape(-1, 4)
    gp = np.asarray(cm.geom_pos, dtype=np.float64).reshape(-1, 3).astype(F)
    P, M = [], []
    for g in range(int(cm.ngeom)):
        b = int(cm.geom_bodyid[g])
        Rb = _q2m32(xquat[b].astype(F)) if b > 0 else np.eye(3, dtype=F)
        xp = xpos[b].astype(F) if b > 0 else np.zeros(3, dtype=F)
        gm = quat_to_mat(gq[g] / np.linalg.norm(gq[g])).astype(F)
        M.append((Rb @ gm).astype(F))
        P.append((xp + Rb @ gp[g]).astype(F))
    return np.array(P, dtype=F), np.array(M, dtype=F)


def cast32(cm, planes, xpos, xquat, near, far, config=None, width=0, height=0, body=-1, origins=None, dirs=None):
    """The kernel's float32 arithmetic: a camera (config, width, height, body) or given
    world rays (origins / dirs [n, 3], dirs normalised here).  planes: the library's
    (Model.hull_planes) per hull.  Returns (t [n] float32 with inf for a miss, geom [n])."""
    P, M = geom_poses32(cm, xpos, xquat)
    if config is not None:
        frame = cameras_lib.camera_frame(config.xyaxes).astype(F)
        pos = np.asarray(config.pos, dtype=F)
        if body is not None and body >= 0:
            Rb = _q2m32(xquat[body].astype(F))
            co = (xpos[body].astype(F) + Rb @ pos).astype(F)
            cx, cy, cz = [(Rb @ frame[k]).astype(F) for k in range(3)]
        else:
            co, (cx, cy, cz) = pos, frame
        f = F(cameras_lib.focal_length(config.fovy, height))
        inv_f = F(1) / f
        u = ((np.arange(width, dtype=F) + F(0.5) - F(0.5) * F(width)) * inv_f).astype(F)
        v = ((np.arange(height, dtype=F) + F(0.5) - F(0.5) * F(height)) * inv_f).astype(F)
        U, V = np.meshgrid(u, v)
        U, V = U.reshape(-1, 1), V.reshape(-1, 1)
        n = U.shape[0]
    else:
        dirs = np.asarray(dirs, dtype=F).reshape(-1, 3)
        origins = np.asarray(origins, dtype=F).reshape(-1, 3)
        n2 = (dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1] + dirs[:, 2] * dirs[:, 2]).astype(F)
        dirs = (dirs * (F(1) / np.sqrt(n2))[:, None]).astype(F)
        n = len(dirs)
    best = np.full(n, INF, dtype=F)
    geom = np.full(n, -1, dtype=np.int32)
    rad = bound_radius(cm)
    for g in range(int(cm.ngeom)):
        R = M[g]
        if config is not None:
            ol = (R.T @ (co - P[g]).astype(F)).astype(F)
            ax, ay, az = (R.T @ cx).astype(F), (R.T @ cy).astype(F), (R.T @ cz).astype(F)
            d = (ax[None, :] * U - ay[None, :] * V - az[None, :]).astype(F)
            o = np.broadcast_to(ol, d.shape)
        else:
            o = ((origins - P[g]).astype(F) @ R).astype(F)
            d = (dirs @ R).astype(F)
        sel = np.arange(n)
        if int(cm.geom_type[g]) != PLANE:  # (the shortcut of `cast`, in the geom frame)
            o64, d64 = o.astype(np.float64), d.astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                tc = -np.sum(o64 * d64, axis=1) / np.sum(d64 * d64, axis=1)
            perp = np.linalg.norm(o64 + tc[:, None] * d64, axis=1)
            sel = np.nonzero(perp <= 1.05 * rad[g] + 1e-3)[0]
            if not len(sel):
                continue
        t = _entry32(cm, planes, g, o[sel], d[sel])
        hit = (t >= F(near)) & (t <= F(far)) & (t < best[sel])
        best[sel] = np.where(hit, t, best[sel])
        geom[sel] = np.where(hit, g, geom[sel])
    return best, geom


# --------------------------------------------------------------------------- #
# the states of the GPU tests
# --------------------------------------------------------------------------- #
def posed_qpos(cm, n, seed, prop_box=None):
    """[n, nq]: env 0 at qpos0; the others with every limited hinge joint uniform in the
    middle 60 % of its range and, with a free joint, the prop uniform in `prop_box`
    ((lo[3], hi[3])) at a uniform random orientation."""
    rng = np.random.RandomState(seed)
    out = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (n, 1))
    rng_rows = range(1, n)
    for e in rng_rows:
        for j in range(int(cm.njnt)):
            adr = int(cm.jnt_qposadr[j])
            if int(cm.jnt_type[j]) == 3 and int(cm.jnt_limited[j]):
                lo, hi = np.asarray(cm.jnt_range, dtype=np.float64).reshape(-1, 2)[j]
                out[e, adr] = rng.uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo))
            elif int(cm.jnt_type[j]) == 0 and prop_box is not None:
                out[e, adr:adr + 3] = rng.uniform(prop_box[0], prop_box[1])
                q = rng.normal(size=4)
                out[e, adr + 3:adr + 7] = q / np.linalg.norm(q)
    return out


def depth_bound(e32, depth):
    """The GPU tests' depth tolerance: 4 max(e32, 16 eps32 depth)."""
    return 4.0 * np.maximum(e32, 16 * EPS32 * np.abs(depth))


@functools.lru_cache(maxsize=None)
def library_planes(asset):
    """The library's plane table of an asset, per hull (no GPU)."""
    from dexterity_amd import physics as physics_lib

    m = physics_lib.Model.from_file(asset)
    return tuple(m.hull_planes(k) for k in range(len(m.compiled.mesh_vertnum)))


def thin_pieces(cm, width=1e-6):
    """[(geom, unit normal in the geom frame, centre in the geom frame)] of the hull geoms
    thinner than `width` metres along some facet normal (scipy's facets)."""
    V = np.asarray(cm.mesh_vert, dtype=np.float64).reshape(-1, 3)
    out = []
    for g in range(int(cm.ngeom)):
        if int(cm.geom_type[g]) != MESH:
            continue
        k = int(cm.geom_dataid[g])
        E = hull_equations(cm)[k]
        v = V[int(cm.mesh_vertadr[k]):int(cm.mesh_vertadr[k]) + int(cm.mesh_vertnum[k])]
        widths = (-(v @ E[:, :3].T + E[:, 3])).max(axis=0)
        if widths.min() < width:
            out.append((g, E[np.argmin(widths), :3].copy(), v.mean(axis=0)))
    return out


def facing_camera(gpos, gmat, g, normal, centre, side, distance=0.05, fovy=4.0):
    """A narrow world-fixed camera `distance` in front of geom g's point `centre`, on the side
    `side` (+1 / -1) of its local `normal`, looking straight at it."""
    z = gmat[g] @ (side * normal)
    x = np.cross([0.0, 0.0, 1.0], z)
    if np.linalg.norm(x) < 1e-3:
        x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pos = gpos[g] + gmat[g] @ centre + distance * z
    return cameras_lib.CameraConfig("facing", tuple(float(p) for p in pos),
                                    tuple(float(a) for a in x) + tuple(float(a) for a in y), fovy=fovy)
