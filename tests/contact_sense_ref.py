"""Numpy fp64 restatement of the external-force part of MuJoCo's mj_rnePostConstraint
([3P] engine_core_smooth.c): cfrc_ext, the contact-only wrench per body and the pad
forces of include/dx.h's contact force sensing.

Inputs are plain arrays: the oracle's data of one solved state -- `contacts()` records
(pos 3, frame 9 as rows normal / tangent1 / tangent2, dist, geom1, geom2, condim),
`efc_force`, `subtree_com`, `xipos`, `xmat` --, the compiled model's pair and body tables,
and the applied wrenches `xfrc` ([nbody][6]: force, torque).  Nothing here calls the
oracle's own rne_post_constraint; test_contact_sense_host.py compares the two.

Contact rows are the last rows of efc, in contact order: 4 pyramid rows per condim-3
contact (mju_decodePyramid: normal = their sum, tangent k = (f[2k] - f[2k+1]) * mu_k) and
one row per condim-1 contact."""

import numpy as np


def body_rootid(body_parent):
    """Root (child of the world) of every body's kinematic tree; 0 for the world."""
    parent = np.asarray(body_parent, dtype=int)
    root = np.zeros(len(parent), dtype=int)
    for b in range(1, len(parent)):
        root[b] = b if parent[b] == 0 else root[parent[b]]
    return root


def _pair_friction(cm):
    gg = np.asarray(cm.arrays["gpair_geom"], dtype=int).reshape(-1, 2)
    fr = np.asarray(cm.arrays["gpair_friction"], dtype=np.float64).reshape(-1, 5)
    table = {}
    for (g1, g2), f in zip(gg, fr):
        table[(g1, g2)] = f
        table[(g2, g1)] = f
    return table


def contact_forces(cm, contacts, efc_force):
    """Per contact: (body1, body2, pos, world-frame force acting on body2)."""
    contacts = np.asarray(contacts, dtype=np.float64).reshape(-1, 16)
    efc = np.asarray(efc_force, dtype=np.float64)
    geom_body = np.asarray(cm.arrays["geom_bodyid"], dtype=int)
    friction = _pair_friction(cm)
    rows = [4 if int(c[15]) == 3 else 1 for c in contacts]
    assert all(int(c[15]) in (1, 3) for c in contacts), "condim 1 and 3 only"
    r = len(efc) - sum(rows)
    assert r >= 0, (len(efc), rows)
    out = []
    for c, n in zip(contacts, rows):
        g1, g2 = int(c[13]), int(c[14])
        f = efc[r:r + n]
        r += n
        if n == 1:
            local = np.array([f[0], 0.0, 0.0])
        else:
            mu = friction[(g1, g2)]
            local = np.array([f.sum(), (f[0] - f[1]) * mu[0], (f[2] - f[3]) * mu[1]])
        frame = c[3:12].reshape(3, 3)
        out.append((int(geom_body[g1]), int(geom_body[g2]), c[0:3].copy(), frame.T @ local))
    return out


def _moved(force, torque, to, at):
    """[torque about `to`, force] of (force, torque) applied at `at`."""
    return np.concatenate([torque + np.cross(at - to, force), force])


def applied_wrench(cm, xfrc, subtree_com, xipos):
    """cfrc_ext's xfrc_applied part, [nbody][6]."""
    nb = cm.nbody
    root = body_rootid(cm.arrays["body_parent"])
    com = np.asarray(subtree_com, dtype=np.float64).reshape(nb, 3)
    xi = np.asarray(xipos, dtype=np.float64).reshape(nb, 3)
    x = np.zeros((nb, 6)) if xfrc is None else np.asarray(xfrc, dtype=np.float64).reshape(nb, 6)
    out = np.zeros((nb, 6))
    for b in range(1, nb):
        out[b] = _moved(x[b, :3], x[b, 3:], com[root[b]], xi[b])
    return out


def contact_wrench(cm, contacts, efc_force, subtree_com):
    """The contacts' part of cfrc_ext, [nbody][6]: + on body 2, - on body 1, world row zero."""
    nb = cm.nbody
    root = body_rootid(cm.arrays["body_parent"])
    com = np.asarray(subtree_com, dtype=np.float64).reshape(nb, 3)
    out = np.zeros((nb, 6))
    for b1, b2, pos, f in contact_forces(cm, contacts, efc_force):
        if b1:
            out[b1] -= _moved(f, np.zeros(3), com[root[b1]], pos)
        if b2:
            out[b2] += _moved(f, np.zeros(3), com[root[b2]], pos)
    return out


def cfrc_ext(cm, contacts, efc_force, subtree_com, xipos, xfrc):
    return applied_wrench(cm, xfrc, subtree_com, xipos) + contact_wrench(cm, contacts, efc_force, subtree_com)


def pad_forces(cm, contacts, efc_force, xmat, pads):
    """[npad][3]: for each pad (body, partner; -1 any) the summed force its partner's
    contacts exert on the body, in the body's frame (xmat^T F)."""
    R = np.asarray(xmat, dtype=np.float64).reshape(-1, 3, 3)
    out = np.zeros((len(pads), 3))
    cf = contact_forces(cm, contacts, efc_force)
    for k, (body, partner) in enumerate(pads):
        F = np.zeros(3)
        for b1, b2, _, f in cf:
            if b2 == body and partner in (-1, b1):
                F += f
            elif b1 == body and partner in (-1, b2):
                F -= f
        out[k] = R[body].T @ F
    return out


def prop_pads(cm, prop_body):
    """The env's pad table: every body, other than the world and the prop, with a collision
    pair against a geom of the prop body, in body order; the prop is the partner."""
    gg = np.asarray(cm.arrays["gpair_geom"], dtype=int).reshape(-1, 2)
    gb = np.asarray(cm.arrays["geom_bodyid"], dtype=int)
    hit = set()
    for g1, g2 in gg:
        b1, b2 = gb[g1], gb[g2]
        if b1 == prop_body and b2 != prop_body:
            hit.add(int(b2))
        if b2 == prop_body and b1 != prop_body:
            hit.add(int(b1))
    hit.discard(0)
    return [(b, prop_body) for b in sorted(hit)]
