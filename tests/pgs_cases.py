"""Shared by test_pgs_restatement.py (CPU) and test_gpu_pgs_dispatch.py (GPU): scenes with
chosen constraint-row counts, a warm start that PGS keeps by construction, and a numpy
restatement of the oracle's PGS (oracle/dx_oracle.c solve_pgs).

Scenes.  A free cube (half-size 2 cm) resting 0.1 mm into K coincident condim-3 planes has
4 contacts and 16 pyramid rows per plane; `parts` adds cubes to the same 6 dofs; a rack of
hinges with friction loss (its own tiny MJCF) adds one boxed row per hinge.  Row order is
the oracle's: friction-loss rows, limits, contacts.

Warm start.  qacc_warmstart = w* + eps (qacc_smooth - w*) with w* the Newton optimum of the
same state.  At eps = 0 the primal forces at w* are the dual optimum, whose dual cost
-f'(A + R)f / 2 is negative and stationary, so PGS keeps the warm start (`keep`) and every
loaded row -- the redundant planes share the load through R -- starts nonzero.
"""

import os

import numpy as np

from dexterity_amd import blob

PGS_AR = 64  # rows per register block of dx_step.hip solve_pgs_ar
EPS = (0.0, 1e-4, 1e-3, 1e-2)  # 1e-2: the warm start is dropped (the negative control)

# The dispatch matrix of dx_step.hip solve_pgs for a scene without a specialisation.
# (id, (boxes, planes, parts, hinges), tier, NB, nv, contacts, nefc, path).  tier: "step"
# (the generic step kernel, 32 or fewer contacts), "mid" (33..64 contacts, a queued step),
# "hi" (the overflow tier: the mid tier switched off, or more than 64 contacts).  path:
# "tail" (rows NB*64.. one at a time in w space), "blocks" (no tail: a control),
# "rows" (the register-row path above NB*64 + 64 rows), "chol" (nv > 30).
CASES = [
    ("step-146", (2, 4, 0, 18), "step", 2, 30, 32, 146, "tail"),
    ("step-138", (1, 8, 0, 10), "step", 2, 16, 32, 138, "tail"),
    ("step-128", (1, 8, 0, 0), "step", 2, 6, 32, 128, "blocks"),
    ("mid-144", (1, 9, 0, 0), "mid", 2, 6, 36, 144, "tail"),
    ("mid-160", (2, 5, 0, 0), "mid", 2, 12, 40, 160, "tail"),
    ("mid-192", (2, 6, 0, 0), "mid", 2, 12, 48, 192, "tail"),
    ("mid-224", (2, 7, 0, 0), "mid", 2, 12, 56, 224, "rows"),
    ("hi-224", (2, 7, 0, 0), "hi", 3, 12, 56, 224, "tail"),
    # (three cubes: a cube with two parts on five planes also has 240 rows, but its tail
    # moves qacc by only 2e-4 of the scale and its warm start is dropped at eps 1e-3)
    ("hi-240", (3, 5, 0, 0), "hi", 3, 18, 60, 240, "tail"),
    ("hi-256", (2, 8, 0, 0), "hi", 3, 12, 64, 256, "tail"),
    ("hi-192", (2, 6, 0, 0), "hi", 3, 12, 48, 192, "blocks"),
    ("hi-288", (2, 9, 0, 0), "hi", 3, 12, 72, 288, "rows"),
    ("step-nv36", (6, 1, 0, 0), "step", 2, 36, 24, 96, "chol"),
    ("mid-nv36", (6, 2, 0, 0), "mid", 2, 36, 48, 192, "chol"),
]
CASE_IDS = [c[0] for c in CASES]

_RACK = """<mujoco>
  <worldbody>
{bodies}
  </worldbody>
</mujoco>
"""
_HINGE = """    <body name="h{i}" pos="{x} 0.5 0.5">
      <inertial pos="0 0 0" mass="0.1" diaginertia="1e-4 1e-4 1e-4"/>
      <joint name="j{i}" type="hinge" axis="0 0 1" range="-1 1" frictionloss="{fl}"/>
    </body>"""


def scene(n_boxes, n_planes, parts=0, hinges=0, tmp_path=None):
    """`n_boxes` free cubes (each with `parts` more cubes attached) on `n_planes` coincident
    ground planes, and `hinges` friction-loss hinges (written as MJCF under `tmp_path`).
    The cubes stand in a row centred on the planes (whose bounding sphere is finite)."""
    from dexterity_amd.mjcf.compiler import Scene

    s = Scene()
    spacing = 0.2 if n_boxes <= 3 else 0.1
    for k in range(n_planes):
        s.add_world_geom(f"ground{k}", "plane", (1, 1, 0.1))
    for i in range(n_boxes):
        s.add_free_box(f"box{i}", 0.02, [spacing * (i - 0.5 * (n_boxes - 1)), 0.0, 0.0199],
                       parts=[(0.05 * k, 0.0, 0.0) for k in range(1, parts + 1)])
    if hinges:
        path = os.path.join(str(tmp_path), f"rack{hinges}.xml")
        with open(path, "w") as f:
            f.write(_RACK.format(bodies="\n".join(
                _HINGE.format(i=i, x=0.1 * i, fl=0.001 * (1 + i % 3)) for i in range(hinges))))
        s.attach_mjcf(path, "rack/")
    return s.compile().with_solver("PGS")


def settled_state(oracle_mod, cm, seed=2, nstep=2):
    """(qpos, qvel) after `nstep` Newton steps of the oracle from qpos0 with small random
    velocities (the hinges faster: friction-loss rows inside their box and at its bounds).
    Two steps leave every cube in contact (after six, a cube on one plane can have lifted
    off) and the contact forces large, which is what the tail's share of qacc scales with."""
    om = oracle_mod.OracleModel(blob.pack(cm.with_solver("Newton").arrays))
    rng = np.random.RandomState(seed)
    d = oracle_mod.OracleData(om)
    nfree = 6 * (cm.nq - cm.nv)
    d.qvel[:nfree] = rng.uniform(-0.02, 0.02, size=nfree)
    d.qvel[nfree:] = rng.uniform(-1.0, 1.0, size=cm.nv - nfree)
    for _ in range(nstep):
        d.step()
    return d.qpos.copy(), d.qvel.copy()


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def oracle_at(oracle_mod, om, qpos, qvel, warm=None, contacts=None, ctrl=None, xfrc=None, step=False):
    """The oracle's forward pass (or one step) at the fp32-rounded state, optionally on a
    given contact list (dxo_set_contacts) and warm start."""
    d = oracle_mod.OracleData(om)
    if xfrc is not None:
        d.xfrc_applied[:] = f32(xfrc).ravel()
    d.qpos[:], d.qvel[:] = f32(qpos), f32(qvel)
    if ctrl is not None:
        d.ctrl[:] = f32(ctrl)
    if warm is not None:
        d.qacc_warmstart[:] = f32(warm)
    if contacts is not None:
        d.set_contacts(np.asarray(contacts, dtype=np.float64))
    d.step() if step else d.forward()
    return d


class Problem:
    """The dual problem of the oracle's last forward pass, from its fields alone."""

    def __init__(self, d, cm):
        nv, n = int(cm.nv), d.nefc
        self.nv, self.nefc = nv, n
        self.J = d.efc_J.reshape(n, nv).copy()
        self.R = d.efc_R.copy()
        self.aref = d.efc_aref.copy()
        self.a0 = d.qacc_smooth.copy()
        self.M = d.M.reshape(nv, nv).copy()
        self.M = np.tril(self.M) + np.tril(self.M, -1).T
        fl = np.asarray(cm.dof_frictionloss, dtype=np.float64)
        dofs = np.flatnonzero(fl > 0)
        self.nfric = len(dofs)
        self.floss = np.full(n, np.inf)
        self.floss[: self.nfric] = fl[dofs]
        # friction-loss rows come first, one unit entry each at their dof
        unit = np.zeros((self.nfric, nv))
        unit[np.arange(self.nfric), dofs] = 1.0
        assert np.array_equal(self.J[: self.nfric], unit)
        self.scale = 1.0 / (float(cm.meaninertia) * max(nv, 1))
        self.iterations, self.tolerance = int(cm.iterations), float(cm.tolerance)

    def warm_forces(self, warm):
        """Primal forces of every row at qacc = warm (row_cost)."""
        jar = self.J @ warm - self.aref
        f = np.where(jar < 0, -jar / self.R, 0.0)
        k = self.nfric
        f[:k] = np.clip(-jar[:k] / self.R[:k], -self.floss[:k], self.floss[:k])
        return f

    def dual_cost(self, f):
        g = self.J.T @ f
        return 0.5 * f @ (self.R * f) - f @ self.aref + 0.5 * g @ np.linalg.solve(self.M, g) + g @ self.a0


def solve_pgs(p, warm, tail_from=None):
    """MuJoCo's PGS as the oracle states it: warm-start forces kept when their dual cost is
    negative, AR's diagonal, rows in order, boxed (friction loss) and one-sided projections,
    a sweep's scaled dual-cost decrease against the tolerance.  Returns (qacc, sweeps, keep,
    starting forces).  `tail_from`: a model of a solver that forgets the starting forces of
    rows tail_from.. in qacc (they stay in f): what seeding w without the tail computes."""
    MiJt = np.linalg.solve(p.M, p.J.T)  # column r: M^-1 J_r'
    f = p.warm_forces(warm)
    keep = p.dual_cost(f) < 0
    if not keep:
        f[:] = 0.0
    f0 = f.copy()
    seen = f.copy()
    if tail_from is not None:
        seen[tail_from:] = 0.0
    qacc = p.a0 + MiJt @ seen
    ard = np.einsum("rk,kr->r", p.J, MiJt) + p.R
    it = 0
    while it < p.iterations:
        impr = 0.0
        for r in range(p.nefc):
            res = p.J[r] @ qacc - p.aref[r] + p.R[r] * f[r]
            fn = f[r] - res / ard[r]
            fn = min(max(fn, -p.floss[r]), p.floss[r]) if r < p.nfric else max(fn, 0.0)
            dl = fn - f[r]
            if dl != 0:
                qacc = qacc + dl * MiJt[:, r]
                f[r] = fn
                impr -= 0.5 * ard[r] * dl * dl + dl * res
        it += 1
        if p.scale * impr < p.tolerance:
            break
    return qacc, it, keep, f0


def warm_start(w_star, a0, eps):
    return w_star + eps * (a0 - w_star)
