"""PGS (dx_step.hip solve_pgs) aimed at every cell of its dispatch matrix, with a warm start
that is kept by construction (tests/pgs_cases.py): the generic step kernel, the mid tier and
the overflow tier; the register blocks alone, the blocks with a tail (rows NB*64.. one at a
time in whitened force space), the register-row path above NB*64 + 64 rows and the nv > 30
Cholesky path.  Each scene is one batch with one env per eps: qacc_warmstart = w* +
eps (qacc_smooth - w*), w* the oracle's Newton optimum on the GPU's own contact list; kept
for eps up to 1e-3 -- every tail row then starts from a nonzero force -- and dropped at
1e-2.  One queued physics step against the oracle's PGS on the same contacts and warm start.

Which path ran is asserted from what the library reports: contacts, efc_count, the health
counters.  (A deferral that the mid tier did not take is counted in deferred_behind_launch;
a mid-tier case runs one env per launch and holds that count at 0.)

Measured, |qacc| error / scale, max over the four eps: tail cases 1.5e-6 .. 5.0e-6, controls
2.0e-7 .. 4.7e-6.  The same cases on a kernel whose tail started from zero: 8.7e-4 .. 6.6e-3
on every tail case with a kept warm start (the numpy model's figures, test_pgs_restatement.py,
to three digits), the controls unchanged."""

import numpy as np
import pytest

from dexterity_amd import _lib, blob
from tests import pgs_cases as pc
from tests.test_gpu_parity import PGS_QPOS_MAX, PGS_QVEL_MAX, PGS_TAIL_MAX, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

SWITCHES = ("DX_NO_MID", "DX_DEFER_AT", "DX_MID_DEFER_AT", "DX_GENERIC_KERNEL", "DX_NO_QUEUE")


def _step(gpu, cm, q, v, warm, one_by_one=False):
    """One queued physics step of len(warm) copies of the state (q, v), env e warm-started
    at warm[e]; everything the test reads back.  `one_by_one`: a batch per env, the health
    counters summed -- the mid tier is one workgroup that takes a launch's deferrals in turn
    while the overflow tier, behind the launch, takes those still waiting, so of four
    deferrals it runs one or two.  A single deferral it takes unless the launch, which
    has nothing else to do, is over before the mid tier has started (measured: 1 launch in
    40); that launch, whose step ran in the overflow tier, is done again, three times at
    the most."""
    if one_by_one:
        outs = []
        for e in range(len(warm)):
            for _ in range(3):
                o = _step(gpu, cm, q, v, warm[e:e + 1])
                if o["health"]["deferred_behind_launch"] == 0:
                    break
            outs.append(o)
        out = {k: np.concatenate([o[k] for o in outs]) for k in outs[0] if k not in ("health", "timeouts")}
        out["health"] = {k: sum(o["health"][k] for o in outs) for k in outs[0]["health"]}
        out["timeouts"] = sum(o["timeouts"] for o in outs)
        return out
    n = len(warm)
    model = gpu.Model(cm)
    ph = gpu.BatchedPhysics(model, n)
    ph.set(_lib.QPOS, np.tile(q, (n, 1)))
    ph.set(_lib.QVEL, np.tile(v, (n, 1)))
    ph.set(_lib.QACC_WARMSTART, np.asarray(warm))
    ph.debug(True)
    ph.health_clear()
    ph.step(1)
    ph.sync()
    out = dict(con=ph.debug_get("contact"), efc=ph.debug_get("efc_count"), ncon=ph.get(_lib.NCON)[:, 0],
               sweeps=ph.get(_lib.NITER)[:, 0], qacc=ph.get(_lib.QACC_WARMSTART).astype(np.float64),
               qpos=ph.qpos.astype(np.float64), qvel=ph.qvel.astype(np.float64), health=ph.health(),
               timeouts=int(ph.debug_get("queue_timeouts")[0]))
    ph.close()
    return out


@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_pgs_dispatch(gpu, oracle_mod, monkeypatch, tmp_path, case):  # noqa: F811
    name, spec, tier, NB, nv, ncon, nefc, path = case
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if tier == "hi" and ncon <= 64:
        monkeypatch.setenv("DX_NO_MID", "1")
    cm = pc.scene(*spec, tmp_path=tmp_path)
    om = oracle_mod.OracleModel(blob.pack(cm.arrays))
    om_nt = oracle_mod.OracleModel(blob.pack(cm.with_solver("Newton").arrays))
    q, v = pc.settled_state(oracle_mod, cm)
    n = len(pc.EPS)
    # the GPU's own contact list, then the Newton optimum on it
    first = _step(gpu, cm, q, v, np.zeros((n, cm.nv)), tier == "mid")
    assert list(first["ncon"]) == [ncon] * n
    gc = first["con"][0, :ncon].astype(np.float64)
    dn = pc.oracle_at(oracle_mod, om_nt, q, v, contacts=gc)
    w, a0 = dn.qacc.copy(), dn.qacc_smooth.copy()
    scale = max(1.0, np.abs(a0).max())
    warm = np.stack([pc.f32(pc.warm_start(w, a0, eps)) for eps in pc.EPS])
    out = _step(gpu, cm, q, v, warm, tier == "mid")
    # the path
    h = out["health"]
    assert cm.nv == nv and list(out["ncon"]) == [ncon] * n
    np.testing.assert_array_equal(out["con"], first["con"])
    assert list(out["efc"][:, 0]) == [nefc] * n and not out["efc"][:, 1].any()
    assert out["timeouts"] == 0
    assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, h
    assert h["contact_deferred"] == (0 if tier == "step" else n), h
    if tier == "mid":
        # every deferral was taken by the mid tier: none ran behind its launch, in the
        # overflow tier, and the mid tier never ended its wait early
        assert h["deferred_behind_launch"] == 0 and h["mid_tier_gave_up"] == 0, h
    tail = NB * pc.PGS_AR
    ntail = max(0, nefc - tail)
    assert {"tail": 0 < ntail <= pc.PGS_AR, "blocks": ntail == 0, "rows": ntail > pc.PGS_AR, "chol": nv > 30}[path]
    errs = []
    for e, eps in enumerate(pc.EPS):
        d = pc.oracle_at(oracle_mod, om, q, v, warm=warm[e], contacts=gc, step=True)
        p = pc.Problem(d, cm)
        f0 = p.warm_forces(warm[e])
        dc = p.dual_cost(f0)
        # the inputs: the row count, a kept warm start, a tail that starts loaded
        assert d.nefc == nefc
        if eps <= 1e-3:
            assert dc < -1, (name, eps, dc)
            if path == "tail":
                assert np.count_nonzero(f0[tail:]) > 0
        elif path != "chol":
            assert dc > 0, (name, eps, dc)
        ea = np.abs(out["qacc"][e] - d.qacc).max() / scale
        eq = np.abs(out["qpos"][e] - d.qpos).max()
        ev = np.abs(out["qvel"][e] - d.qvel).max() / scale
        print(f"{name} [{tier} tier, NB {NB}, {path}] nv {nv} ncon {ncon} nefc {nefc} "
              f"tail {ntail if path == 'tail' else 0} eps {eps:g}: dual cost {dc:.3g}, "
              f"sweeps {out['sweeps'][e]} (oracle {d.niter}), |qacc| err / scale {ea:.2e}, "
              f"|qpos| {eq:.1e}, |qvel| / scale {ev:.1e}, behind launch {h['deferred_behind_launch']}")
        errs.append((ea, eq, ev))
    ea, eq, ev = (max(x) for x in zip(*errs))
    assert ea <= PGS_TAIL_MAX, errs
    assert eq <= PGS_QPOS_MAX and ev <= PGS_QVEL_MAX, errs
