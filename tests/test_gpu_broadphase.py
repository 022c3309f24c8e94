"""The body-pair cull transforms each distinct bounding sphere and plane once per pass
(dx_model.hip bp_item / bp_cull, dx_step.hip collision step 1).  The host tables must expand
back to the pair arrays of the compiled model bit for bit, and stepping must give exactly
what the per-pair loop of the parent revision gave (tests/golden/broadphase_parent.npz,
recorded by tools/record_broadphase_golden.py with the parent's library)."""

import glob
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(ROOT, "assets", "*.npz")))
CULL_PLANE, CULL_KEEP = 1 << 30, 1 << 31


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_broadphase_golden", os.path.join(ROOT, "tools", "record_broadphase_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("asset", ASSETS)
def test_tables_expand_to_the_pair_arrays(asset):
    """Every unit's two items give back the bodies, the spheres the cull reads, the margin
    and the plane geom of bpair_*, as float32 bits; the items are exactly the distinct
    (body, sphere) and plane geoms of the units; every id is in range."""
    from dexterity_amd import physics
    from dexterity_amd.mjcf.compiler import CompiledModel

    cm = CompiledModel.load(os.path.join(ROOT, "assets", asset + ".npz"))
    A = cm.arrays
    ph = physics.BatchedPhysics(physics.Model(cm), 1)
    nitem, nplane, nbp = (int(v) for v in ph.debug_get("bp_sizes"))
    item, cull = ph.debug_get("bp_item"), ph.debug_get("bp_cull")
    ph.close()
    body = A["bpair_body"].reshape(-1, 2)
    sph = A["bpair_sphere"].reshape(-1, 8).astype(np.float32)
    plane = A["bpair_plane"].ravel()
    margin = A["gpair_margin"].ravel().astype(np.float32)[A["bpair_adr"].ravel()]
    gbody, gpos = A["geom_bodyid"].ravel(), A["geom_pos"].reshape(-1, 3).astype(np.float32)
    assert nbp == len(body) and item.shape == (nitem, 8) and cull.shape == (nbp, 2)
    tag = item[:, 7].view(np.int32)
    ibody, isplane = tag & 0xffff, (tag >> 16) != 0
    assert np.all(isplane[:nplane]) and not np.any(isplane[nplane:])  # planes take the first ids
    want = set()
    want_planes = set()
    w = cull[:, 0].view(np.uint32)
    i1, i2 = (w & 0xfff).astype(int), ((w >> 12) & 0xfff).astype(int)
    assert np.array_equal(_bits(cull[:, 1].view(np.float32)), _bits(margin))
    for k in range(nbp):
        s1, s2, pg = sph[k, :4], sph[k, 4:], int(plane[k])
        tested = s2[3] >= 0 and (pg >= 0 or s1[3] >= 0)
        assert bool(w[k] & CULL_KEEP) == (not tested), k
        assert bool(w[k] & CULL_PLANE) == (tested and pg >= 0), k
        if not tested:
            continue
        assert 0 <= i2[k] < nitem and 0 <= i1[k] < nitem, k
        assert not isplane[i2[k]] and ibody[i2[k]] == body[k, 1], k
        assert np.array_equal(_bits(item[i2[k], :4]), _bits(s2)), k
        want.add((int(body[k, 1]), _bits(s2).tobytes()))
        if pg >= 0:
            assert isplane[i1[k]] and i1[k] < nplane, k
            assert item[i1[k], 3:4].view(np.int32)[0] == pg, k
            assert ibody[i1[k]] == gbody[pg] == body[k, 0], k
            assert np.array_equal(_bits(item[i1[k], :3]), _bits(gpos[pg])), k
            want_planes.add(pg)
        else:
            assert not isplane[i1[k]] and ibody[i1[k]] == body[k, 0], k
            assert np.array_equal(_bits(item[i1[k], :4]), _bits(s1)), k
            want.add((int(body[k, 0]), _bits(s1).tobytes()))
    # a plane item's normal: the z axis of the geom's frame, a unit vector
    for p in range(nplane):
        assert abs(np.linalg.norm(item[p, 4:7].astype(np.float64)) - 1.0) < 1e-6
    assert nplane == len(want_planes)
    assert nitem - nplane == len(want)
    have = {(int(ibody[i]), _bits(item[i, :4]).tobytes()) for i in range(nplane, nitem)}
    assert have == want
    # the world-space items fit the LDS area the kernel gives them (16 portal groups x 36 words)
    assert nitem + nplane <= 16 * 36 // 4


@pytest.fixture(scope="module")
def golden_parent():
    with np.load(os.path.join(ROOT, "tests", "golden", "broadphase_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_golden_holds_real_contacts(golden_parent):
    rec = _recorder()
    assert rec.contact_fraction(golden_parent["reorient/ncon"]) >= rec.MIN_CONTACT_FRACTION
    assert golden_parent["bimanual/ncon"].shape == (8,) and golden_parent["adroit_reach/ncon"].shape == (16,)


@pytest.mark.parametrize("scene", ["reorient", "bimanual", "adroit_reach"])
def test_results_are_the_parents(golden_parent, scene):
    """The same calls on this tree's library: state, task outputs and the final state's
    contact records equal the parent revision's, bit for bit."""
    rec = _recorder()
    key, domain, nenv, steps = next(s for s in rec.SCENES if s[0] == scene)
    got = rec.run_scene(domain, nenv, steps)
    for name, a in got.items():
        want = golden_parent[f"{key}/{name}"]
        assert a.shape == want.shape and a.dtype == want.dtype, name
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(want).tobytes(), name
