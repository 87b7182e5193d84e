"""pclhip_boundary off the easy path: closed forms on lattices with the normal along every axis, a wedge at every phase of
the angle bins and across the +-pi cut, neighbourhoods whose every gap is ambiguous to the occupancy mask (the repeated
resolve pass), duplicates, non-finite records and normals, steep neighbours, synthetic families and an index with three
levels of boxes.  The yardstick is tests/boundary_restatement.py; flags are compared exactly outside its unstable band."""
import math

import numpy as np
import pytest

import boundary_restatement as br
from test_boundary_restatement import LATTICE_ROTATIONS
from test_gpu_boundary import check_exact, estimator, run

pytestmark = pytest.mark.gpu
Z = np.array((0, 0, 1), np.float32)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def tiled(normal, n):
    return np.ascontiguousarray(np.tile(np.asarray(normal, np.float32), (n, 1)))


@pytest.mark.parametrize("name", sorted(LATTICE_ROTATIONS))
def test_planar_lattice(gpu, name):
    """9 x 9, r = 1.5 spacings: the gaps are pi / 4 inside, pi on an edge, 3 pi / 2 in a corner; the thresholds stay 0.1 away"""
    pts, nrm, ij = br.planar_lattice(9, LATTICE_ROTATIONS[name])
    want = br.lattice_gap(ij, 9)
    for thr, count in ((0.6, 81), (math.pi / 2, 32), (4.0, 4), (5.0, 0)):
        flags, bad = run(gpu, pts, tiled(nrm, 81), radius=1.5, thr=thr)
        assert bad == 0 and int(flags.sum()) == count and np.array_equal(flags != 0, want > thr)
        check_exact((flags, bad), br.restate(pts, nrm, threshold=thr, radius=1.5), "lattice %s thr %.2f" % (name, thr))


RING_M, RING_GRID, RING_PITCH = 48, 12, 4.0


def ring_field(thr, wedge):
    """128 rings of 48 points around their centres, 4 apart on a grid: the wedge of ring i starts at the phase
    base + (i % 64 + 0.37) * 2 pi / 4096 -- 64 steps across one bin of 2 pi / 64 -- with base 0.1 for the first 64 rings and
    pi - thr / 2 (the wedge spans the +-pi cut) for the others -> points, the centres' records"""
    clouds, centres = [], []
    for i in range(128):
        base = 0.1 if i < 64 else math.pi - thr / 2
        p = br.ring(RING_M, wedge, base + (i % 64 + 0.37) * 2 * math.pi / 4096).astype(np.float64)
        p[:, 0] += RING_PITCH * (i % RING_GRID)
        p[:, 1] += RING_PITCH * (i // RING_GRID)
        centres.append(i * (RING_M + 1))
        clouds.append(p)
    return np.ascontiguousarray(np.concatenate(clouds).astype(np.float32)), np.array(centres, np.int32)


@pytest.mark.parametrize("thr", (math.pi / 8 + 0.01, math.pi / 4, math.pi / 2, math.pi))
def test_ring_at_every_bin_phase(gpu, thr):
    for wedge, want in ((thr + 1e-3, 1), (thr - 1e-3, 0)):
        pts, centres = ring_field(thr, wedge)
        ref = br.restate(pts, Z, threshold=thr, radius=1.5, rows=centres)
        assert (ref["m"] == RING_M + 1).all() and br.unstable(ref) == 0 and (ref["flag"] == want).all()
        assert np.abs(ref["max32"] - wedge).max() <= 2e-5  # (the rings' coordinates are rounded at up to 48)
        flags, bad = run(gpu, pts, tiled(Z, len(pts)), radius=1.5, thr=thr, indices=centres)
        assert bad == 0 and (flags == want).all(), np.nonzero(flags != want)[0]


def test_many_ambiguous_runs(gpu):
    """thr = pi / 8 + 0.01 and 16 neighbours pi / 8 apart: every gap spans 3 or 4 empty bins, which the mask cannot tell
    from thr, and none exceeds it -- four resolve passes look at all 16.  One neighbour less: a gap of pi / 4."""
    thr = math.pi / 8 + 0.01
    even = br.ring(16, math.pi / 8, 0.05)
    b = estimator(gpu, even, tiled(Z, 17), radius=1.5, thr=thr, indices=np.array([0], np.int32))
    assert b.compute().tolist() == [0] and b.lastResolved() == 1
    assert br.restate(even, Z, threshold=thr, radius=1.5, rows=[0])["flag"].tolist() == [0]
    assert run(gpu, even[:-1], tiled(Z, 16), radius=1.5, thr=thr, indices=np.array([0], np.int32))[0].tolist() == [1]
    # fifteen gaps below thr and one just above / below it, the wide one in every quarter of the bins: it is found in the
    # first resolve pass or in the last
    for phase in (-3.0, -1.4, 0.2, 1.8, 2.9):
        for wedge, want in ((thr + 1e-3, 1), (thr - 1e-3, 0)):
            pts = br.ring(16, wedge, phase)
            ref = br.restate(pts, Z, threshold=thr, radius=1.5, rows=[0])
            assert ref["flag"].tolist() == [want] and br.unstable(ref) == 0
            b = estimator(gpu, pts, tiled(Z, 17), radius=1.5, thr=thr, indices=np.array([0], np.int32))
            assert b.compute().tolist() == [want] and b.lastResolved() == 1, (phase, wedge)
            assert estimator(gpu, pts, tiled(Z, 17), k=17, thr=thr).compute()[0] == want  # k mode: the same steps


def test_duplicates_and_few_neighbours(gpu):
    pts = np.array([(0, 0, 0), (0, 0, 0), (0, 0, 0), (5, 0, 0), (5.5, 0, 0), (9, 9, 9), (20, 0, 0), (20.5, 0, 0), (19.8, 0.5, 0),
                    (30, 0, 0), (30, 0, 0), (30.5, 0, 0)], np.float32)
    ref = br.restate(pts, Z, radius=1.0)
    assert ref["m"].tolist() == [3, 3, 3, 2, 2, 1, 3, 3, 3, 3, 3, 3] and not ref["invalid"].any()
    # three entries and no angle; two neighbours; alone; two angles; a duplicate and one angle (the wrap-around alone: 2 pi)
    assert ref["flag"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
    check_exact(run(gpu, pts, tiled(Z, len(pts)), radius=1.0), ref, "duplicates")
    for thr in (6.2, 6.28, 6.29, 7.0):  # one angle: max_dif = 2 * float(pi) exactly
        want = br.restate(pts, Z, threshold=thr, radius=1.0)
        assert want["flag"][9:11].tolist() == [int(thr < 6.2831855)] * 2
        assert np.array_equal(run(gpu, pts, tiled(Z, len(pts)), radius=1.0, thr=thr)[0], want["flag"])


def test_non_finite_records_and_normals(gpu):
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(25), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    pts = np.concatenate([g + rng.uniform(-0.3, 0.3, g.shape), rng.normal(0, 0.05, (1000, 1))], axis=1).astype(np.float32)
    pts = pts[rng.permutation(1000)]
    nrm = (np.array((0.05, -0.1, 1.0)) + rng.normal(0, 0.05, (1000, 3))).astype(np.float32)
    bad_rec = rng.permutation(1000)[:40]
    pts[bad_rec[:20], rng.integers(0, 3, 20)] = np.nan
    pts[bad_rec[20:], rng.integers(0, 3, 20)] = np.inf
    bad_nrm = np.setdiff1d(rng.permutation(1000)[:60], bad_rec)
    nrm[bad_nrm[::2]] = 0
    nrm[bad_nrm[1::2], 1] = np.nan
    ref = br.restate(pts, nrm, radius=1.6)
    assert int(ref["invalid"].sum()) == 40 + len(bad_nrm) and not ref["flag"][ref["invalid"]].any()
    assert 50 < ref["flag"].sum() < 500
    flags, bad = run(gpu, pts, nrm, radius=1.6)
    check_exact((flags, bad), ref, "non-finite")
    # the finite records' flags are those of the cloud without the non-finite ones (a bad normal stays a neighbour)
    keep = np.setdiff1d(np.arange(1000), bad_rec)
    removed, bad2 = run(gpu, np.ascontiguousarray(pts[keep]), np.ascontiguousarray(nrm[keep]), radius=1.6)
    assert np.array_equal(removed, flags[keep]) and bad2 == len(bad_nrm)
    assert np.array_equal(removed, br.restate(pts[keep], nrm[keep], radius=1.6)["flag"])
    lists, _ = KdTreeOf(gpu, pts).nearestKSearch(np.ascontiguousarray(pts[keep]), 8)
    kflags, kbad = run(gpu, pts, nrm, k=8)
    want = br.restate(pts, nrm, lists=lists, rows=keep)
    assert br.unstable(want) == 0 and np.array_equal(kflags[keep], want["flag"]) and kbad == bad
    assert not kflags[bad_rec].any()


def KdTreeOf(gpu, pts):
    import pcl_amd
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    return tree


def test_steep_neighbours(gpu):
    """a 12 x 12 sheet and, over 20 of its points, a point almost along the normal, 1e-3 off it in the direction 0.2 rad:
    kappa = 10^3 for that neighbour (and for the sheet point under it as a neighbour), E = 6e-4 for its gaps.  The gaps are
    multiples of pi / 4, such multiples -+ 0.2, and 0.2: thr = 2.0 and 1.2 stay 0.05 away from all of them."""
    pts, nrm, ij = br.planar_lattice(12)
    rng = np.random.default_rng(3)
    base = rng.permutation(144)[:20]
    steep = pts[base].astype(np.float64) + np.array([1e-3 * math.cos(0.2), 1e-3 * math.sin(0.2), 1.0])
    cloud = np.ascontiguousarray(np.concatenate([pts, steep.astype(np.float32)]))
    for thr in (2.0, 1.2):
        ref = br.restate(cloud, Z, threshold=thr, radius=1.5)
        assert ref["kappa"] >= 500 and ref["closest"].min() >= 0.05 and br.unstable(ref) == 0
        check_exact(run(gpu, cloud, tiled(Z, len(cloud)), radius=1.5, thr=thr), ref, "steep thr %.1f" % thr)


def device_normals(gpu, pts, k=10):
    """-> the index and the k-nearest-neighbour normals it now holds"""
    import pcl_amd
    tree = KdTreeOf(gpu, pts)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(pts)
    ne.setSearchMethod(tree)
    ne.setKSearch(k)
    return tree, np.ascontiguousarray(ne.compute()[:, :3])


BAND_CAP = 2  # queries per family that may own an unstable comparison


@pytest.mark.parametrize("family", ("clusters", "cube", "layers", "sheet"))
def test_synthetic_5003(gpu, family):
    """5,003 points (no multiple of 16 or 64), k = 10 normals from the device, the radius at 3 median spacings"""
    import pcl_amd
    import iss_restatement as ir
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud(family, 5003)[:, :3])
    tree, nrm = device_normals(gpu, pts)
    r = 3 * ir.median_spacing(pts)
    for thr in (math.pi / 2, math.pi / 4):
        ref = br.restate(pts, nrm, threshold=thr, radius=r)
        print("%s thr %.2f: %d boundary points of %d, %d invalid, %d in the band, %.1f neighbours, worst ratio %.3f"
              % (family, thr, int(ref["flag"].sum()), len(pts), int(ref["invalid"].sum()), br.unstable(ref),
                 float(ref["m"].mean()) - 1, ref["ratio"]))
        assert br.unstable(ref) <= BAND_CAP and ref["ratio"] <= 1.0
        assert 0 < ref["flag"].sum() < len(pts)
        flags, bad = run(gpu, pts, None, radius=r, thr=thr, tree=tree)
        ok = ~ref["own"]
        assert np.array_equal(flags[ok], ref["flag"][ok]) and bad == int(ref["invalid"].sum())


DEEP_N, DEEP_R = 16 * 4096 + 16 * 5 + 3, 0.0711  # tests/test_gpu_iss_regimes.py::test_three_box_levels


def test_three_box_levels(gpu):
    """65,619 points: 4,102 leaves, more than the 4,096 that two levels of boxes hold; 2,000 random queries through indices"""
    import pcl_amd
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud("cube", DEEP_N, seed=77)[:, :3])
    tree, nrm = device_normals(gpu, pts)
    idx = np.random.default_rng(5).permutation(DEEP_N)[:2000].astype(np.int32)
    ref = br.restate(pts, nrm, radius=DEEP_R, rows=idx)
    print("deep: %d boundary points of 2000, %d in the band, %.1f neighbours" % (int(ref["flag"].sum()), br.unstable(ref),
                                                                                 float(ref["m"].mean()) - 1))
    assert br.unstable(ref) <= BAND_CAP and 0 < ref["flag"].sum() < 2000 and (ref["m"] < 3).any()
    flags, bad = run(gpu, pts, None, radius=DEEP_R, tree=tree, indices=idx)
    ok = ~ref["own"]
    assert np.array_equal(flags[ok], ref["flag"][ok]) and bad == int(ref["invalid"].sum())
