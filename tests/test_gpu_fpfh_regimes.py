"""pclhip_fpfh off the path of tests/test_gpu_fpfh.py (bun0, one 5,003-point cloud, 200 points with edge records): clouds
smaller than a leaf (16) and a wavefront (64), the strict bound d2 < float(r * r) of the FPFH walks' own comparison
(leaf_hits_lt), radii whose float square is 0, the smallest subnormal and +inf, clouds far from the origin, duplicates en
masse, an index with three box levels, a coplanar grid whose rows are known in closed form, and the object's state
between calls.

The bars are those of tests/test_gpu_fpfh.py (check_spfh, check_weighting): SPFH rows bit for bit for points without an
unstable pair, elsewhere L1 of the counts <= 2 u; the weighting of the device's own SPFH rows within (m + 4) * 2^-24 * 100.

Every test asserts ON THE RESTATEMENT that its input is in the regime it is meant for (the neighbour counts), so that a
later change of an input cannot quietly empty it."""
import numpy as np
import pytest

import fpfh_restatement as fr
from test_gpu_fpfh import bits, check_spfh, check_weighting, run

pytestmark = pytest.mark.gpu

HOT = [5, 16, 27]  # the bins of f1 = f2 = f3 = 0 (bin coordinate 5.5 in each histogram)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cube(n, seed=3):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3), dtype=np.float32), unit_normals(rng, n)


def full_checks(gpu, pts, nrm, r, label):
    ref = fr.restate(pts, nrm, r)
    out, spfh, nans = run(gpu, pts, nrm, r)
    assert out.shape == (len(pts), 33) and spfh.shape == (len(pts), 33)
    check_spfh(spfh, ref, label)
    check_weighting(out, spfh, pts, r, ref["hoods"], label)
    return ref, out, spfh, nans


# ---- sizes around the leaf and the wavefront ---------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [4.0, 0.3])
@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129])
def test_small_clouds(gpu, n, r):
    pts, nrm = cube(n)
    ref, out, spfh, nans = full_checks(gpu, pts, nrm, r, "n=%d r=%g" % (n, r))
    assert nans == 0
    if r == 4.0:  # one neighbourhood: every point a neighbour of every point
        assert (ref["m"] == n).all()
    else:
        assert ref["m"].min() >= 1 and (n < 15 or ref["m"].max() < n)
    if n == 1:  # a lone point: zeros, not NaN
        assert (bits(spfh) == 0).all() and (bits(out) == 0).all()


# ---- the strict bound ----------------------------------------------------------------------------------------------------
LATTICE_R = [(0.25, 1), (0.5, 27), (float(np.nextafter(np.float32(0.5), np.float32(1))), 33), (0.75, 93)]


@pytest.mark.parametrize("r,expected", LATTICE_R)
def test_strict_bound_on_a_lattice(gpu, r, expected):
    """6 x 6 x 6 points at spacing 0.25: every squared distance is an exact float, and the lattice's shells sit exactly
    on r = 0.25, 0.5 and 0.75.  d2 < float(r * r) keeps a shell out; the next float above 0.5 lets it in."""
    g = np.arange(6, dtype=np.float32) * np.float32(0.25)
    pts = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    nrm = unit_normals(np.random.default_rng(3), len(pts))
    centre = (2 * 6 + 2) * 6 + 2
    assert (pts[centre] == 0.5).all()
    ref, out, spfh, nans = full_checks(gpu, pts, nrm, r, "lattice r=%r" % r)
    assert nans == 0
    assert ref["m"][centre] == expected
    counts = fr.counts_from_rows(spfh, ref["m"])
    for h in range(3):  # hist_incr = 100 / (expected - 1) added expected - 1 times over each histogram
        assert counts[centre, 11 * h:11 * h + 11].sum() == expected - 1
    # ... and every other point's count
    assert np.array_equal(counts[:, :11].sum(axis=1), ref["m"] - 1)


# ---- radii at the ends of float ----------------------------------------------------------------------------------------------
def fresh_bits(gpu, pts, nrm, r):
    out, spfh, nans = run(gpu, pts, nrm, r)
    return bits(out).copy(), bits(spfh).copy(), nans


@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("r,square_is_zero", [(1e-30, True), (3e-23, False)])
def test_radius_whose_square_underflows(gpu, r, square_is_zero, edges):
    """float(r * r) == 0: no point has a neighbour, not even itself -- a valid call: zero SPFH rows, NaN FPFH rows, every
    one counted.  float(r * r) == the smallest subnormal: every point finds itself alone -- zero rows in both outputs, no
    NaN.  With `edges` the cloud also holds a record the index drops and a point without a normal (NaN rows in both
    outputs, as at any radius) and an exact duplicate, which the subnormal bound finds at d2 == 0 (binned with
    f1 = f2 = f3 = 0, weighing nothing) and the zero bound does not."""
    import pcl_amd
    assert (np.float32(r * r) == 0) == square_is_zero and np.float32(r * r) <= np.float32(1.5e-45)
    n = 150
    pts, nrm = cube(n, seed=8)
    no_row = np.zeros(n, bool)
    want_m = np.full(n, 0 if square_is_zero else 1, np.int64)  # the restatement's neighbourhoods
    if edges:
        pts[41] = pts[40]
        pts[60] = np.nan
        nrm[80] = np.nan
        no_row[[60, 80]] = True
        want_m[60] = 0
        if not square_is_zero:
            want_m[[40, 41]] = 2
    ref = fr.restate(pts, nrm, r)
    assert np.array_equal(ref["m"], want_m) and ref["unstable"].sum() == 0
    zero_row = ~no_row & (want_m < 2)
    assert (bits(ref["spfh"][zero_row]) == 0).all() and np.isnan(ref["spfh"][no_row]).all()
    assert (ref["counts"][want_m == 2].sum(axis=1) == 3).all() and (ref["counts"][want_m == 2][:, HOT] == 1).all()
    if square_is_zero:
        assert np.isnan(ref["fpfh64"]).all() and np.isnan(ref["fpfh32"]).all()
    else:
        assert (ref["fpfh64"][~no_row] == 0).all() and (bits(ref["fpfh32"][~no_row]) == 0).all()

    tree = pcl_amd.KdTree(gpu)
    f = pcl_amd.FPFHEstimation(gpu)
    f.setSearchMethod(tree)
    f.setInputCloud(pts)
    f.setInputNormals(nrm)
    f.setRadiusSearch(r)
    out, spfh = f.computeBoth()
    assert np.isnan(spfh[no_row]).all() and (bits(spfh[zero_row]) == 0).all()
    assert np.array_equal(bits(spfh), bits(ref["spfh"]))  # (no unstable pair: every row, the NaN ones too)
    assert np.isnan(out[no_row]).all()
    if square_is_zero:
        assert np.isnan(out).all() and f.nan_count == n
    else:
        assert (bits(out[~no_row]) == 0).all() and f.nan_count == int(no_row.sum())
    check_spfh(spfh, ref, "r=%g" % r)
    check_weighting(out, spfh, pts, r, ref["hoods"], "r=%g" % r)
    # through indices, repeats included
    sel = np.array([3, 60, 3, 149], np.int32)
    f.setIndices(sel)
    sub = f.compute()
    assert np.array_equal(np.isnan(sub), np.isnan(out[sel])) and f.nan_count == int(np.isnan(out[sel, 0]).sum())
    # the next, ordinary call on the same tree: the bits of a fresh object
    f.setIndices(None)
    f.setRadiusSearch(0.3)
    out2, spfh2 = f.computeBoth()
    want_out, want_spfh, want_nans = fresh_bits(gpu, pts, nrm, 0.3)
    assert np.array_equal(bits(out2), want_out) and np.array_equal(bits(spfh2), want_spfh)
    assert f.nan_count == want_nans == int(no_row.sum())


def test_radius_zero_and_negative_stay_invalid(gpu):
    import ctypes as C
    import pcl_amd
    from pcl_amd import _lib
    pts, nrm = cube(20)
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    tree.setNormals(nrm)
    out = np.empty((20, 33), np.float32)
    nan = C.c_uint64(0)
    lib = _lib.load()
    for r in (0.0, -0.0, -1e-30, -1.0, float("nan")):
        assert lib.pclhip_fpfh(tree.h, None, 0, r, C.c_void_p(out.ctypes.data), 132, None, C.byref(nan)) == -1
    assert lib.pclhip_fpfh(tree.h, None, 0, 1e-30, C.c_void_p(out.ctypes.data), 132, None, C.byref(nan)) == 0
    assert nan.value == 20 and np.isnan(out).all()


def test_radius_whose_square_is_infinite(gpu):
    pts, nrm = cube(100, seed=4)
    with np.errstate(over="ignore"):
        ref, out, spfh, nans = full_checks(gpu, pts, nrm, 1e30, "r=1e30")
    assert nans == 0 and (ref["m"] == 100).all()


# ---- away from the origin ----------------------------------------------------------------------------------------------------
def test_exact_translation(gpu):
    """700 points on a 2^-10 grid in the unit cube, moved by whole numbers: every coordinate and every difference of two
    is the same float before and after, so the pair features are, and the SPFH rows are bit for bit the unmoved ones
    whatever order the moved index puts the points in."""
    rng = np.random.default_rng(3)
    pts = (rng.integers(0, 1025, (700, 3)) / 1024.0).astype(np.float32)
    nrm = unit_normals(rng, 700)
    r = 0.15
    ref, out, spfh, nans = full_checks(gpu, pts, nrm, r, "grid")
    assert nans == 0 and 5 <= ref["m"].mean() - 1 <= 20
    for shift in ((1024.0, -2048.0, 4096.0), (-8192.0, 8192.0, 8192.0)):
        moved = (pts + np.float32(shift)).astype(np.float32)
        assert np.array_equal(moved.astype(np.float64), pts.astype(np.float64) + np.float64(shift))  # exact in float
        assert np.array_equal(moved - np.float32(shift), pts)
        out_m, spfh_m, nans_m = run(gpu, moved, nrm, r)
        assert nans_m == 0
        assert np.array_equal(bits(spfh_m), bits(spfh))
        check_weighting(out_m, spfh_m, pts, r, ref["hoods"], "grid + %r" % (shift,))  # the unmoved float64 weighting


def test_every_point_twice(gpu):
    """150 points, each present twice with another normal: every point has a neighbour at distance 0, which is binned
    with f1 = f2 = f3 = 0 and weighs nothing."""
    rng = np.random.default_rng(3)
    p = rng.random((150, 3), dtype=np.float32)
    pts = np.ascontiguousarray(np.concatenate([p, p])[rng.permutation(300)])
    nrm = unit_normals(rng, 300)
    ref, out, spfh, nans = full_checks(gpu, pts, nrm, 0.3, "twice")
    assert nans == 0 and all((d2 == 0).sum() == 2 for _nb, d2 in ref["hoods"].values())
    counts = fr.counts_from_rows(spfh, ref["m"])
    assert (counts[:, HOT] >= 1).all()


# ---- three box levels ----------------------------------------------------------------------------------------------------------
DEEP_N, DEEP_RADIUS = 16 * 4096 + 16 * 5 + 3, 0.0711


def test_three_box_levels(gpu):
    """65,619 points: 4,102 leaves, more than the 4,096 that two levels of boxes hold.  The restatement takes 400 sampled
    points, each with its neighbourhood by one pass over the cloud."""
    import pcl_amd
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud("cube", DEEP_N, seed=77)[:, :3])
    assert len(pts) == DEEP_N
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(pts)
    ne.setSearchMethod(tree)
    ne.setKSearch(10)
    nrm = np.ascontiguousarray(ne.compute()[:, :3])
    assert np.isfinite(nrm).all()
    out, spfh, nans = run(gpu, pts, None, DEEP_RADIUS, tree=tree)  # the normals the tree holds
    assert nans == 0 and not np.isnan(spfh).any()
    sample = np.sort(np.random.default_rng(5).permutation(DEEP_N)[:400])
    hoods = fr.neighbourhoods_of(pts, DEEP_RADIUS, sample)
    ref = fr.restate(pts, nrm, DEEP_RADIUS, hoods=hoods)
    m, u = ref["m"][sample], ref["unstable"][sample]
    print("deep: %.1f neighbours per sampled point, %d of 400 own an unstable pair" % (float(m.mean() - 1), int((u > 0).sum())))
    assert 8 <= m.mean() - 1 <= 16
    assert (u > 0).mean() <= 0.10
    same = (bits(spfh[sample]) == bits(ref["spfh"][sample])).all(axis=1)
    assert same[u == 0].all()
    counts = fr.counts_from_rows(spfh[sample], m)
    assert (counts >= 0).all()
    assert np.array_equal(counts[:, :11].sum(axis=1), m - 1)
    assert (np.abs(counts - ref["counts"][sample]).sum(axis=1) <= 2 * u).all()
    # the weighting of the sampled points from the device's own SPFH rows
    _f32, f64, mm = fr.weigh(spfh, pts, DEEP_RADIUS, hoods)
    bound = (mm[sample] + 4) * 2.0 ** -24 * 100.0
    err = np.abs(out[sample].astype(np.float64) - f64[sample]).max(axis=1)
    print("deep: largest error / bound = %.4f" % float((err / bound).max()))
    assert not np.isnan(f64[sample]).any() and (err <= bound).all()


# ---- coplanar, analytic ----------------------------------------------------------------------------------------------------------
def plane_grid(side):
    g = np.arange(side, dtype=np.float32) / np.float32(side)
    pts = np.zeros((side * side, 3), np.float32)
    pts[:, 0] = np.repeat(g, side)
    pts[:, 1] = np.tile(g, side)
    nrm = np.zeros_like(pts)
    nrm[:, 2] = 1.0
    return pts, nrm


def plane_rows(n):
    """the SPFH row of a point of a plane with n - 1 neighbours, all normals along the plane's: every pair has
    angle1 = angle2 = 0, f3 = 0, v = d x u in the plane, f2 = v . n = 0, f1 = atan2(w . n, u . n) = atan2(0, 1) = 0"""
    counts = np.zeros(33, np.int64)
    counts[HOT] = n - 1
    return fr.spfh_values(counts, n)


def check_plane_fpfh(rows):
    want = np.zeros(33, np.float32)
    want[HOT] = 100.0
    cold = np.ones(33, bool)
    cold[HOT] = False
    assert (bits(rows[:, cold]) == 0).all()
    assert (np.abs(rows[:, HOT].astype(np.float64) - 100.0) <= float(np.spacing(np.float32(100.0)))).all()


def test_coplanar_grid_in_closed_form(gpu):
    pts, nrm = plane_grid(32)
    # the pair features of the restatement: exactly 0, the bin coordinates 5.5 (f1's up to the float 1 / (2 pi))
    f1, f2, f3 = fr.pair_features(pts[37], nrm[37], np.delete(pts, 37, axis=0), np.delete(nrm, 37, axis=0))[:3]
    assert (f1 == 0).all() and (f2 == 0).all() and (f3 == 0).all()
    assert (np.abs(fr.bin_coords(f1, f2, f3) - 5.5) < 1e-6).all()
    out, spfh, nans = run(gpu, pts, nrm, 10.0)
    assert nans == 0
    assert (bits(spfh) == bits(plane_rows(1024))[None, :]).all()
    check_plane_fpfh(out)


# ---- indices and state ---------------------------------------------------------------------------------------------------------
def test_indices_with_repeats_and_none_at_all(gpu):
    import pcl_amd
    pts, nrm = fr.load_bun0()
    full, full_spfh, _ = run(gpu, pts, nrm, 0.02)
    sel = np.array([5, 5, 396, 0, 5], np.int32)
    sub, spfh, nans = run(gpu, pts, nrm, 0.02, indices=sel)
    assert nans == 0 and np.array_equal(bits(sub), bits(full[sel])) and np.array_equal(bits(spfh), bits(full_spfh))
    f = pcl_amd.FPFHEstimation(gpu)
    f.setInputCloud(pts)
    f.setInputNormals(nrm)
    f.setRadiusSearch(0.02)
    f.setIndices(np.zeros(0, np.int32))
    out, spfh = f.computeBoth()
    assert out.shape == (0, 33) and f.nan_count == 0
    assert np.array_equal(bits(spfh), bits(full_spfh))  # the SPFH pass does not depend on the queries
    assert f.compute().shape == (0, 33)


def test_one_object_radius_there_and_back(gpu):
    import pcl_amd
    pts, nrm = cube(300, seed=6)
    f = pcl_amd.FPFHEstimation(gpu)
    f.setInputCloud(pts)
    f.setInputNormals(nrm)
    got = {}
    for step, r in enumerate((0.2, 0.4, 0.2)):
        f.setRadiusSearch(r)
        out, spfh = f.computeBoth()
        got[step] = (bits(out).copy(), bits(spfh).copy())
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])
    assert not np.array_equal(got[0][1], got[1][1])
    for step, r in ((0, 0.2), (1, 0.4)):  # ... and both are a fresh object's
        want_out, want_spfh, _ = fresh_bits(gpu, pts, nrm, r)
        assert np.array_equal(got[step][0], want_out) and np.array_equal(got[step][1], want_spfh)


def test_new_cloud_on_the_same_tree_needs_new_normals(gpu):
    import pcl_amd
    pts, nrm = cube(100, seed=6)
    other, _ = cube(90, seed=7)
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    tree.setNormals(nrm)
    f = pcl_amd.FPFHEstimation(gpu)
    f.setSearchMethod(tree)
    f.setInputCloud(pts)
    f.setRadiusSearch(0.3)
    assert f.compute().shape == (100, 33)
    f.setInputCloud(other)  # the tree is rebuilt over it: the normals it held are gone
    with pytest.raises(pcl_amd.PclHipError) as e:
        f.compute()
    assert e.value.status == -4
    f.setInputNormals(unit_normals(np.random.default_rng(1), 90))
    assert f.compute().shape == (90, 33)
