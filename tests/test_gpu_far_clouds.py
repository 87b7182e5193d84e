"""Six features on clouds far from the origin (tests/far_clouds.py): MovingLeastSquares, BoundaryEstimation, RegionGrowing,
EuclideanClusterExtraction, the outlier filters and the normal-plane SAC models.  Map-frame clouds sit hundreds or thousands
of units out: a float's ulp there is 1e-4 to 1e-3, and every sub-segment of the index build fits the packed 24-bit key form
with many equal keys -- a regime none of the features' own modules reaches.

The clouds: a wavy sheet on a 2^-10 grid (`grid`), the same moved by (8192, -8192, 4096) (`moved`: every coordinate
difference is the same float, so whatever is computed from differences must give the SAME answer, and the restatement of
the unmoved cloud is the exact expectation), scaled by 2^-20 and 2^20 (`small`, `large`: likewise, in units of the scale), and
the raw surface stored as float32 around (1500, -3000, 700) (`far_raw`: nothing exact, three ulps, float-grid ties).

MovingLeastSquares goes through run / check / float_ok of tests/test_gpu_mls.py: indices and m exactly, normal and curvature
within the UNMOVED (m + 32) * 2^-53 * kappa -- a translation does not change them --, the point within that times r PLUS
mls_restatement.far_point_term, the one rounding at |q| each of two correct implementations owes.  The other five go through
their own modules' check / check_exact / check_sor unchanged: exact, the cap on unstable cases 0, and every case asserts its
guard on the restatement alone before the device is asked."""
import functools
import math

import numpy as np
import pytest

import boundary_restatement as br
import cluster_restatement as cr
import far_clouds as fc
import mls_restatement as mr
import outlier_restatement as rs
import region_growing_restatement as rr
import sac_models_restatement as sm
import test_gpu_boundary as tb
import test_gpu_cluster as tc
import test_gpu_mls as tm
import test_gpu_outlier_removal as to
import test_gpu_region_growing as tr
import test_gpu_sac_models as ts

pytestmark = pytest.mark.gpu
SHIFT = np.asarray(fc.SHIFT, np.float64)
FAR_RAW_RADIUS = 0.05  # the largest of 0.1, 0.05, ... at which far_raw has dropped, plane-only and fitted records (asserted)
SCALES = {"small": -20, "large": 20}
THREE = ("grid", "moved", "far_raw")
FIVE = THREE + tuple(SCALES)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


# ---- MovingLeastSquares ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet():
    return fc.grid_sheet()[0]


@functools.lru_cache(maxsize=None)
def sheet_restated(r):
    ref = mr.restate(fc.grid_sheet()[0], r)
    assert int(ref["excluded"].sum()) == 0 and len(ref["indices"]) == len(fc.grid_sheet()[0])
    return ref


def expectation(ref, cloud, shift=0.0, plane=False):
    """the restatement `ref` as the expectation for `cloud` = its cloud + shift: the points move, the point bound gains the
    rounding at |q|, everything else stays"""
    point = ref["plane_point"] if plane else ref["point"]
    return dict(ref, point=point + shift, normal=ref["plane_normal"] if plane else ref["normal"],
                bound_point=ref["bound_point"] + mr.far_point_term(cloud, ref["indices"]))


@pytest.mark.parametrize("r", [0.1, 0.06])
def test_mls_moved_grid(gpu, sheet, r):
    ref = sheet_restated(r)
    far = fc.moved(sheet)
    tm.check(tm.run(gpu, far, r), expectation(ref, far, SHIFT), "moved grid r=%g" % r)


def test_mls_far_raw(gpu):
    """against the query-relative restatement of the stored floats themselves; the radius leaves records without output,
    with the plane alone and with a fit in one cloud"""
    pts = fc.far_raw()[0]
    r = FAR_RAW_RADIUS
    ref = mr.restate(pts, r, query_relative=True)
    m = ref["m_all"]
    assert (m < 3).any() and ((m >= 3) & (m < 6)).any() and ref["fitted"].any() and (~ref["fitted"]).any()
    tm.check(tm.run(gpu, pts, r), expectation(ref, pts), "far_raw r=%g" % r)


@pytest.mark.parametrize("name", sorted(SCALES))
def test_mls_scaled(gpu, sheet, name):
    """the outputs divided by the scale against the unmoved restatement within the unmoved bounds: a power of two changes no
    mantissa anywhere in the call"""
    r, f = 0.1, 2.0 ** SCALES[name]
    ref = sheet_restated(r)
    p, n, c, idx, d = tm.run(gpu, fc.scaled(sheet, SCALES[name]), r * f)
    d = d.copy()
    d[:, :3] /= f
    tm.check(((p / np.float32(f)).astype(np.float32), n, c, idx, d), ref, "grid x 2^%d" % SCALES[name])


def test_mls_moved_grid_plane_records(gpu, sheet):
    """order 0 and the method NONE: the plane record is the output"""
    r = 0.1
    far = fc.moved(sheet)
    outs = [tm.run(gpu, far, r, order=o, method=m) for o, m in ((0, tm.SIMPLE), (2, tm.NONE))]
    tm.check(outs[0], expectation(sheet_restated(r), far, SHIFT, plane=True), "moved grid plane")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs[0], outs[1]))
    assert tm.sign_rule_holds(outs[0][4][:, 3:6])


# ---- the clouds of the other five features ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(name):
    """-> (points, (nx, ny, nz, curvature) records, the factor lengths are multiplied by)"""
    if name == "far_raw":
        return fc.far_raw() + (1.0,)
    pts, rec = fc.grid_sheet(hole=True)
    if name == "moved":
        pts = fc.moved(pts)
    if name in SCALES:
        return fc.scaled(pts, SCALES[name]), rec, 2.0 ** SCALES[name]
    return pts, rec, 1.0


def normals_of(name):
    return np.ascontiguousarray(cloud(name)[1][:, :3])


# ---- BoundaryEstimation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIVE)
def test_boundary(gpu, name):
    import pcl_amd
    pts, _, f = cloud(name)
    nrm = normals_of(name)
    ref = br.restate(pts, nrm, threshold=math.pi / 2, radius=0.08 * f)
    assert br.unstable(ref) == 0 and 200 < int(ref["flag"].sum()) < len(pts) // 2
    if name != "far_raw":  # the same differences: the same flags as the grid's
        assert np.array_equal(ref["flag"], br.restate(cloud("grid")[0], nrm, threshold=math.pi / 2, radius=0.08)["flag"])
    tb.check_exact(tb.run(gpu, pts, nrm, radius=0.08 * f, thr=math.pi / 2), ref, name + " r = 0.08")
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    tree.setNormals(nrm)
    lists, _ = tree.nearestKSearch(pts, 10)
    refk = br.restate(pts, nrm, threshold=math.pi / 2, lists=lists)
    assert (refk["m"] == 10).all() and br.unstable(refk) == 0 and 0 < int(refk["flag"].sum()) < len(pts)
    tb.check_exact(tb.run(gpu, pts, None, k=10, thr=math.pi / 2, tree=tree), refk, name + " k = 10")


# ---- RegionGrowing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIVE)
def test_region_growing(gpu, name):
    pts, rec, _ = cloud(name)
    theta = rr.clear_theta(pts, rec, 9, 0.08)
    clusters, labels, _ = tr.check(gpu, pts, rec, k=9, theta=theta)  # (asserts near_threshold == 0 first)
    assert len(clusters) > 3 and (labels >= 0).all()
    if name != "far_raw":
        base = tr.reference(cloud("grid")[0], rec, 9, theta, rr.DEFAULT_CURVATURE)
        assert labels.tobytes() == base[2].tobytes() and all(np.array_equal(a, b) for a, b in zip(clusters, base[3]))


# ---- EuclideanClusterExtraction -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIVE)
def test_euclidean_clusters(gpu, name):
    pts, _, f = cloud(name)
    ref = cr.euclidean_clusters(pts, 0.03 * f)
    assert len(ref[0]) > 50 and len(ref[0][0]) > 20
    if name != "far_raw":
        base = cr.euclidean_clusters(cloud("grid")[0], 0.03)
        assert np.array_equal(ref[1], base[1]) and ref[2] == base[2]
    tc.check(gpu, pts, 0.03 * f, ref=ref)


# ---- StatisticalOutlierRemoval, RadiusOutlierRemoval --------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE)
def test_outlier_filters(gpu, name):
    """on the 2^-10 grid squared distances are small integers times 2^-20 and tie among the nine nearest
    (tests/test_far_clouds_restatement.py::test_clouds_tie_and_repeat): the k-NN tie rule decides which of them enter the
    mean, near the origin and 8192 away alike"""
    pts = cloud(name)[0]
    ref = rs.statistical_outlier_removal(pts, 8, 1.0)
    assert 0 < len(ref["removed"]) < len(pts) // 2
    base = rs.statistical_outlier_removal(cloud("grid")[0], 8, 1.0)
    if name == "moved":
        assert np.array_equal(ref["kept"], base["kept"]) and np.array_equal(to.bits(ref["dist"]), to.bits(base["dist"]))
    f, kept = to.sor(gpu, pts, 8, 1.0)
    to.check_sor(f, kept, ref, name)
    if name == "moved":
        assert np.array_equal(np.asarray(kept), base["kept"])
    for dense in (True, False):
        want = rs.radius_outlier_removal(pts, 0.05, 4, dense=dense)
        assert 0 < len(want["removed"]) < len(pts) // 2
        if name == "moved":
            assert np.array_equal(want["kept"], rs.radius_outlier_removal(cloud("grid")[0], 0.05, 4, dense=dense)["kept"])
        f, kept = to.ror(gpu, pts, 0.05, 4, is_dense=dense)
        assert np.array_equal(np.asarray(kept), want["kept"]), (name, dense)
        assert np.array_equal(np.asarray(f.getRemovedIndices()), want["removed"]), (name, dense)


# ---- the normal-plane SAC models ----------------------------------------------------------------------------------------
SAC_MODELS = {11: dict(model_type=11, ndw=0.1), 16: dict(model_type=16, axis=(0.0, 0.0, 1.0), eps_angle=0.3, ndw=0.1)}


@pytest.mark.parametrize("model", sorted(SAC_MODELS))
@pytest.mark.parametrize("name", ["far_raw", "moved"])
def test_normal_plane_counts(gpu, name, model):
    """64 hypotheses of the far cloud itself through pclhip_sac_model_evaluate.  n . p + d cancels thousands against
    thousands in float here: far_raw is the cloud where the order of the float sum decides counts (asserted)."""
    pts, rec, _ = cloud(name)
    mk = SAC_MODELS[model]
    coeffs = sm.hypotheses(pts, 64)
    clear = [t for t in (0.03, 0.031, 0.029)
             if (lambda ev: ev["in_band"] == 0 and ev["gate_band"] == 0)(sm.evaluate(sm.Model(**mk), pts, rec, coeffs, t))]
    assert clear, "no threshold of the three leaves the band empty"
    thr = clear[0]
    sensitive = sm.order_sensitive(mk, pts, rec, coeffs, thr)
    print("%s model %d: threshold %g, %d flags depend on the order of the float sums" % (name, model, thr, sensitive))
    if name == "far_raw":
        assert sensitive > 0
    cnt = ts.evaluated(gpu, pts, rec, thr, mk, coeffs)  # (asserts in_band == 0 and gate_band == 0 first)
    assert cnt.max() > 100
    if model == 16:
        valid = sm.Model(**mk).gate(coeffs)[0]
        assert 0 < valid.sum() < len(valid) and not cnt[~valid].any()
