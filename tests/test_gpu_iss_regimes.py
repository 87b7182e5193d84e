"""pclhip_iss_keypoints off the path of tests/test_gpu_iss.py (bun0 and four 5,003-point clouds at the reference's radii):
clouds smaller than a leaf (16) and a wavefront (64), an index with three box levels, min_neighbors at exactly the
neighbour count in either pass, the strict bound d2 < float(r * r) at a lattice shell, radii whose float square is 0, the
smallest subnormal and +inf, lattices whose sums are exact and whose answers are known in closed form (tests/
test_iss_restatement.py holds the restatement to the same closed forms), coincident, collinear and coplanar clouds,
non-finite records, a cloud far from the origin, extreme thresholds, a non-max radius above the salient one, and every
error path.

The conventions are those of tests/test_gpu_iss.py (check): eigenvalues within B = (m + 32) * 2^-53 * trace, the salient set
and the keypoints exactly outside the unstable band, every call made twice and compared bytewise.  Every test asserts ON THE
RESTATEMENT that its input is in the regime it is meant for."""
import ctypes as C

import numpy as np
import pytest

import iss_restatement as ir
from test_gpu_iss import check, check_exact, detector, raw_call, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def cube(n, seed=3):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


# ---- sizes around the leaf and the wavefront -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 15, 16, 17, 63, 64, 65])
def test_small_clouds(gpu, n):
    pts = cube(n)
    ref = ir.restate(pts, 0.6, 0.4)
    if n < 5:
        assert (ref["m"] < 5).all() and len(ref["keypoints"]) == 0
    else:
        assert ref["m"].max() >= 5
    out = run(gpu, pts, 0.6, 0.4)
    check_exact(out, ref, pts, "n=%d" % n)
    # one neighbourhood: every point a neighbour of every point in both passes -- the points with the largest saliency
    ref = ir.restate(pts, 4.0, 4.0, min_neighbors=1)
    assert (ref["m"] == n).all() and (ref["m_nms"] == n).all()
    out = run(gpu, pts, 4.0, 4.0, min_neighbors=1)
    if n == 1:  # a lone point: C = 0, the one comparison there is sits at 0 <= B = 0; zeros, no keypoint
        assert ref["own"].all() and len(out[0]) == 0 and (out[1] == 0).all() and (out[2] == 0).all()
        check(out, ref, pts, "n=1 r=4", min_neighbors=1)
    else:
        check_exact(out, ref, pts, "n=%d r=4" % n, min_neighbors=1)


DEEP_N, DEEP_RS, DEEP_RN = 16 * 4096 + 16 * 5 + 3, 0.0711, 0.05  # tests/test_gpu_fpfh_regimes.py: the size and the radius


def test_three_box_levels(gpu):
    """65,619 points: 4,102 leaves, more than the 4,096 that two levels of boxes hold.  The restatement takes 400 sampled
    points, each by one pass over the cloud; their non-max pass is restated over the DEVICE's saliencies (which the sample
    holds to the restatement's), so it is compared exactly."""
    import pcl_amd
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud("cube", DEEP_N, seed=77)[:, :3])
    assert len(pts) == DEEP_N
    idx, sal, eig = run(gpu, pts, DEEP_RS, DEEP_RN)
    sample = np.sort(np.random.default_rng(5).permutation(DEEP_N)[:400])
    m, c = ir.scatter_of(pts, DEEP_RS, sample)
    assert 8 <= m.mean() - 1 <= 16 and (m >= 5).mean() > 0.9 and (m < 5).any()
    e = np.linalg.eigvalsh(c)[:, ::-1]
    trace = np.trace(c, axis1=1, axis2=2)
    B = (m + ir.SOLVER_ALLOWANCE) * 2.0 ** -53 * trace
    live = m >= 5
    assert (eig[sample][~live] == 0).all() and (sal[sample][~live] == 0).all()
    err = np.abs(eig[sample][live] - e[live]).max(axis=1)
    print("deep: worst |e^ - e| / (2^-53 trace) - m = %.2f" % float((err / (2.0 ** -53 * trace[live]) - m[live]).max()))
    assert (err <= B[live]).all()
    want = ir.saliency_from(e, m, 0.975, 0.975, 5)
    own = live & ((np.abs(e[:, 1] - 0.975 * e[:, 0]) <= 2 * B) | (np.abs(e[:, 2] - 0.975 * e[:, 1]) <= 2 * B)
                  | (e[:, 2] <= B) | (e[:, 1] <= B))
    assert own.sum() == 0
    assert np.array_equal(sal[sample] > 0, want > 0) and (np.abs(sal[sample] - want) <= B).all()
    assert (want > 0).sum() >= 20
    key, m_nms = ir.nms_of(pts, DEEP_RN, sample, sal, 5)
    assert (m_nms < 5).any() and key.any()
    flag = np.zeros(DEEP_N, bool)
    flag[idx] = True
    assert np.array_equal(flag[sample], key)
    assert (np.diff(idx) > 0).all() and (sal[idx] > 0).all()


# ---- lattices: exact sums, closed forms ------------------------------------------------------------------------------------------
ANISO = (1, 2, 4)
ANISO_RS, ANISO_RN = 4.25, 3.0  # an interior point: m = 35, C = diag(152, 124, 96); 15 points within the non-max radius


def interior_sets(ijk, shape, spacing, rs, rn):
    return ir.lattice_interior(ijk, shape, spacing, [rs]), ir.lattice_interior(ijk, shape, spacing, [rs, rn])


@pytest.fixture(scope="module")
def aniso():
    shape = (21, 13, 9)
    pts, ijk = ir.lattice(shape, ANISO)
    inner, core = interior_sets(ijk, shape, ANISO, ANISO_RS, ANISO_RN)
    assert inner.sum() >= 100 and core.sum() == 27
    assert ir.lattice_closed_form(ANISO, ANISO_RS) == (35, pytest.approx([152.0, 124.0, 96.0], abs=0))
    assert ir.lattice_closed_form(ANISO, ANISO_RN)[0] == 15
    return pts, inner, core


@pytest.mark.parametrize("min_neighbors,salient,keypoints", [(15, True, True), (16, True, False), (35, True, False),
                                                             (36, False, False)])
def test_anisotropic_lattice_and_min_neighbors(gpu, aniso, min_neighbors, salient, keypoints):
    """Spacings (1, 2, 4): every interior point carries the same bits of s = 96, so with min_neighbors within both counts
    (15 in the non-max ball, 35 in the salient one) EVERY point whose non-max ball is interior is a keypoint -- the strict
    `<`.  min_neighbors = 16 fails the non-max count alone, 35 is exactly the salient count, 36 fails it."""
    pts, inner, core = aniso
    ref = ir.restate(pts, ANISO_RS, ANISO_RN, min_neighbors=min_neighbors)
    idx, sal, eig = out = run(gpu, pts, ANISO_RS, ANISO_RN, min_neighbors=min_neighbors)
    check(out, ref, pts, "aniso min=%d" % min_neighbors, min_neighbors=min_neighbors)
    assert (ref["m"][inner] == 35).all() and (ref["m_nms"][inner] == 15).all() and ref["m"].max() == 35
    if salient:
        assert (eig[inner] == [152.0, 124.0, 96.0]).all() and (sal[inner] == 96.0).all()
    else:
        assert (eig == 0).all() and (sal == 0).all() and len(idx) == 0
    flag = np.zeros(len(pts), bool)
    flag[idx] = True
    assert flag[core].all() if keypoints else not flag.any()


def test_non_max_radius_above_the_salient_one_on_the_lattice(gpu):
    shape = (24, 14, 10)
    pts, ijk = ir.lattice(shape, ANISO)
    rn = 5.0
    inner, core = interior_sets(ijk, shape, ANISO, ANISO_RS, rn)
    assert core.sum() == 8 and ir.lattice_closed_form(ANISO, rn)[0] == 67
    for min_neighbors, any_salient in ((35, True), (36, False)):  # the salient count decides: the non-max ball holds 67
        ref = ir.restate(pts, ANISO_RS, rn, min_neighbors=min_neighbors)
        idx, sal, eig = out = run(gpu, pts, ANISO_RS, rn, min_neighbors=min_neighbors)
        check(out, ref, pts, "aniso rn=5 min=%d" % min_neighbors, min_neighbors=min_neighbors)
        flag = np.zeros(len(pts), bool)
        flag[idx] = True
        if any_salient:
            assert (sal[inner] == 96.0).all() and flag[core].all()
        else:
            assert (sal == 0).all() and not flag.any()


STRICT = [(3.0, 93, 146.0), (float(np.nextafter(np.float32(3), np.float32(4))), 123, 236.0)]


@pytest.mark.parametrize("r,m,s", STRICT)
def test_cubic_lattice_and_the_strict_bound(gpu, r, m, s):
    """9 x 9 x 9 integer points.  The shell |v|^2 = 9 sits exactly on float(3 * 3): d2 < 9 keeps its 30 points out, the next
    float radius lets them in.  C = s * I for an interior point: the ratios are 1 and nothing is salient."""
    shape = (9, 9, 9)
    pts, ijk = ir.lattice(shape)
    inner = ir.lattice_interior(ijk, shape, (1, 1, 1), [r])
    assert inner.sum() == 1 and (pts[inner] == 4).all()
    assert np.float32(r * r) == 9 if m == 93 else 9 < np.float32(r * r) < 9.00001
    cm, ce = ir.lattice_closed_form((1, 1, 1), r)
    assert cm == m and (ce == s).all()
    ref = ir.restate(pts, r, r)
    assert ref["m"][inner] == m and (ref["eig"][inner] == s).all() and ref["sal"][inner] == 0
    idx, sal, eig = out = run(gpu, pts, r, r)
    check(out, ref, pts, "cubic r=%r" % r)
    assert (eig[inner] == s).all() and sal[inner] == 0
    # min_neighbors at exactly that count and one above, decided by the strict bound
    assert (run(gpu, pts, r, r, min_neighbors=m)[2][inner] == s).all()
    assert (run(gpu, pts, r, r, min_neighbors=m + 1)[2] == 0).all()


# ---- radii at the ends of float ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["salient", "non_max", "both"])
@pytest.mark.parametrize("r,square_is_zero", [(1e-30, True), (3e-23, False)])
def test_radius_whose_square_underflows(gpu, r, square_is_zero, which):
    """float(r * r) == 0: no point has a neighbour, not even itself -- a valid call without keypoints.  The smallest
    subnormal: every point finds itself (and its exact duplicate) alone."""
    assert (np.float32(r * r) == 0) == square_is_zero and np.float32(r * r) <= np.float32(1.5e-45)
    pts = cube(150, seed=8)
    pts[41] = pts[40]
    pts[60] = np.nan
    rs, rn = (r if which != "non_max" else 0.4), (r if which != "salient" else 0.4)
    for min_neighbors in (1, 2):
        ref = ir.restate(pts, rs, rn, min_neighbors=min_neighbors)
        if which != "non_max":
            want_m = np.full(150, 0 if square_is_zero else 1)
            want_m[60] = 0
            if not square_is_zero:
                want_m[[40, 41]] = 2
            assert np.array_equal(ref["m"], want_m)
        idx, sal, eig = out = run(gpu, pts, rs, rn, min_neighbors=min_neighbors)
        check(out, ref, pts, "r=%g %s" % (r, which), min_neighbors=min_neighbors)
        if which == "non_max" and not square_is_zero:
            # every point is alone in its non-max ball (40 and 41 share theirs, and their saliency): with min_neighbors 1
            # each salient one wins, with 2 the twins alone
            salient = np.nonzero(ref["sal"] > 0)[0]
            assert len(salient) >= 100 and ref["sal"][40] == ref["sal"][41] > 0
            assert ref["keypoints"].tolist() == (salient.tolist() if min_neighbors == 1 else [40, 41])
            assert not ref["excluded"].any() and np.array_equal(idx, ref["keypoints"])
        else:
            assert len(ref["keypoints"]) == 0 and len(idx) == 0
        if which != "non_max":  # C = 0 wherever there is one: nothing is salient
            assert (sal == 0).all() and (eig[np.isfinite(eig)] == 0).all() and np.isnan(eig[60]).all()
    # the next, ordinary call on the same object's tree: the bits of a fresh one
    d = detector(gpu, pts, rs, rn)
    d.compute()
    d.setSalientRadius(0.4)
    d.setNonMaxRadius(0.3)
    again = d.computeAll()
    fresh = run(gpu, pts, 0.4, 0.3)
    assert all(np.asarray(a).tobytes() == b.tobytes() for a, b in zip(again, fresh))


@pytest.mark.parametrize("which", ["salient", "non_max", "both"])
def test_radius_whose_square_is_infinite(gpu, which):
    pts = cube(100, seed=4)
    rs, rn = (1e30 if which != "non_max" else 0.4), (1e30 if which != "salient" else 0.3)
    ref = ir.restate(pts, rs, rn)
    assert which == "non_max" or (ref["m"] == 100).all()
    assert which == "salient" or ((ref["m_nms"] == 100).all() and len(ref["keypoints"]) <= 1)
    check_exact(run(gpu, pts, rs, rn), ref, pts, "r=1e30 %s" % which)


# ---- degenerate clouds -----------------------------------------------------------------------------------------------------------
def test_coincident_points(gpu):
    """300 records of one point and 40 of another: C = 0 exactly, the ratios are 0 / 0, nothing is salient"""
    pts = np.empty((340, 3), np.float32)
    pts[:300] = (0.25, -1.5, 3.0)
    pts[300:] = (9.0, 9.0, 9.0)
    ref = ir.restate(pts, 0.5, 0.5)
    assert sorted(set(ref["m"].tolist())) == [40, 300] and (ref["trace"] == 0).all()
    assert ref["own"].all() and (ref["sal"] == 0).all()  # (every comparison sits at 0 <= B = 0: the answer below is exact anyway)
    idx, sal, eig = out = run(gpu, pts, 0.5, 0.5)
    check(out, ref, pts, "coincident")
    assert len(idx) == 0 and (sal == 0).all() and (eig == 0).all()


@pytest.mark.parametrize("shape", ["line", "plane"])
def test_collinear_and_coplanar(gpu, shape):
    """Integer points on the line (k, 2k, -k) / the plane z = x + y: the sums are exact, e3 (and on the line e2) is 0 up to
    the solver's rounding.  Every such point sits inside the `e3 <= B` band and is left out of the exact comparison --
    and they are the only ones; a device e3 that is zero or negative gives s = 0 (check)."""
    rng = np.random.default_rng(12)
    if shape == "line":
        k = rng.permutation(400)[:200].astype(np.float32)
        pts = np.stack([k, 2 * k, -k], axis=1)
        r = 30.0
    else:
        ij = rng.permutation(40 * 40)[:500]
        i, j = (ij // 40).astype(np.float32), (ij % 40).astype(np.float32)
        pts = np.stack([i, j, i + j], axis=1)
        r = 6.0
    pts = np.ascontiguousarray(pts)
    ref = ir.restate(pts, r, r)
    live = ref["m"] >= 5
    assert live.sum() >= 100
    band = (ref["eig"][:, 2] <= ref["B"]) | (ref["eig"][:, 1] <= ref["B"])
    assert band[live].all() and np.array_equal(ref["own"], live)  # the band, and nothing else
    idx, sal, eig = out = run(gpu, pts, r, r)
    check(out, ref, pts, shape)
    assert (np.abs(eig[live][:, 2]) <= ref["B"][live]).all()
    if shape == "line":
        assert (np.abs(eig[live][:, 1]) <= ref["B"][live]).all()


def test_a_quarter_of_the_records_non_finite(gpu):
    rng = np.random.default_rng(21)
    pts = cube(400, seed=21)
    bad = rng.permutation(400)[:100]
    pts[bad[:40], 0] = np.nan
    pts[bad[40:70], 1] = np.inf
    pts[bad[70:], 2] = -np.inf
    ref = ir.restate(pts, 0.3, 0.2)
    assert len(ref["keypoints"]) >= 3 and (ref["m"][bad] == 0).all()
    idx, sal, eig = out = run(gpu, pts, 0.3, 0.2)
    check_exact(out, ref, pts, "non-finite")
    assert np.isnan(eig[bad]).all() and (sal[bad] == 0).all() and not np.isin(idx, bad).any()
    none = np.full((50, 3), np.nan, np.float32)  # no finite record at all
    idx, sal, eig = run(gpu, none, 0.3, 0.2)
    assert len(idx) == 0 and (sal == 0).all() and np.isnan(eig).all()


def test_shifted_cloud(gpu):
    """Points on a 2^-10 grid moved by (1000, -2000, 500): every coordinate and every difference of two is the same float
    before and after, so the restatement of the UNMOVED cloud and its bound hold for the moved one."""
    pts = (np.random.default_rng(3).integers(0, 1025, (700, 3)) / 1024.0).astype(np.float32)
    ref = ir.restate(pts, 0.3, 0.2)
    assert len(ref["keypoints"]) >= 3
    check_exact(run(gpu, pts, 0.3, 0.2), ref, pts, "grid")
    shift = np.float32((1000.0, -2000.0, 500.0))
    moved = (pts + shift).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), pts.astype(np.float64) + shift.astype(np.float64))
    assert np.array_equal(moved - shift, pts)
    check_exact(run(gpu, moved, 0.3, 0.2), ref, moved, "grid moved")


@pytest.mark.parametrize("g21,g32", [(1e-3, 1e-3), (1e6, 1e6), (1e6, 1e-3), (1e-3, 1e6)])
def test_extreme_thresholds(gpu, g21, g32):
    pts = cube(600, seed=9)
    ref = ir.restate(pts, 0.25, 0.15, g21=g21, g32=g32)
    if min(g21, g32) < 1:
        assert (ref["sal"] == 0).all()
    else:
        assert ((ref["sal"] > 0) == (ref["m"] >= 5)).all() and len(ref["keypoints"]) >= 10
    check_exact(run(gpu, pts, 0.25, 0.15, g21=g21, g32=g32), ref, pts, "gammas %g %g" % (g21, g32))


def test_non_max_radius_above_the_salient_one(gpu):
    import pcl_amd
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud("sheet", 2000, seed=5)[:, :3])
    sp = ir.median_spacing(pts)
    ref = ir.restate(pts, 4 * sp, 9 * sp)
    assert (ref["m_nms"] > ref["m"]).mean() > 0.9 and 3 <= len(ref["keypoints"]) < (ref["sal"] > 0).sum() / 4
    check_exact(run(gpu, pts, 4 * sp, 9 * sp), ref, pts, "rn > rs")


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_error_paths(gpu):
    import pcl_amd
    from pcl_amd import _lib
    lib = _lib.load()
    pts = ir.load_bun0()
    rs, rn = 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    idx = np.full(397, -7, np.int32)
    nan, inf = float("nan"), float("inf")
    assert raw_call(lib, tree, rs, rn, 397, idx=idx) == (0, 6)
    for bad in (0.0, -0.0, -1.0, -1e-30, nan, inf, -inf):  # PCLHIP_ERR_INVALID, the count zeroed
        assert raw_call(lib, tree, bad, rn, 397, idx=idx) == (-1, 0)
        assert raw_call(lib, tree, rs, bad, 397, idx=idx) == (-1, 0)
        assert raw_call(lib, tree, rs, rn, 397, idx=idx, g21=bad) == (-1, 0)
        assert raw_call(lib, tree, rs, rn, 397, idx=idx, g32=bad) == (-1, 0)
    for bad in (0, -1, -2 ** 31):
        assert raw_call(lib, tree, rs, rn, 397, idx=idx, min_neighbors=bad) == (-1, 0)
    assert raw_call(lib, tree, rs, rn, 397) == (-1, 0)  # a capacity without a buffer
    k = C.c_uint64(0)
    assert lib.pclhip_iss_keypoints(None, rs, rn, 0.975, 0.975, 5, C.c_void_p(idx.ctypes.data), 397, C.byref(k), None, None) == -1
    assert lib.pclhip_iss_keypoints(tree.h, rs, rn, 0.975, 0.975, 5, C.c_void_p(idx.ctypes.data), 397, None, None, None) == -1
    # PCLHIP_ERR_STATE: an index that is scaled, or covers a selection of the cloud
    scaled = pcl_amd.KdTree(gpu)
    scaled.setPointRepresentation([1.0, 2.0, 1.0])
    scaled.setInputCloud(pts)
    assert raw_call(lib, scaled, rs, rn, 397, idx=idx) == (-4, 0)
    subset = pcl_amd.KdTree(gpu)
    subset.setInputCloud(pts, np.arange(0, 397, dtype=np.int32))
    assert raw_call(lib, subset, rs, rn, 397, idx=idx) == (-4, 0)
    d = detector(gpu, pts, rs, rn, tree=subset)
    d.tree._cloud_id = (id(pts), None)  # as if it were the whole cloud's: the library itself refuses
    with pytest.raises(pcl_amd.PclHipError) as e:
        d.compute()
    assert e.value.status == -4
    # PCLHIP_ERR_OVERFLOW after the count
    assert raw_call(lib, tree, rs, rn, 0) == (-5, 6)
    assert raw_call(lib, tree, rs, rn, 3, idx=idx) == (-5, 6)
    with pytest.raises(pcl_amd.PclHipError) as e:
        detector(gpu, pts, 0.0, rn).compute()
    assert e.value.status == -1
    # an invalid call leaves the index usable
    assert raw_call(lib, tree, rs, rn, 397, idx=idx) == (0, 6) and idx[:6].tolist() == ir.BUN0_RECORDS
    # a float square of +inf is a radius like any other; an infinite radius is not
    assert raw_call(lib, tree, 1e30, 1e30, 397, idx=idx)[0] == 0
