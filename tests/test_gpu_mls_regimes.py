"""pclhip_mls_process off the path of tests/test_gpu_mls.py (bun0): clouds below and across a leaf (16), a wavefront (64) and
a block, the padding of the last leaf, an index with three box levels, the strict bound d2 < float(r * r) at a lattice shell,
clouds whose answers are known in closed form (tests/test_mls_restatement.py holds the restatement to the same closed
forms), the reference's almost-on-a-line cloud, non-finite records, and every refusal.

The conventions are those of tests/test_gpu_mls.py (check): counts and indices exactly, the doubles within
(m + 32) * 2^-53 * kappa (* r), every call made twice and compared bytewise.  Every test asserts ON THE RESTATEMENT that its
input is in the regime it is meant for."""
import ctypes as C

import numpy as np
import pytest

import iss_restatement as ir
import mls_restatement as mr
from test_gpu_mls import NONE, ORTHOGONAL, SIMPLE, check, raw_call, run, sign_rule_holds, smoother

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def cube(n, seed=3):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


# ---- sizes around the leaf, the wavefront and the block ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 1025])
def test_sizes(gpu, n):
    pts = cube(n)
    r = 0.6 if n < 1000 else 0.1
    ref = mr.restate(pts, r)
    if n == 1:
        assert len(ref["indices"]) == 0
    elif n >= 63:
        assert ref["fitted"].any() and (ref["m_all"] < 6).any() == (n == 1025)
    if n == 1025:  # dropped, plane-only and fitted records in one cloud
        assert 0 < len(ref["indices"]) < n and (~ref["fitted"]).any()
    check(run(gpu, pts, r), ref, "n=%d" % n)
    if 1 < n < 1000:  # one neighbourhood: every point a neighbour of every point
        ref = mr.restate(pts, 4.0)
        assert (ref["m_all"] == n).all()
        check(run(gpu, pts, 4.0), ref, "n=%d r=4" % n)


@pytest.mark.parametrize("k", [1, 4])
def test_padding_of_the_last_leaf_is_no_neighbour(gpu, k):
    """16 k + 1 points against the first 16 k: the last leaf holds one point and 15 pads.  The extra point lies in the
    middle of the cloud, so a pad taken for a point would show in some neighbour count."""
    pts = cube(16 * k + 1, seed=6)
    pts[-1] = (0.5, 0.5, 0.5)
    r = 0.8
    ref, short = mr.restate(pts, r), mr.restate(pts[:-1], r)
    assert (ref["m_all"][:-1] == short["m_all"] + 1).all()  # the extra point is everybody's neighbour, and nothing else is
    check(run(gpu, pts, r), ref, "16 * %d + 1" % k)
    check(run(gpu, np.ascontiguousarray(pts[:-1]), r), short, "16 * %d" % k)


DEEP_N, DEEP_R = 16 * 4096 + 16 * 5 + 3, 0.05  # tests/test_gpu_iss_regimes.py::test_three_box_levels: its size, its non-max radius


def test_three_box_levels(gpu):
    """65,619 points: 4,102 leaves, more than the 4,096 that two levels of boxes hold.  The restatement takes 400 sampled
    points, each by one pass over the cloud."""
    import pcl_amd
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud("cube", DEEP_N, seed=77)[:, :3])
    assert len(pts) == DEEP_N
    p, n, c, idx, d = run(gpu, pts, DEEP_R)
    sample = np.sort(np.random.default_rng(5).permutation(DEEP_N)[:400])
    ref = mr.restate(pts, DEEP_R, rows=sample)
    assert (ref["m_all"] < 3).sum() >= 10 and (~ref["fitted"]).sum() >= 50 and ref["fitted"].sum() >= 100
    assert (np.diff(idx) > 0).all()
    # the sampled records of the device's output: present exactly when m >= 3
    at = np.searchsorted(idx, sample)
    present = (at < len(idx)) & (idx[np.minimum(at, len(idx) - 1)] == sample)
    assert np.array_equal(present, ref["m_all"] >= 3) and np.array_equal(sample[present], ref["indices"])
    rows = at[present]
    check((p[rows], n[rows], c[rows], idx[rows], d[rows]), ref, "deep")
    # every record of the cloud: m >= 3, a unit normal, a point within r of its input point
    assert (d[:, 7] >= 3).all() and (np.abs(np.linalg.norm(d[:, 3:6], axis=1) - 1) <= 8 * mr.U).all()
    assert (np.linalg.norm(d[:, :3] - pts[idx], axis=1) < DEEP_R).all()


# ---- the strict bound --------------------------------------------------------------------------------------------------------
STRICT = [(3.0, 93), (float(np.nextafter(np.float32(3), np.float32(4))), 123)]


@pytest.mark.parametrize("r,m", STRICT)
def test_cubic_lattice_and_the_strict_bound(gpu, r, m):
    """9 x 9 x 9 integer points.  The shell |v|^2 = 9 sits exactly on float(3 * 3): d2 < 9 keeps its 30 points out, the next
    float radius lets them in.  (C = s * I at the interior point: no gap, its normal is anybody's -- the record is excluded
    from the bounds, as the restatement says; its count and its point are not.)"""
    shape = (9, 9, 9)
    pts, ijk = ir.lattice(shape)
    inner = np.nonzero(ir.lattice_interior(ijk, shape, (1, 1, 1), [r]))[0]
    assert len(inner) == 1 and (pts[inner] == 4).all()
    assert np.float32(r * r) == 9 if m == 93 else 9 < np.float32(r * r) < 9.00001
    assert ir.lattice_closed_form((1, 1, 1), r)[0] == m
    ref = mr.restate(pts, r)
    at = int(np.searchsorted(ref["indices"], inner[0]))
    assert ref["m"][at] == m and ref["excluded"][at]
    out = run(gpu, pts, r, method=NONE)
    check(out, dict(ref, point=ref["plane_point"], normal=ref["plane_normal"]), "cubic r=%r" % r, max_excluded=None)
    assert out[4][at, 7] == m and (out[0][at] == 4).all()  # q == c: the plane goes through the point whatever its normal


# ---- closed forms ------------------------------------------------------------------------------------------------------------
def test_plane_lattice(gpu):
    """integer points in z = 0: the points come back bitwise, normal (0, 0, 1), curvature 0 -- with and without the fit"""
    pts = mr.plane_lattice()
    ref = mr.restate(pts, 2.5)
    assert len(ref["indices"]) == len(pts) and ref["fitted"].all()
    for method in (SIMPLE, NONE):
        p, n, c, idx, d = run(gpu, pts, 2.5, method=method)
        assert len(idx) == len(pts) and np.array_equal(d[:, 7], ref["m"])
        assert p.tobytes() == pts.tobytes()
        assert (d[:, 3:6] == [0.0, 0.0, 1.0]).all() and (d[:, 6] == 0).all() and (c == 0).all()


def test_rotated_plane_lattice(gpu):
    pts64 = mr.plane_lattice().astype(np.float64) @ mr.rotation().T
    pts = np.ascontiguousarray(pts64.astype(np.float32))
    ref = mr.restate(pts, 2.5)
    assert not ref["excluded"].any() and (ref["curvature"] < 2.0 ** -40).all()
    out = run(gpu, pts, 2.5)
    check(out, ref, "rotated plane")
    assert (out[4][:, 6] < 2.0 ** -40).all()
    axis = mr.rotation()[:, 2]
    assert (np.abs(np.abs(out[4][:, 3:6] @ axis) - 1.0) <= 1e-6).all()


def test_axis_line(gpu):
    """integer points on the x axis: C = diag(s, 0, 0) exactly, a Cholesky pivot is exactly 0 -- the fit falls back and the
    output equals the input bitwise"""
    pts = mr.axis_line()
    ref = mr.restate(pts, 6.5)
    assert ref["excluded"].all() and not ref["fitted"].any() and (ref["m"] >= 6).all()
    p, n, c, idx, d = run(gpu, pts, 6.5)
    assert np.array_equal(idx, np.arange(len(pts))) and np.array_equal(d[:, 7], ref["m"])
    assert p.tobytes() == pts.tobytes() and (d[:, 6] == 0).all()
    assert (d[:, 3] == 0).all() and (np.abs(np.linalg.norm(d[:, 3:6], axis=1) - 1) <= 8 * mr.U).all()
    assert sign_rule_holds(d[:, 3:6])


def test_identical_points(gpu):
    pts = np.tile(np.float32([0.25, -1.5, 3.0]), (7, 1))
    for k in (7, 5, 3, 2):
        p, n, c, idx, d = run(gpu, np.ascontiguousarray(pts[:k]), 0.5)
        if k < 3:
            assert len(idx) == 0
            continue
        assert np.array_equal(idx, np.arange(k)) and (d[:, 7] == k).all()
        assert p.tobytes() == pts[:k].tobytes() and (c == 0).all() and np.isfinite(d).all()
        assert (np.abs(np.linalg.norm(d[:, 3:6], axis=1) - 1) <= 8 * mr.U).all()


def test_almost_on_a_line(gpu):
    """the reference's cloud (test/surface/test_moving_least_squares.cpp:66-70): four records, all finite"""
    pts = mr.almost_on_line()
    ref = mr.restate(pts, mr.ALMOST_ON_LINE_RADIUS)
    assert len(ref["indices"]) == 4 and not ref["excluded"].any()
    out = run(gpu, pts, mr.ALMOST_ON_LINE_RADIUS)
    assert len(out[3]) == 4 and np.isfinite(out[0]).all() and np.isfinite(out[1]).all() and np.isfinite(out[4]).all()
    check(out, ref, "almost on a line")


# ---- records and indices -----------------------------------------------------------------------------------------------------
def test_non_finite_records(gpu):
    rng = np.random.default_rng(21)
    pts = cube(400, seed=21)
    bad = rng.permutation(400)[:100]
    pts[bad[:40], 0] = np.nan
    pts[bad[40:70], 1] = np.inf
    pts[bad[70:], 2] = -np.inf
    ref = mr.restate(pts, 0.25)
    assert len(ref["indices"]) >= 250 and not np.isin(ref["indices"], bad).any()
    out = run(gpu, pts, 0.25)
    check(out, ref, "non-finite")
    assert not np.isin(out[3], bad).any()
    none = np.full((50, 3), np.nan, np.float32)  # no finite record at all
    assert len(run(gpu, none, 0.25)[3]) == 0


@pytest.mark.parametrize("r,square_is_zero", [(1e-30, True), (3e-23, False)])
def test_radius_whose_square_underflows(gpu, r, square_is_zero):
    """float(r * r) == 0: no point has a neighbour -- a valid call without output.  The smallest subnormal: every point finds
    itself and its exact duplicates; three of them make a record"""
    assert (np.float32(r * r) == 0) == square_is_zero
    pts = cube(150, seed=8)
    pts[41] = pts[42] = pts[40]
    ref = mr.restate(pts, r)
    assert ref["indices"].tolist() == ([] if square_is_zero else [40, 41, 42])
    p, n, c, idx, d = run(gpu, pts, r)
    assert idx.tolist() == ref["indices"].tolist()
    if not square_is_zero:
        assert p.tobytes() == pts[40:43].tobytes() and (d[:, 7] == 3).all() and (c == 0).all()


def test_refusals(gpu):
    import pcl_amd
    from pcl_amd import _lib
    lib = _lib.load()
    pts = mr.load_bun0()
    r = 0.01
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    idx = np.full(397, -7, np.int32)
    nan, inf = float("nan"), float("inf")
    assert raw_call(lib, tree, r, 397, idx=idx) == (0, 380)
    for bad in (0.0, -0.0, -1.0, -1e-30, nan, inf, -inf):  # PCLHIP_ERR_INVALID, the count zeroed
        assert raw_call(lib, tree, bad, 397, sg=r * r, idx=idx) == (-1, 0)
        assert raw_call(lib, tree, r, 397, sg=bad, idx=idx) == (-1, 0)
    assert raw_call(lib, tree, 1e-30, 397, sg=r * r, idx=idx) == (0, 0)  # a valid radius whose float square is 0
    for order in (-1, 3, 4):
        assert raw_call(lib, tree, r, 397, order=order, idx=idx) == (-1, 0)
    assert raw_call(lib, tree, r, 397, method=ORTHOGONAL, idx=idx) == (-1, 0)
    assert b"ORTHOGONAL" in lib.pclhip_last_error(gpu.h)
    for method in (-1, 3):
        assert raw_call(lib, tree, r, 397, method=method, idx=idx) == (-1, 0)
    k = C.c_uint64(0)
    assert lib.pclhip_mls_process(None, r, r * r, 2, SIMPLE, None, None, C.c_void_p(idx.ctypes.data), 397, C.byref(k), None) == -1
    assert lib.pclhip_mls_process(tree.h, r, r * r, 2, SIMPLE, None, None, C.c_void_p(idx.ctypes.data), 397, None, None) == -1
    # PCLHIP_ERR_STATE: an index that is scaled, or covers a selection of the cloud
    scaled = pcl_amd.KdTree(gpu)
    scaled.setPointRepresentation([1.0, 2.0, 1.0])
    scaled.setInputCloud(pts)
    assert raw_call(lib, scaled, r, 397, idx=idx) == (-4, 0)
    subset = pcl_amd.KdTree(gpu)
    subset.setInputCloud(pts, np.arange(0, 397, dtype=np.int32))
    assert raw_call(lib, subset, r, 397, idx=idx) == (-4, 0)
    s = smoother(gpu, pts, r, tree=subset)
    s.tree._cloud_id = (id(pts), None)  # as if it were the whole cloud's: the library itself refuses
    with pytest.raises(pcl_amd.PclHipError) as e:
        s.process()
    assert e.value.status == -4
    # the Python class: the same codes, and the upsampling methods
    for kw in (dict(order=3), dict(method=ORTHOGONAL)):
        with pytest.raises(pcl_amd.PclHipError) as e:
            smoother(gpu, pts, r, **kw).process()
        assert e.value.status == -1
    with pytest.raises(pcl_amd.PclHipError) as e:
        smoother(gpu, pts, 0.0).process()
    assert e.value.status == -1
    s = pcl_amd.MovingLeastSquares(gpu)
    s.setUpsamplingMethod(pcl_amd.MovingLeastSquares.UPSAMPLING_NONE)
    for method in (s.DISTINCT_CLOUD, s.SAMPLE_LOCAL_PLANE, s.RANDOM_UNIFORM_DENSITY, s.VOXEL_GRID_DILATION):
        with pytest.raises(NotImplementedError):
            s.setUpsamplingMethod(method)
    # a refused call leaves the index usable
    assert raw_call(lib, tree, r, 397, idx=idx) == (0, 380)
