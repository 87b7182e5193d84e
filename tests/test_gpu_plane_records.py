"""Plane records of the point-to-plane accumulation (search.hip: plane_records_kernel, PairAcc<1>::add_plane): the pair
gathers (nx, ny, nz, c) of its target point, c the float prefix fl(fl(fl(nx tx) + fl(ny ty)) + fl(nz tz)) of the residual
of impl/transformation_estimation_point_to_plane_lls.hpp:235.  Every writer of an index's normals refreshes the records:
k-NN normals, radius normals and normals the user supplies."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20000
MAX_D = 0.1


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def clouds():
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(N)
    return tgt, src


def _radius(gpu, tgt):
    """a radius that holds ~10 neighbours of a typical point"""
    import pcl_amd
    t = pcl_amd.KdTree(gpu)
    t.setInputCloud(tgt)
    _, d2 = t.nearestKSearch(tgt[:2000], 10)
    return float(np.sqrt(np.median(d2[:, -1])))


def _write(gpu, tree, tgt, how, arg=None):
    """set the tree's normals through one writer; -> the normals as (N, 4) float32 in the cloud's order"""
    import pcl_amd
    if how == "user":
        tree.setNormals(arg)
        return np.ascontiguousarray(arg, np.float32)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(tgt)
    ne.setSearchMethod(tree)
    if how == "knn":
        ne.setKSearch(8)
    else:
        ne.setRadiusSearch(arg)
    ne.setViewPoint(0, 0, 10)
    return ne.compute()


def _run(gpu, tree, src):
    """(reduction record of the first iteration, transform of a whole alignment)"""
    import pcl_amd
    out = []
    for whole in (False, True):
        icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
        icp.setSearchMethodTarget(tree, True)
        icp.setInputSource(src)
        icp.setMaximumIterations(10)
        icp.setMaxCorrespondenceDistance(MAX_D)
        icp.setTransformationEpsilon(1e-10)
        if whole:
            icp.align()
            out.append(np.array(icp.getFinalTransformation(), np.float32))
        else:
            out.append(icp.iterate(np.eye(4, dtype=np.float32)))
    return out


def _user_normals(nrm):
    """other valid normals: every third one flipped, a few removed (NaN)"""
    u = np.array(nrm[:, :3], np.float32)
    u[::3] *= -1.0
    u[5::97] = np.nan
    return u


def _host_sums(tgt, src, nrm, q, m):
    """PairAcc<1>'s per-pair float terms restated in numpy (float32 operations round like __fmul_rn / __fadd_rn), summed
    in double: only the order of the double sums differs from the device's"""
    f = np.float32
    n = np.asarray(nrm, f)[m, :3]
    t = np.asarray(tgt, f)[m, :3]
    s = np.asarray(src, f)[q, :3]
    ok = np.isfinite(n).all(axis=1)
    n, t, s = n[ok], t[ok], s[ok]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    a = (nz * sy - ny * sz).astype(np.float64)
    b = (nx * sz - nz * sx).astype(np.float64)
    c = (ny * sx - nx * sy).astype(np.float64)
    pre = (nx * t[:, 0] + ny * t[:, 1]) + nz * t[:, 2]
    df = ((pre - nx * sx) - ny * sy) - nz * sz
    d = df.astype(np.float64)
    X, Y, Z = nx.astype(np.float64), ny.astype(np.float64), nz.astype(np.float64)
    terms = [a * a, a * b, a * c, a * X, a * Y, a * Z, b * b, b * c, b * X, b * Y, b * Z, c * c, c * X, c * Y, c * Z,
             (nx * nx).astype(np.float64), (nx * ny).astype(np.float64), (nx * nz).astype(np.float64),
             (ny * ny).astype(np.float64), (ny * nz).astype(np.float64), (nz * nz).astype(np.float64),
             a * d, b * d, c * d, X * d, Y * d, Z * d]
    return np.array([t_.sum() for t_ in terms]), int((~ok).sum())


@pytest.mark.parametrize("how", ["knn", "radius", "user"])
def test_plane_records_equal_the_host_prefix(gpu, clouds, how):
    """the first iteration's sums from plane records against the per-pair terms computed on the host from the normals
    this writer produced (a stale record or a contracted prefix moves ATb far beyond the order of the double sums)"""
    import pcl_amd
    tgt, src = clouds
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(tgt)
    arg = {"knn": None, "radius": _radius(gpu, tgt), "user": None}[how]
    if how == "user":
        arg = _user_normals(_write(gpu, tree, tgt, "knn"))
    nrm = _write(gpu, tree, tgt, how, arg)
    sums, _ = _run(gpu, tree, src)
    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputTarget(tgt)
    ce.setInputSource(src)
    q, m, _ = ce.determineCorrespondences(MAX_D)
    host, skipped = _host_sums(tgt, src, nrm, q, m)
    assert int(sums[28]) == len(q)
    assert int(sums[29]) == skipped
    scale = np.abs(host).max()
    np.testing.assert_allclose(sums[:27], host, rtol=1e-9, atol=1e-12 * scale)


def test_replaced_normals_leave_no_stale_record(gpu, clouds):
    """normals written over normals: what an alignment computes equals it on a fresh index with the last normals alone"""
    import pcl_amd
    tgt, src = clouds
    r = _radius(gpu, tgt)
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(tgt)
    knn = _write(gpu, tree, tgt, "knn")
    first = _run(gpu, tree, src)
    user = _user_normals(knn)
    for how, arg in (("user", user), ("radius", r), ("knn", None)):
        _write(gpu, tree, tgt, how, arg)
        got = _run(gpu, tree, src)
        fresh = pcl_amd.KdTree(gpu)
        fresh.setInputCloud(tgt)
        _write(gpu, fresh, tgt, how, arg)
        want = _run(gpu, fresh, src)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), how
        if how == "user":
            assert not np.array_equal(got[0], first[0]), "the user normals must change the sums"
        if how == "knn":
            for g, w in zip(got, first):
                assert np.array_equal(g, w)
