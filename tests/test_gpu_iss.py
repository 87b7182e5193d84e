"""pclhip_iss_keypoints / pcl_amd.ISSKeypoint3D on the device against the numpy restatement (tests/iss_restatement.py) and
the reference's own six keypoints on bun0 (test/keypoints/test_iss_3d.cpp:56-101).

Eigenvalues: |e^_k - e_k| <= B_i = (m_i + 32) * 2^-53 * trace(C_i) (the restatement's docstring: a sequential double sum
of m_i products in any order, by Weyl's inequality, + 32 for the two solvers).  The worst |e^ - e| / (2^-53 * trace) is
printed with its m; DESIGN.md row f-12 records it.
Keypoints: the salient set and the keypoint list are compared EXACTLY; a point that owns an unstable comparison, or has such
a point in its non-max neighbourhood, would be left out of that -- and the cap on such points is 0 on every cloud of this
module: the restatement must report none.  Every case runs twice and the two results are compared bytewise."""
import ctypes as C

import numpy as np
import pytest

import iss_restatement as ir

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def bun0():
    return ir.load_bun0()


@pytest.fixture(scope="module")
def bun0_restated(bun0):
    return ir.restate(bun0, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION)


def detector(gpu, pts, rs, rn, g21=0.975, g32=0.975, min_neighbors=5, tree=None):
    import pcl_amd
    d = pcl_amd.ISSKeypoint3D(gpu)
    if tree is not None:
        d.setSearchMethod(tree)
    d.setInputCloud(pts)
    d.setSalientRadius(rs)
    d.setNonMaxRadius(rn)
    d.setThreshold21(g21)
    d.setThreshold32(g32)
    d.setMinNeighbors(min_neighbors)
    return d


def run(gpu, pts, rs, rn, **kw):
    """-> (indices, saliency, eigenvalues) as numpy; the call is made twice, the bytes must agree"""
    d = detector(gpu, pts, rs, rn, **kw)
    idx, sal, eig = (np.array(a) for a in d.computeAll())
    idx2, sal2, eig2 = d.computeAll()
    assert idx.tobytes() == np.asarray(idx2).tobytes()
    assert sal.tobytes() == np.asarray(sal2).tobytes() and eig.tobytes() == np.asarray(eig2).tobytes()
    assert idx.dtype == np.int32 and sal.dtype == np.float64 and eig.shape == (len(pts), 3)
    assert np.array_equal(np.asarray(d.getKeypointsIndices()), idx)
    return idx, sal, eig


def check(out, ref, pts, label, min_neighbors=5):
    """the device's eigenvalues within B; the salient set and the keypoints exactly outside the unstable band.
    -> the points left out of the exact comparison"""
    idx, sal, eig = out
    n = len(pts)
    fin = np.isfinite(np.asarray(pts, np.float32)[:, :3]).all(axis=1)
    m, B = ref["m"], ref["B"]
    assert np.isnan(eig[~fin]).all() and (sal[~fin] == 0).all()
    low = fin & (m < min_neighbors)
    assert (eig[low] == 0).all() and (sal[low] == 0).all()
    live = fin & (m >= min_neighbors)
    assert np.isfinite(eig[live]).all() and (np.diff(eig[live], axis=1) <= 0).all()  # descending
    err = np.abs(eig[live] - ref["eig"][live]).max(axis=1)
    pos = ref["trace"][live] > 0
    if pos.any():
        ratio = err[pos] / (U * ref["trace"][live][pos])
        w = int(np.argmax(ratio - m[live][pos]))
        print("%s: worst |e^ - e| / (2^-53 trace) = %.2f at m = %d (largest ratio %.2f)"
              % (label, ratio[w], m[live][pos][w], ratio.max()))
    assert (err <= B[live]).all(), (label, float((err / np.maximum(B[live], 1e-300)).max()))
    # a saliency is the device's own third eigenvalue or 0, and never that of a zero or negative e3
    assert ((sal == 0) | (sal == eig[:, 2])).all() and (sal >= 0).all()
    assert (sal[live & (eig[:, 2] <= 0)] == 0).all()
    own, excluded = ref["own"], ref["excluded"]
    print("%s: %d of %d points own an unstable comparison, %d are left out of the exact comparison"
          % (label, int(own.sum()), n, int(excluded.sum())))
    assert np.array_equal((sal > 0)[~own], (ref["sal"] > 0)[~own])
    both = ~own & (sal > 0)
    assert (np.abs(sal[both] - ref["sal"][both]) <= B[both]).all()
    assert (np.diff(idx) > 0).all()  # ascending
    flag = np.zeros(n, bool)
    flag[idx] = True
    want = np.zeros(n, bool)
    want[ref["keypoints"]] = True
    assert np.array_equal(flag[~excluded], want[~excluded])
    return excluded


def check_exact(out, ref, pts, label, min_neighbors=5):
    """instability cap 0: nothing is left out"""
    assert ir.unstable(ref) == 0
    excluded = check(out, ref, pts, label, min_neighbors=min_neighbors)
    assert not excluded.any()
    assert np.array_equal(out[0], ref["keypoints"])


def test_bun0_golden(gpu, bun0, bun0_restated):
    out = run(gpu, bun0, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION)
    check_exact(out, bun0_restated, bun0, "bun0")
    assert out[0].tolist() == ir.BUN0_RECORDS
    assert np.abs(bun0[out[0]] - ir.BUN0_KEYPOINTS).max() <= 1e-6
    d = detector(gpu, bun0, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION)
    assert d.compute().tolist() == ir.BUN0_RECORDS
    assert np.abs(d.getKeypoints() - ir.BUN0_KEYPOINTS).max() <= 1e-6
    a, b = d.lastPassMs()
    assert a >= 0.0 and b >= 0.0 and d.lastKernelMs() >= 0.0


FAMILY_KEYPOINTS = {"sheet": 296, "cube": 37, "clusters": 25, "layers": 337}


@pytest.mark.parametrize("family", sorted(FAMILY_KEYPOINTS))
def test_synthetic_5003(gpu, family):
    """5,003 points (no multiple of 16 or 64), radii 6 x and 4 x the median nearest-neighbour spacing"""
    import pcl_amd
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud(family, 5003)[:, :3])
    sp = ir.median_spacing(pts)
    ref = ir.restate(pts, 6 * sp, 4 * sp)
    assert len(ref["keypoints"]) == FAMILY_KEYPOINTS[family]
    check_exact(run(gpu, pts, 6 * sp, 4 * sp), ref, pts, family)


def test_torch_device_buffers(gpu, bun0):
    import torch
    t = torch.from_numpy(bun0).cuda()
    d = detector(gpu, t, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION)
    idx, sal, eig = d.computeAll()
    assert idx.is_cuda and sal.is_cuda and eig.is_cuda and idx.dtype == torch.int32
    host = run(gpu, bun0, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION)
    assert idx.cpu().numpy().tobytes() == host[0].tobytes()
    assert sal.cpu().numpy().tobytes() == host[1].tobytes() and eig.cpu().numpy().tobytes() == host[2].tobytes()
    assert idx.cpu().tolist() == ir.BUN0_RECORDS
    kp = d.getKeypoints()
    assert kp.is_cuda and np.array_equal(kp.cpu().numpy(), bun0[ir.BUN0_RECORDS])
    assert np.array_equal(d.compute().cpu().numpy(), host[0])


def raw_call(lib, tree, rs, rn, capacity, idx=None, sal=None, eig=None, g21=0.975, g32=0.975, min_neighbors=5):
    k = C.c_uint64(12345)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    st = lib.pclhip_iss_keypoints(tree.h, rs, rn, g21, g32, min_neighbors, ptr(idx), capacity, C.byref(k), ptr(sal), ptr(eig))
    return st, int(k.value)


def test_optional_outputs_and_capacity(gpu, bun0):
    import pcl_amd
    from pcl_amd import _lib
    lib = _lib.load()
    rs, rn = 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION
    full = run(gpu, bun0, rs, rn)
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(bun0)
    # capacity 0 (and no buffer at all): the count is written, the call reports the overflow
    assert raw_call(lib, tree, rs, rn, 0) == (-5, 6)
    # exact
    idx = np.full(7, -7, np.int32)
    assert raw_call(lib, tree, rs, rn, 6, idx=idx) == (0, 6)
    assert idx[:6].tolist() == ir.BUN0_RECORDS and idx[6] == -7
    # one short: the first five are written, nothing behind them
    idx = np.full(7, -7, np.int32)
    assert raw_call(lib, tree, rs, rn, 5, idx=idx) == (-5, 6)
    assert idx[:5].tolist() == ir.BUN0_RECORDS[:5] and (idx[5:] == -7).all()
    # the optional outputs one at a time and together: the same bytes
    for want_sal, want_eig in ((True, False), (False, True), (True, True), (False, False)):
        idx = np.empty(397, np.int32)
        sal = np.empty(397, np.float64) if want_sal else None
        eig = np.empty((397, 3), np.float64) if want_eig else None
        assert raw_call(lib, tree, rs, rn, 397, idx=idx, sal=sal, eig=eig) == (0, 6)
        assert idx[:6].tobytes() == full[0].tobytes()
        assert sal is None or sal.tobytes() == full[1].tobytes()
        assert eig is None or eig.tobytes() == full[2].tobytes()
    d = detector(gpu, bun0, rs, rn, tree=tree)
    assert np.array_equal(d.compute(), full[0]) and d.getSearchMethod() is tree


def test_keypoints_feed_fpfh(gpu, bun0):
    """the pipeline: the detector's output as FPFHEstimation's indices, on the index the detector used -- the rows of the
    full-cloud call at the keypoints"""
    import fpfh_restatement as fr
    import pcl_amd
    pts, nrm = fr.load_bun0()
    assert np.array_equal(pts, bun0)
    tree = pcl_amd.KdTree(gpu)
    d = detector(gpu, pts, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION, tree=tree)
    keys = d.compute()
    assert keys.tolist() == ir.BUN0_RECORDS
    f = pcl_amd.FPFHEstimation(gpu)
    f.setSearchMethod(tree)
    f.setInputCloud(pts)
    f.setInputNormals(nrm)
    f.setRadiusSearch(0.02)
    full = f.compute()
    f.setIndices(keys)
    sub = f.compute()
    assert sub.shape == (6, 33) and f.nan_count == 0
    assert np.array_equal(sub.view(np.uint32), full[keys].view(np.uint32))


def test_border_and_normal_radius_are_refused(gpu):
    import pcl_amd
    d = pcl_amd.ISSKeypoint3D(gpu)
    d.setBorderRadius(0.0)
    d.setNormalRadius(0.0)
    with pytest.raises(NotImplementedError):
        d.setBorderRadius(0.01)
    with pytest.raises(NotImplementedError):
        d.setNormalRadius(0.01)
