"""pclhip_boundary / pcl_amd.BoundaryEstimation on the device against the numpy restatement (tests/boundary_restatement.py)
and the reference's own expectations on bun0 (test/features/test_boundary_estimation.cpp).

The flags are compared EXACTLY.  A query that owns an unstable comparison (a gap within E of the threshold, the
restatement's docstring) would be left out -- and the cap on such queries is 0 on every cloud of this module: the restatement
must report none.  Every case runs twice and the two results are compared bytewise."""
import ctypes as C
import math

import numpy as np
import pytest

import boundary_restatement as br

pytestmark = pytest.mark.gpu
RADII = (2, 3, 4, 6)
# every combination of these with RADII has an empty band on bun0 (asserted below before the device is asked)
THRESHOLDS = (math.pi / 8, math.pi / 4, math.pi / 2, 2.0, math.pi, 4.0, 5.0)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def bun0():
    return br.load_bun0()


@pytest.fixture(scope="module")
def bun0_tree(gpu, bun0):
    """one index with the file's normals for the cases that only vary the call"""
    import pcl_amd
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(bun0[0])
    tree.setNormals(bun0[1])
    return tree


def estimator(gpu, pts, nrm, radius=None, k=None, thr=None, indices=None, tree=None):
    import pcl_amd
    b = pcl_amd.BoundaryEstimation(gpu)
    if tree is not None:
        b.setSearchMethod(tree)
    b.setInputCloud(pts)
    if nrm is not None:
        b.setInputNormals(nrm)
    if radius is not None:
        b.setRadiusSearch(radius)
    if k is not None:
        b.setKSearch(k)
    if thr is not None:
        b.setAngleThreshold(thr)
    b.setIndices(indices)
    return b


def run(gpu, pts, nrm, **kw):
    """-> (flags uint8, invalid_count); the call is made twice, the bytes must agree"""
    b = estimator(gpu, pts, nrm, **kw)
    f1 = np.array(b.compute())
    bad = b.invalid_count
    f2 = np.array(b.compute())
    assert f1.dtype == np.uint8 and f1.tobytes() == f2.tobytes() and bad == b.invalid_count
    assert set(np.unique(f1).tolist()) <= {0, 1}
    return f1, bad


def check_exact(out, ref, label):
    """instability cap 0: nothing is left out"""
    flags, bad = out
    assert br.unstable(ref) == 0, label
    assert np.array_equal(flags, ref["flag"]), (label, np.nonzero(flags != ref["flag"])[0][:10])
    assert bad == int(ref["invalid"].sum()), label


def test_bun0_golden(gpu, bun0):
    pts = bun0[0]
    n = len(pts)
    g = br.global_normal(pts)
    import pcl_amd
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    tree.setNormals(np.ascontiguousarray(np.tile(g, (n, 1))))  # pclhip_index_set_normals
    b = estimator(gpu, pts, None, radius=10.0, tree=tree)
    assert b.getAngleThreshold() == math.pi / 2
    flags = b.compute()
    assert [int(flags[i]) for i in (0, n // 3, n // 2, n - 1)] == [0, 0, 0, 1]
    check_exact((flags, b.invalid_count), br.restate(pts, g, radius=10.0), "bun0 golden")
    a, c = b.lastPassMs()
    assert a >= 0.0 and c >= 0.0 and b.lastKernelMs() >= 0.0 and 0 <= b.lastResolved() <= n


@pytest.mark.parametrize("factor", RADII)
def test_bun0_file_normals(gpu, bun0, bun0_tree, factor):
    pts, nrm = bun0
    r = factor * br.BUN0_RESOLUTION
    for thr in THRESHOLDS:
        ref = br.restate(pts, nrm, threshold=thr, radius=r)
        assert br.unstable(ref) == 0, (factor, thr)
        check_exact(run(gpu, pts, None, radius=r, thr=thr, tree=bun0_tree), ref, "bun0 r = %d x, thr = %.3f" % (factor, thr))
    # the estimator that builds its own index and takes the normals itself
    check_exact(run(gpu, pts, nrm, radius=r), br.restate(pts, nrm, radius=r), "bun0 r = %d x, own index" % factor)


@pytest.mark.parametrize("k", (3, 10, 20))
def test_bun0_k_mode(gpu, bun0, bun0_tree, k):
    """the restatement is fed the device's own pclhip_knn lists: tie order is not under test"""
    pts, nrm = bun0
    lists, _ = bun0_tree.nearestKSearch(pts, k)
    for thr in (math.pi / 4, math.pi / 2):
        ref = br.restate(pts, nrm, threshold=thr, lists=lists)
        assert (ref["m"] == k).all()
        check_exact(run(gpu, pts, None, k=k, thr=thr, tree=bun0_tree), ref, "bun0 k = %d" % k)
    # two angles leave a gap of at least pi: with k = 3 every point is a boundary point
    assert int(ref["flag"].sum()) == len(pts) if k == 3 else 0 < int(ref["flag"].sum()) < len(pts)


def test_indices(gpu, bun0, bun0_tree):
    pts, nrm = bun0
    r = 3 * br.BUN0_RESOLUTION
    full, _ = run(gpu, pts, None, radius=r, tree=bun0_tree)
    rng = np.random.default_rng(5)
    idx = rng.permutation(len(pts))[:150].astype(np.int32)
    idx = np.concatenate([idx, idx[:40], idx[:1].repeat(5)])  # repeats
    rng.shuffle(idx)
    sub, bad = run(gpu, pts, None, radius=r, tree=bun0_tree, indices=idx)
    assert sub.shape == idx.shape and bad == 0 and np.array_equal(sub, full[idx])
    subk, _ = run(gpu, pts, None, k=10, tree=bun0_tree, indices=idx)
    assert np.array_equal(subk, run(gpu, pts, None, k=10, tree=bun0_tree)[0][idx])
    empty, bad = run(gpu, pts, None, radius=r, tree=bun0_tree, indices=np.zeros(0, np.int32))
    assert empty.shape == (0,) and bad == 0


def raw_call(lib, tree, radius, k, thr, n, indices=None, min_neighbors=3):
    out = np.full(n, 7, np.uint8)
    bad = C.c_uint64(12345)
    ind = None if indices is None else C.c_void_p(indices.ctypes.data)
    st = lib.pclhip_boundary(tree.h, ind, 0 if indices is None else len(indices), radius, k, thr, min_neighbors,
                             C.c_void_p(out.ctypes.data), C.byref(bad))
    return st, out, int(bad.value)


def test_arguments_and_state(gpu, bun0, bun0_tree):
    import pcl_amd
    from pcl_amd import _lib
    lib = _lib.load()
    pts, nrm = bun0
    n = len(pts)
    r, half = 3 * br.BUN0_RESOLUTION, math.pi / 2
    INVALID, STATE = -1, -4  # PCLHIP_ERR_INVALID, PCLHIP_ERR_STATE
    assert lib.pclhip_boundary(None, None, 0, r, 0, half, 3, None, None) == INVALID
    st, out, bad = raw_call(lib, bun0_tree, r, 0, half, n)
    assert st == 0 and bad == 0 and np.array_equal(out, br.restate(pts, nrm, radius=r)["flag"])
    # both or neither of radius and k; a radius that is no radius
    for radius, k in ((r, 10), (0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -3)):
        st, out, bad = raw_call(lib, bun0_tree, radius, k, half, n)
        assert st == INVALID and bad == 0 and (out == 7).all(), (radius, k)
    for thr in (float("nan"), float("inf"), -float("inf"), 0.39, 0.0, -1.0):
        assert raw_call(lib, bun0_tree, r, 0, thr, n)[0] == INVALID, thr
    assert raw_call(lib, bun0_tree, r, 0, math.pi / 8, n)[0] == 0
    assert raw_call(lib, bun0_tree, r, 0, half, n, indices=np.array([0, n], np.int32))[0] == INVALID
    assert raw_call(lib, bun0_tree, r, 0, half, n, indices=np.array([-1], np.int32))[0] == INVALID
    # min_neighbors below 3 acts as 3; a larger one clears the flags of smaller neighbourhoods
    ref = br.restate(pts, nrm, radius=r)
    assert np.array_equal(raw_call(lib, bun0_tree, r, 0, half, n, min_neighbors=-5)[1], ref["flag"])
    want = br.restate(pts, nrm, radius=r, min_neighbors=12)
    assert 0 < want["flag"].sum() < ref["flag"].sum()
    assert np.array_equal(raw_call(lib, bun0_tree, r, 0, half, n, min_neighbors=12)[1], want["flag"])
    # state: no normals, a selection-built index, a scaled index
    bare = pcl_amd.KdTree(gpu)
    bare.setInputCloud(pts)
    assert raw_call(lib, bare, r, 0, half, n)[0] == STATE
    sel = pcl_amd.KdTree(gpu)
    sel.setInputCloud(pts, np.arange(0, n, 2, dtype=np.int32))
    assert raw_call(lib, sel, r, 0, half, n)[0] == STATE
    scaled = pcl_amd.KdTree(gpu)
    scaled.setPointRepresentation(np.array([2.0, 1.0, 1.0], np.float32))
    scaled.setInputCloud(pts)
    assert raw_call(lib, scaled, r, 0, half, n)[0] == STATE
    with pytest.raises(pcl_amd.PclHipError):
        estimator(gpu, pts, None, radius=r, tree=bare).compute()
    # a radius whose float square is 0: a valid call in which nobody has a neighbour
    st, out, bad = raw_call(lib, bun0_tree, 1e-30, 0, half, n)
    assert st == 0 and bad == n and (out == 0).all()
    sub = np.array([5, 5, 9], np.int32)
    st, out, bad = raw_call(lib, bun0_tree, 1e-30, 0, half, 3, indices=sub)
    assert st == 0 and bad == 3 and (out == 0).all()


def test_torch_device_buffers(gpu, bun0):
    import torch
    pts, nrm = bun0
    r = 3 * br.BUN0_RESOLUTION
    host = run(gpu, pts, nrm, radius=r)
    t = torch.from_numpy(pts).cuda()
    b = estimator(gpu, t, torch.from_numpy(nrm).cuda(), radius=r)
    flags = b.compute()
    assert flags.is_cuda and flags.dtype == torch.uint8
    assert flags.cpu().numpy().tobytes() == host[0].tobytes() and b.invalid_count == host[1]
    idx = np.array([7, 3, 3, 200], np.int32)
    b.setIndices(idx)
    assert np.array_equal(b.compute().cpu().numpy(), host[0][idx])
