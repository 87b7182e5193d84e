"""RegionGrowing on the device against the literal transcription of the reference's flood
(tests/region_growing_restatement.py, pinned by tests/test_region_growing_restatement.py): labels, offsets and indices
equal as bytes.  Every case first asserts, with the restatement alone, that no |dot| lies within 2 ulp of the cosine
threshold, and runs twice: the two runs must give the same bytes.  This module: the roof, sizes and k at the edges of
leaves, waves and kernels, the size filter, the C-only mode, the refusals, the capacities and torch buffers."""
import ctypes as C

import numpy as np
import pytest

import region_growing_restatement as rr

pytestmark = pytest.mark.gpu
U64P = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def grower(gpu, points, normals, k=30, theta=rr.DEFAULT_THETA, curvature=rr.DEFAULT_CURVATURE, mn=1, mx=0xFFFFFFFF,
           indices=None):
    import pcl_amd
    g = pcl_amd.RegionGrowing(gpu)
    g.setInputCloud(points)
    g.setInputNormals(normals)
    g.setIndices(indices)
    g.setNumberOfNeighbours(k)
    g.setSmoothnessThreshold(theta)
    g.setCurvatureThreshold(curvature)
    g.setMinClusterSize(mn)
    g.setMaxClusterSize(mx)
    return g


def reference(points, normals, k, theta, curvature, mn=1, mx=0xFFFFFFFF, indices=None, curvature_test=True, lists=None):
    """the guard, then the literal restatement -> (offsets uint64, indices int32, labels int32, clusters)"""
    if lists is None:
        lists = rr.knn_lists(points, k, rr.selected(points, indices))
    assert rr.near_threshold(normals, lists, theta) == 0
    clusters, labels, nc = rr.literal(points, normals, k, theta, curvature, mn, mx, indices, curvature_test, lists)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.uint64)
    idx = np.concatenate(clusters).astype(np.int32) if clusters else np.empty(0, np.int32)
    assert int(off[-1]) == nc
    return off, idx, labels.astype(np.int32), clusters


def same_bytes(got, ref):
    off, idx, lab = got
    assert off.dtype == np.uint64 and idx.dtype == np.int32 and lab.dtype == np.int32
    assert off.tobytes() == ref[0].tobytes()
    assert idx.tobytes() == ref[1].tobytes()
    assert lab.tobytes() == ref[2].tobytes()


def check(gpu, points, normals, k=30, theta=rr.DEFAULT_THETA, curvature=rr.DEFAULT_CURVATURE, mn=1, mx=0xFFFFFFFF,
          indices=None, lists=None):
    """guard, two runs with equal bytes, bytes equal to the literal restatement's -> (clusters, labels, the object)"""
    ref = reference(points, normals, k, theta, curvature, mn, mx, indices, lists=lists)
    g = grower(gpu, points, normals, k, theta, curvature, mn, mx, indices)
    first = g.extractCSR()
    second = g.extractCSR()
    same_bytes(first, ref)
    same_bytes(second, first)
    clusters = g.extract()
    assert len(clusters) == len(ref[3]) and all(np.array_equal(a, b) for a, b in zip(clusters, ref[3]))
    assert np.array_equal(g.labels(), ref[2])
    return clusters, ref[2], g


# ---- the roof -----------------------------------------------------------------------------------------------------------
def test_roof_defaults(gpu):
    pts, nrm, which = rr.roof()
    clusters, lab, g = check(gpu, pts, nrm)
    assert len(clusters) == 2 and (lab >= 0).all()
    assert len(set(lab[which == 0])) == 1 and len(set(lab[which == 1])) == 1 and lab[which == 0][0] != lab[which == 1][0]
    st = g.lastStats()
    assert st["leftover"] == 0 and st["phase2_rounds"] == 0 and st["phase1_rounds"] >= 1 and st["unions"] > 0
    # a ridge point is a leaf of the segment of the lower-ranked seed that reaches it, and getSegmentFromPoint finds it
    ridge = int(np.flatnonzero(which == -1)[0])
    assert np.array_equal(g.getSegmentFromPoint(ridge), clusters[lab[ridge]])


def test_roof_small_theta_cuts_the_sheets(gpu):
    pts, nrm, _ = rr.roof()
    clusters, _, _ = check(gpu, pts, nrm, theta=float(np.deg2rad(0.3)))
    assert len(clusters) > 4


# ---- sizes and k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 30, 31, 63, 64, 65, 2049])
def test_sizes(gpu, n):
    pts, nrm = rr.wavy_sheet(n, seed=n)
    clusters, lab, _ = check(gpu, pts, nrm, k=30, theta=rr.clear_theta(pts, nrm, 30, 0.1))
    assert (lab >= 0).all() and sum(len(c) for c in clusters) == n


def test_empty_cloud_no_normals_no_neighbours(gpu):
    pts, nrm = rr.wavy_sheet(100)
    for p, r, k in ((pts[:0], nrm[:0], 30), (pts, None, 30), (pts, nrm[:-1], 30), (pts, nrm, 0)):
        g = grower(gpu, p, r, k=k)
        off, idx, lab = g.extractCSR()
        assert off.tolist() == [0] and len(idx) == 0 and len(lab) == len(p) and (lab == -1).all() and g.extract() == []
        assert len(g.getSegmentFromPoint(0)) == 0


@pytest.mark.parametrize("k", [1, 2, 30, 33, 64])
def test_k(gpu, k):
    pts, nrm = rr.wavy_sheet(300, seed=7)
    clusters, _, _ = check(gpu, pts, nrm, k=k, theta=rr.clear_theta(pts, nrm, k, 0.15))
    if k == 1:  # the list holds the point itself: every point alone, in curvature order
        order = sorted(range(300), key=lambda i: (nrm[i, 3], i))
        assert [c.tolist() for c in clusters] == [[i] for i in order]


def test_k_above_n(gpu):
    pts, nrm = rr.wavy_sheet(12, seed=5)
    check(gpu, pts, nrm, k=30, theta=rr.clear_theta(pts, nrm, 30, 0.1))
    check(gpu, pts, nrm, k=64, theta=rr.clear_theta(pts, nrm, 64, 0.2))


# ---- filters, indices, the C-only mode --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet():
    return rr.wavy_sheet(1500, seed=11)


@pytest.fixture(scope="module")
def theta12(sheet):
    return rr.clear_theta(sheet[0], sheet[1], 12, 0.06)


@pytest.fixture(scope="module")
def theta10(sheet):
    return rr.clear_theta(sheet[0], sheet[1], 10, 0.1)


def test_size_filter_drops_first_middle_last(gpu, sheet, theta12):
    pts, nrm = sheet
    full, _, _ = check(gpu, pts, nrm, k=12, theta=theta12)
    sizes = [len(c) for c in full]
    assert len(sizes) > 6 and len(set(sizes)) > 3
    first, last = sizes[0], sizes[-1]
    mid = sizes[len(sizes) // 2]
    for mn, mx in ((first + 1, 0xFFFFFFFF), (1, first - 1), (mid + 1, 0xFFFFFFFF), (1, mid - 1), (last + 1, 0xFFFFFFFF),
                   (1, max(last - 1, 1)), (2, max(sizes) - 1)):
        kept, lab, _ = check(gpu, pts, nrm, k=12, theta=theta12, mn=mn, mx=mx)
        assert [len(c) for c in kept] == [s for s in sizes if mn <= s <= mx]  # the order of the rest is kept
    kept, lab, _ = check(gpu, pts, nrm, k=12, theta=theta12, mn=6, mx=5)  # min > max
    assert kept == [] and (lab == -1).all()


def test_index_built_with_indices(gpu, sheet):
    pts, nrm = sheet
    ind = np.arange(1, len(pts), 3, dtype=np.int32)
    clusters, lab, _ = check(gpu, pts, nrm, k=10, theta=rr.clear_theta(pts, nrm, 10, 0.1, indices=ind), indices=ind)
    rest = np.setdiff1d(np.arange(len(pts)), ind)
    assert (lab[rest] == -1).all() and (lab[ind] >= 0).all() and np.isin(np.concatenate(clusters), ind).all()


def c_call(gpu, tree, nrm, n, prm, off_cap=None, idx_cap=None, with_labels=True):
    lab = np.full(n, 77, np.int32)
    off = np.full(n + 1, 99, np.uint64)
    idx = np.full(max(n, 1), -7, np.int32)
    k, nc = C.c_uint64(123), C.c_uint64(456)
    nr = np.ascontiguousarray(nrm, np.float32)
    st = gpu.lib.pclhip_region_growing(tree.h, C.c_void_p(nr.ctypes.data), nr.shape[1] * 4, C.byref(prm),
                                       C.c_void_p(lab.ctypes.data) if with_labels else None, off.ctypes.data_as(U64P),
                                       n + 1 if off_cap is None else off_cap, C.c_void_p(idx.ctypes.data),
                                       n if idx_cap is None else idx_cap, C.byref(k), C.byref(nc))
    return st, lab, off, idx, int(k.value), int(nc.value)


def default_params(gpu, **kw):
    import pcl_amd
    prm = pcl_amd._lib.RegionGrowingParams()
    gpu.lib.pclhip_region_growing_params_default(C.byref(prm))
    assert (prm.number_of_neighbours, prm.curvature_test, prm.smooth_mode, prm.residual_test) == (30, 1, 1, 0)
    assert prm.smoothness_threshold == np.float32(rr.DEFAULT_THETA) and prm.curvature_threshold == np.float32(0.05)
    assert prm.residual_threshold == np.float32(0.05) and (prm.min_cluster_size, prm.max_cluster_size) == (1, 0xFFFFFFFF)
    for name, value in kw.items():
        setattr(prm, name, value)
    return prm


def test_curvature_test_off_through_c(gpu, sheet, theta10):
    """every point expands: reachable from the C interface only"""
    import pcl_amd
    pts, nrm = sheet
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    ref_off = reference(pts, nrm, 10, theta10, 0.05, curvature_test=False)
    ref_on = reference(pts, nrm, 10, theta10, 0.05)
    assert len(ref_off[3]) != len(ref_on[3])
    prm = default_params(gpu, number_of_neighbours=10, smoothness_threshold=theta10, curvature_test=0)
    for _ in range(2):
        st, lab, off, idx, k, nc = c_call(gpu, tree, nrm, len(pts), prm)
        assert st == 0 and k == len(ref_off[3]) and nc == len(ref_off[1])
        same_bytes((off[:k + 1], idx[:nc], lab), ref_off)


def test_capacities(gpu, sheet, theta10):
    import pcl_amd
    pts, nrm = sheet
    n = len(pts)
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    ref = reference(pts, nrm, 10, theta10, 0.05, mn=3)
    nseg, rn = len(ref[3]), len(ref[1])
    assert 0 < rn < n
    prm = default_params(gpu, number_of_neighbours=10, smoothness_threshold=theta10, min_cluster_size=3)
    for off_cap, idx_cap in ((nseg, n), (n + 1, rn - 1), (0, 0)):
        st, lab, off, idx, k, nc = c_call(gpu, tree, nrm, n, prm, off_cap, idx_cap)
        assert st == -5 and k == nseg and nc == rn and lab.tobytes() == ref[2].tobytes()  # PCLHIP_ERR_OVERFLOW
    st, lab, off, idx, k, nc = c_call(gpu, tree, nrm, n, prm, nseg + 1, rn)  # exactly enough
    assert st == 0 and off[nseg + 1] == 99
    same_bytes((off[:k + 1], idx[:nc], lab), ref)
    k, nc = C.c_uint64(0), C.c_uint64(0)  # every output is optional: the counts alone
    nr = np.ascontiguousarray(nrm, np.float32)
    assert gpu.lib.pclhip_region_growing(tree.h, C.c_void_p(nr.ctypes.data), 16, C.byref(prm), None, None, 0, None, 0,
                                         C.byref(k), C.byref(nc)) == 0
    assert (k.value, nc.value) == (nseg, rn)
    assert tree.lastKernelMs() > 0.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, sheet):
    import pcl_amd
    pts, nrm = sheet
    g = grower(gpu, pts, nrm)
    with pytest.raises(NotImplementedError, match="residual"):
        g.setResidualTestFlag(True)
    with pytest.raises(NotImplementedError, match="residual"):
        g.setCurvatureTestFlag(False)
    with pytest.raises(NotImplementedError, match="smooth"):
        g.setSmoothModeFlag(False)
    g.setResidualTestFlag(False)
    g.setCurvatureTestFlag(True)
    g.setSmoothModeFlag(True)
    g.setResidualThreshold(0.5)  # stored only
    assert g.getResidualThreshold() == 0.5 and g.getSmoothModeFlag() and g.getCurvatureTestFlag() and not g.getResidualTestFlag()
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    for kw, word in ((dict(residual_test=1), "residual"), (dict(smooth_mode=0), "smooth"),
                     (dict(number_of_neighbours=65), "64"), (dict(number_of_neighbours=-1), "64"),
                     (dict(smoothness_threshold=float("nan")), "NaN")):
        st, lab, off, idx, k, nc = c_call(gpu, tree, nrm, len(pts), default_params(gpu, **kw))
        assert st == -1 and (k, nc) == (0, 0)  # PCLHIP_ERR_INVALID
        assert word in gpu.lib.pclhip_last_error(gpu.h).decode()
    with pytest.raises(pcl_amd._lib.PclHipError) as ei:
        grower(gpu, pts, nrm, k=65).extract()
    assert ei.value.status == -1
    bad = nrm.copy()
    bad[17, 3] = np.nan
    with pytest.raises(pcl_amd._lib.PclHipError) as ei:
        grower(gpu, pts, bad).extract()
    assert ei.value.status == -1 and "NaN" in str(ei.value)
    scaled = pcl_amd.KdTree(gpu)
    scaled.setPointRepresentation(rescale_values=(1.0, 1.0, 0.5))
    g = grower(gpu, pts, nrm)
    g.setSearchMethod(scaled)
    with pytest.raises(pcl_amd._lib.PclHipError) as ei:
        g.extract()
    assert ei.value.status == -4  # PCLHIP_ERR_STATE
    with pytest.raises(pcl_amd._lib.PclHipError) as ei:  # an index that holds a record twice
        grower(gpu, pts, nrm, indices=np.asarray([1, 5, 5, 9] + list(range(20, 90)), np.int32)).extract()
    assert ei.value.status == -4 and "once" in str(ei.value)


# ---- torch --------------------------------------------------------------------------------------------------------------------
def test_torch_device_buffers(gpu, sheet, theta10):
    import torch
    pts, nrm = sheet
    ref = reference(pts, nrm, 10, theta10, 0.05)
    g = grower(gpu, torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda(), k=10, theta=theta10)
    off, idx, lab = g.extractCSR()
    assert idx.is_cuda and lab.is_cuda and idx.dtype == torch.int32 and lab.dtype == torch.int32
    same_bytes((off, idx.cpu().numpy(), lab.cpu().numpy()), ref)
    off2, idx2, lab2 = g.extractCSR()
    assert off.tobytes() == off2.tobytes() and torch.equal(idx, idx2) and torch.equal(lab, lab2)
    clusters = g.extract()
    assert all(c.is_cuda for c in clusters) and [len(c) for c in clusters] == [len(c) for c in ref[3]]
    seg = g.getSegmentFromPoint(5)
    assert seg.is_cuda and np.array_equal(seg.cpu().numpy(), ref[3][ref[2][5]])
