"""EuclideanClusterExtraction on the device against the numpy restatement of the reference's flood
(tests/cluster_restatement.py, pinned on the reference's data by tests/test_cluster_restatement.py): the cluster lists
exactly equal, the labels consistent with the lists, n_clustered correct.  Every case runs twice and the two runs' outputs
must be the same bytes: the union-find's interleaving must not show."""
import ctypes as C
import os

import numpy as np
import pytest

import cluster_restatement as cr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def sac():
    return np.ascontiguousarray(np.load(os.path.join(GOLD, "sac_plane_radius.npz"))["cloud"][:, :3], np.float32)


@pytest.fixture(scope="module")
def bun0():
    return np.ascontiguousarray(np.load(os.path.join(GOLD, "bunny.npz"))["bun0"][:, :3], np.float32)


def extractor(gpu, cloud, tol, mn=1, mx=0xFFFFFFFF, indices=None, scale=None):
    import pcl_amd
    e = pcl_amd.EuclideanClusterExtraction(gpu)
    if scale is not None:
        tree = pcl_amd.KdTree(gpu)
        tree.setPointRepresentation(rescale_values=scale)
        e.setSearchMethod(tree)
    e.setInputCloud(cloud)
    e.setIndices(indices)
    e.setClusterTolerance(tol)
    e.setMinClusterSize(mn)
    e.setMaxClusterSize(mx)
    return e


def check(gpu, cloud, tol, mn=1, mx=0xFFFFFFFF, indices=None, scale=None, ref=None):
    """two runs, byte-identical; lists, labels and counts equal to the restatement's -> (clusters, labels)"""
    if ref is None:
        ref = cr.euclidean_clusters(cloud, tol, mn, mx, indices=indices, scale=scale)
    rc, rl, rn = ref
    e = extractor(gpu, cloud, tol, mn, mx, indices, scale)
    off, idx, lab = e.extractCSR()
    off2, idx2, lab2 = e.extractCSR()
    assert off.tobytes() == off2.tobytes() and np.asarray(idx).tobytes() == np.asarray(idx2).tobytes()
    assert np.asarray(lab).tobytes() == np.asarray(lab2).tobytes()
    assert off.dtype == np.uint64 and idx.dtype == np.int32 and lab.dtype == np.int32
    assert len(off) == len(rc) + 1 and off[0] == 0 and len(idx) == rn == int(off[-1])
    sizes = np.diff(off.astype(np.int64))
    assert sizes.tolist() == [len(c) for c in rc]
    assert np.array_equal(idx, np.concatenate(rc) if rc else np.empty(0, np.int32))
    assert np.array_equal(lab, rl)
    derived = np.full(len(cloud), -1, np.int32)  # the labels say what the lists say
    derived[idx] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    assert np.array_equal(lab, derived)
    clusters = e.extract()
    assert len(clusters) == len(rc) and all(np.array_equal(a, b) for a, b in zip(clusters, rc))
    assert np.array_equal(np.asarray(e.labels()), rl)
    return clusters, lab


@pytest.mark.parametrize("tol,nclusters,head", [(0.02, 4, [3217, 44, 21, 1]), (0.015, 1009, None), (0.03, 1, [3283])])
def test_sac_plane(gpu, sac, tol, nclusters, head):
    clusters, _ = check(gpu, sac, tol)
    assert len(clusters) == nclusters
    if head:
        assert [len(c) for c in clusters] == head


@pytest.mark.parametrize("tol,expect", [(0.01, [357, 23, 12, 3, 1, 1]), (0.004, 364)])
def test_bun0(gpu, bun0, tol, expect):
    clusters, _ = check(gpu, bun0, tol)
    if isinstance(expect, list):
        assert [len(c) for c in clusters] == expect
    else:
        assert len(clusters) == expect


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 257])
def test_collinear_leaf_and_wave_edges(gpu, n):
    clusters, _ = check(gpu, cr.line_cloud(n), 1.5)
    assert len(clusters) == 1 and np.array_equal(clusters[0], np.arange(n))


def test_strict_bound_chain_20000(gpu):
    chain = cr.integer_chain(20000)
    singles = ([np.asarray([i], np.int32) for i in range(20000)], np.arange(20000, dtype=np.int32), 20000)
    clusters, _ = check(gpu, chain, 1.0, ref=singles)  # d2 = 1 = t: no edge
    assert len(clusters) == 20000
    clusters, _ = check(gpu, chain, cr.JUST_ABOVE_ONE)  # one chain across every block
    assert [len(c) for c in clusters] == [20000]


def test_two_interleaved_rows(gpu):
    cloud, row = cr.two_rows(4096)
    clusters, lab = check(gpu, cloud, cr.JUST_ABOVE_ONE)
    assert [len(c) for c in clusters] == [4096, 4096] and clusters[0][0] == 0 and clusters[0][0] < clusters[1][0]
    assert np.array_equal(lab, np.where(row == row[0], 0, 1))
    clusters, _ = check(gpu, cloud, 1.6)
    assert [len(c) for c in clusters] == [8192]


def test_contention_on_two_roots(gpu):
    cloud, which = cr.contention_cloud(4096)
    clusters, lab = check(gpu, cloud, 0.5)
    assert [len(c) for c in clusters] == [4096, 4096]
    assert np.array_equal(lab, np.where(which == which[0], 0, 1))
    clusters, _ = check(gpu, cloud, 1.5)
    assert [len(c) for c in clusters] == [8192]


def test_size_filter_keeps_both_edges(gpu):
    cloud, ks = cr.blob_cloud()
    clusters, lab = check(gpu, cloud, 0.011, 5, 30)
    assert [len(c) for c in clusters] == sorted([k for k in range(5, 31) for _ in range(2)], reverse=True)
    assert len(clusters) == 52 and np.array_equal(lab >= 0, (ks >= 5) & (ks <= 30))
    clusters, lab = check(gpu, cloud, 0.011, 6, 5)  # min > max
    assert clusters == [] and (lab == -1).all()


@pytest.fixture(scope="module")
def volume():
    return cr.random_volume(50000)


@pytest.mark.parametrize("factor", [0.9, 1.0, 1.1])
def test_random_volume(gpu, volume, factor):
    clusters, _ = check(gpu, volume, factor * 50000 ** (-1.0 / 3.0))
    assert len(clusters) > 1


def test_non_finite_records(gpu, bun0):
    cloud = bun0.copy()
    bad = np.arange(5, len(cloud), 37)
    cloud[bad[0::3], 0] = np.nan
    cloud[bad[1::3], 1] = np.inf
    cloud[bad[2::3], 2] = -np.inf
    clusters, lab = check(gpu, cloud, 0.01)
    assert (lab[bad] == -1).all() and not np.isin(bad, np.concatenate(clusters)).any()
    # the rest is what the cloud without those records gives
    keep = np.setdiff1d(np.arange(len(cloud)), bad)
    rc, _, _ = cr.euclidean_clusters(bun0[keep], 0.01)
    assert len(rc) == len(clusters) and all(np.array_equal(keep[a], b) for a, b in zip(rc, clusters))


def test_index_built_with_indices(gpu, bun0):
    ind = np.arange(0, len(bun0), 3, dtype=np.int32)
    clusters, lab = check(gpu, bun0, 0.01, indices=ind)
    assert np.isin(np.concatenate(clusters), ind).all() and (lab[np.setdiff1d(np.arange(len(bun0)), ind)] == -1).all()
    assert sum(len(c) for c in clusters) == len(ind)


def test_scale_flattens_z(gpu):
    cloud, row = cr.two_rows(4096, gap_axis=2)
    clusters, _ = check(gpu, cloud, cr.JUST_ABOVE_ONE)
    assert [len(c) for c in clusters] == [4096, 4096]
    clusters, _ = check(gpu, cloud, cr.JUST_ABOVE_ONE, scale=(1.0, 1.0, 0.0))
    assert [len(c) for c in clusters] == [8192]


def test_tolerance_edges(gpu, bun0):
    import pcl_amd
    n = len(bun0)
    for tol in (0.0, 1e-30):
        clusters, lab = check(gpu, bun0, tol)
        assert len(clusters) == n and np.array_equal(lab, np.arange(n))
    for tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(pcl_amd._lib.PclHipError) as ei:
            extractor(gpu, bun0, tol).extract()
        assert ei.value.status == -1  # PCLHIP_ERR_INVALID


def test_capacities(gpu, bun0):
    import pcl_amd
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(bun0)
    n = len(bun0)
    rc, rl, rn = cr.euclidean_clusters(bun0, 0.01)
    u64p = C.POINTER(C.c_uint64)

    def call(off_cap, idx_cap, with_labels=True):
        lab = np.full(n, 77, np.int32)
        off = np.full(n + 1, 99, np.uint64)
        idx = np.full(n, -7, np.int32)
        k, nc = C.c_uint64(123), C.c_uint64(456)
        st = gpu.lib.pclhip_euclidean_clusters(tree.h, 0.01, 1, 0xFFFFFFFF, C.c_void_p(lab.ctypes.data) if with_labels else None,
                                               off.ctypes.data_as(u64p), off_cap, C.c_void_p(idx.ctypes.data), idx_cap,
                                               C.byref(k), C.byref(nc))
        return st, lab, off, idx, k.value, nc.value

    for off_cap, idx_cap in ((len(rc), n), (n + 1, rn - 1), (0, 0)):
        st, lab, off, idx, k, nc = call(off_cap, idx_cap)
        assert st == -5 and k == len(rc) and nc == rn and np.array_equal(lab, rl)  # PCLHIP_ERR_OVERFLOW, counts + labels
    st, lab, off, idx, k, nc = call(len(rc) + 1, rn)  # exactly enough
    assert st == 0 and np.array_equal(idx[:rn], np.concatenate(rc)) and off[len(rc)] == rn and off[len(rc) + 1] == 99
    # every output is optional: the counts alone
    k, nc = C.c_uint64(0), C.c_uint64(0)
    assert gpu.lib.pclhip_euclidean_clusters(tree.h, 0.01, 1, 0xFFFFFFFF, None, None, 0, None, 0, C.byref(k), C.byref(nc)) == 0
    assert (k.value, nc.value) == (len(rc), rn)
    st = tree.lastKernelMs()
    assert st > 0.0


def test_torch_device_buffers(gpu, bun0):
    import torch
    cloud = torch.from_numpy(bun0).cuda()
    e = extractor(gpu, cloud, 0.01)
    off, idx, lab = e.extractCSR()
    assert idx.is_cuda and lab.is_cuda and idx.dtype == torch.int32
    rc, rl, rn = cr.euclidean_clusters(bun0, 0.01)
    assert np.array_equal(idx.cpu().numpy(), np.concatenate(rc)) and np.array_equal(lab.cpu().numpy(), rl)
    assert np.diff(off.astype(np.int64)).tolist() == [357, 23, 12, 3, 1, 1]
    off2, idx2, lab2 = e.extractCSR()
    assert torch.equal(idx, idx2) and torch.equal(lab, lab2)
    clusters = e.extract()
    assert all(c.is_cuda for c in clusters) and [len(c) for c in clusters] == [357, 23, 12, 3, 1, 1]
