"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle.

Bars: bit-exact for indices and squared distances; float tolerances are written in each test.
Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def xyz1(a):
    out = np.ones((len(a), 4), np.float32)
    out[:, :3] = a[:, :3]
    return out


@pytest.fixture(scope="module")
def gpu():
    import pcl_amd
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


def build_tree(gpu, cloud, indices=None):
    import pcl_amd
    t = pcl_amd.KdTree(gpu)
    t.setInputCloud(cloud, indices)
    return t


# ------------------------------------------------------------------------------------------------
# k-NN
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8, 10, 16, 20, 32, 64, 512])
def test_knn_random_vs_bruteforce(gpu, orc, k):
    # test/search/test_search.cpp:292-364 (k in {1,8,64,512}, 1200 random points), plus the
    # register (k<=32) / heap (k>32) boundaries
    rng = np.random.default_rng(100 + k)
    pts = rng.uniform(0, 1, (1200, 3)).astype(np.float32)
    qry = rng.uniform(-0.1, 1.1, (777, 3)).astype(np.float32)
    gi, gd = build_tree(gpu, pts).nearestKSearch(qry, k)
    oi, od = orc.knn_bruteforce(pts, qry, k)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od)
    assert np.all(np.diff(gd, axis=1) >= 0)


def test_knn_hand_points_golden(gpu, golden):
    # test/kdtree/test_kdtree.cpp:226-289: the default representation, CustomPointRepresentation(2) (x-y only)
    # and rescale values (1, 2, 3) -- through setPointRepresentation, the points are handed over unscaled
    import pcl_amd
    g = golden["kdtree_hand"]
    pts = np.asarray(g["points"], np.float32)
    qry = np.asarray([g["query"]], np.float32)
    for name, rep in (("xyz", {}), ("xy", {"dimensions": 2}), ("rescaled_123", {"rescale_values": (1, 2, 3)})):
        tree = pcl_amd.KdTree(gpu)
        tree.setPointRepresentation(**rep)
        tree.setInputCloud(pts)
        idx, d2 = tree.nearestKSearch(qry, 10)
        assert idx[0].tolist() == g[name]["indices"], name
        assert np.allclose(d2[0], g[name]["distances"], atol=g["dist_tol"])
    # an axis the representation does not contain need not be finite (point_representation.h:103-135)
    pts2 = pts.copy()
    pts2[3, 2] = np.nan
    tree = pcl_amd.KdTree(gpu)
    tree.setPointRepresentation(dimensions=2)
    tree.setInputCloud(pts2)
    assert tree.size() == len(pts2)
    idx2, _ = tree.nearestKSearch(qry, 10)
    assert idx2[0].tolist() == g["xy"]["indices"]
    # registration needs the default representation: refused loudly
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setSearchMethodTarget(tree, True)
    icp.setInputSource(pts)
    with pytest.raises(pcl_amd.PclHipError, match="rescale"):
        icp.align()


def test_source_and_target_index_subsets(gpu, orc, bunny):
    # PCLBase::setIndices on the registration (common/include/pcl/pcl_base.h:102-125) and
    # CorrespondenceEstimationBase::setIndicesSource / setIndicesTarget (correspondence_estimation.h:194,210):
    # only the listed points take part; indices in the results refer to the original clouds
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    rng = np.random.default_rng(4)
    si = np.sort(rng.choice(len(src), 150, replace=False)).astype(np.int32)
    ti = np.sort(rng.choice(len(tgt), 200, replace=False)).astype(np.int32)
    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputSource(src)
    ce.setIndicesSource(si)
    ce.setIndicesTarget(ti)
    ce.setInputTarget(tgt)
    q, m, d = ce.determineCorrespondences(0.05)
    oq, om, od = orc.KdTree(tgt[ti]).correspondences(src[si], 0.05)
    assert np.array_equal(q, si[oq]) and np.array_equal(m, ti[om]) and np.array_equal(d, od)
    # the whole loop on a source subset == the loop on the extracted sub-cloud
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setIndices(si)
    icp.setMaximumIterations(30)
    icp.setMaxCorrespondenceDistance(0.05)
    icp.align()
    ref = pcl_amd.IterativeClosestPoint(gpu)
    ref.setInputTarget(tgt)
    ref.setInputSource(np.ascontiguousarray(src[si]))
    ref.setMaximumIterations(30)
    ref.setMaxCorrespondenceDistance(0.05)
    ref.align()
    assert icp.nr_iterations_ == ref.nr_iterations_
    assert np.abs(icp.getFinalTransformation() - ref.getFinalTransformation()).max() < 1e-6
    qq, mm, dd = icp.fetchCorrespondences()
    assert set(qq.tolist()) <= set(si.tolist()) and len(qq) > 100
    with pytest.raises(pcl_amd.PclHipError, match="indices"):
        bad = pcl_amd.IterativeClosestPoint(gpu)
        bad.setInputTarget(tgt)
        bad.setInputSource(src)
        bad.setIndices(np.asarray([0, len(src)], np.int32))
        bad.align()


def test_knn_lattice_ties_lowest_index(gpu, orc):
    # 11^3 lattice (test/kdtree/test_kdtree.cpp:161-208): masses of exact distance ties, the lower
    # index must win exactly as in the oracle
    g = np.arange(-5, 6, dtype=np.float32) * np.float32(0.1)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(7)
    qry = np.concatenate([pts[::17], rng.uniform(-0.6, 0.6, (200, 3)).astype(np.float32)])
    tree = build_tree(gpu, pts)
    for k in (1, 8, 20, 40):
        gi, gd = tree.nearestKSearch(qry, k)
        oi, od = orc.knn_bruteforce(pts, qry, k)
        assert np.array_equal(gi, oi), k
        assert np.array_equal(gd, od), k


@pytest.mark.parametrize("nq", [1, 7, 64, 65, 1000, 4000])
def test_knn_few_queries_against_a_large_index(gpu, orc, nq):
    # A batch that is SPARSE against the index is laid out with fewer queries per wavefront (api.hip: sparse_fill -- 64
    # scattered queries would make one wavefront walk the tree for the box of all of them; measured 117 ms for 16 queries
    # against 10M points).  Same results as any other batch: host and (GPU tier) device buffers, k in registers and in the
    # heap, non-finite queries in the batch, a subset index.
    import pcl_amd
    rng = np.random.default_rng(nq)
    tgt, _, _ = pcl_amd.synth.icp_pair(120_000)
    qry = np.ascontiguousarray(tgt[rng.integers(0, len(tgt), nq)] + rng.normal(scale=0.01, size=(nq, 4)).astype(np.float32))
    if nq >= 7:
        qry[3, 1] = np.nan
        qry[nq - 1, 0] = np.inf
    tree = build_tree(gpu, tgt)
    otree = orc.KdTree(tgt)
    for k in (1, 8, 40):
        gi, gd = tree.nearestKSearch(qry, k)
        oi, od = otree.knn(qry, k)
        assert np.array_equal(gi, oi) and np.array_equal(gd.view(np.uint32), od.view(np.uint32)), (nq, k)
    on_device = b"wavesim" not in pcl_amd._lib.load().pclhip_version()   # (the emulation of the CPU tier has no device memory)
    if on_device:
        import torch  # device-resident queries and results (the dump row of the padding slots is not the caller's buffer)
        di, dd = tree.nearestKSearch(torch.from_numpy(qry).cuda(), 8)
        oi, od = otree.knn(qry, 8)
        assert di.is_cuda and np.array_equal(di.cpu().numpy(), oi) and np.array_equal(dd.cpu().numpy().view(np.uint32), od.view(np.uint32))
    if nq in (7, 1000):  # through a rescaling point representation: the queries are mapped into the index's space on the way
        tree3 = pcl_amd.KdTree(gpu)
        tree3.setPointRepresentation(rescale_values=(1, 2, 0.5))
        tree3.setInputCloud(tgt)
        sc = np.array([1, 2, 0.5, 1], np.float32)
        ok = np.isfinite(qry).all(axis=1)
        gi, gd = tree3.nearestKSearch(qry, 5)
        oi, od = orc.KdTree(tgt * sc).knn(np.ascontiguousarray(qry * sc), 5)
        assert np.array_equal(gi[ok], oi[ok]) and np.array_equal(gd[ok].view(np.uint32), od[ok].view(np.uint32))
    sub = np.ascontiguousarray(rng.permutation(len(tgt))[:50_000].astype(np.int32))
    tree2 = build_tree(gpu, tgt, sub)
    gi, gd = tree2.nearestKSearch(qry, 3)
    oi, od = orc.KdTree(tgt[np.sort(sub)]).knn(qry, 3)
    assert np.array_equal(gd.view(np.uint32), od.view(np.uint32))
    assert np.array_equal(np.sort(sub)[np.where(oi >= 0, oi, 0)] * (oi >= 0) - (oi < 0), gi)


def test_tie_policy_where_first_visited_and_lowest_index_differ(gpu, orc, bunny, golden):
    """Exact distance ties are the one place where this library's answer is a POLICY, not the reference's arithmetic:
    FLANN's result set keeps the FIRST-VISITED of tied candidates (strict `<` on insertion; the nearer child of a split is
    descended first -- SURVEY.md 8(c), FLANN 1.9.1 KDTreeSingleIndex::searchLevel: child1 iff (val - divlow) + (val -
    divhigh) < 0), this library and its oracle keep the LOWER INDEX.  A cloud built so that the two rules disagree:

        left cluster  x in [-3, -1], nearest point A = (-1, 0, 0) with index 5
        right cluster x in [ 1,  3], nearest point B = ( 1, 0, 0) with index 40
        query (0, 0, 0): |q - A|^2 = |q - B|^2 = 1.0f exactly

    The widest axis is x, the cut leaves divlow = -1, divhigh = +1: (0 + 1) + (0 - 1) = 0 is not < 0, so FLANN descends
    the RIGHT child first, finds B at 1.0, then visits the left child (cut distance 1.0 <= worst) where A's 1.0 is not
    < 1.0: FLANN answers 40.  Lowest-index answers 5.  Which of the two do the reference's own tests admit?  BOTH:
      * its cross-backend test of the two kd-trees it ships accepts "index equal OR distance equal" per neighbour
        (test/search/test_kdtree_nanoflann.cpp:314-317) -- PCL does not pin the tie order between its own backends;
      * the exact-pair goldens (397 + 53 bunny correspondences, test/registration/test_registration_api_data.h) contain
        no exact tie at all (checked below by brute force), so they cannot tell the rules apart.
    So the lower index is a documented deviation inside what the reference admits, not a mismatch."""
    rng = np.random.default_rng(11)
    left = np.stack([rng.uniform(-3, -1.25, 24), rng.uniform(-0.5, 0.5, 24), rng.uniform(-0.5, 0.5, 24)], 1)
    right = np.stack([rng.uniform(1.25, 3, 24), rng.uniform(-0.5, 0.5, 24), rng.uniform(-0.5, 0.5, 24)], 1)
    pts = np.concatenate([left, right]).astype(np.float32)          # 48 points: FLANN (leaf_max_size 15) must split
    pts[5] = (-1.0, 0.0, 0.0)                                         # A, in the left cluster
    pts[40] = (1.0, 0.0, 0.0)                                         # B, in the right cluster
    q = np.zeros((1, 3), np.float32)
    d = ((pts.astype(np.float32) - q) ** 2).sum(axis=1, dtype=np.float32)
    assert d[5] == d[40] == np.float32(1.0) and np.sum(d <= np.float32(1.0)) == 2
    # the first-visited rule on this cloud, as derived above
    divlow, divhigh = pts[:24, 0].max(), pts[24:, 0].min()
    assert (divlow, divhigh) == (np.float32(-1.0), np.float32(1.0))
    flann_first_child_is_right = not ((q[0, 0] - divlow) + (q[0, 0] - divhigh) < 0)
    first_visited = 40 if flann_first_child_is_right else 5
    assert first_visited == 40
    tree = build_tree(gpu, pts)
    gi, gd = tree.nearestKSearch(q, 2)
    oi, od = orc.KdTree(np.concatenate([pts, np.ones((48, 1), np.float32)], 1)).knn(
        np.concatenate([q, np.ones((1, 1), np.float32)], 1), 2)
    assert gi.tolist() == [[5, 40]] and np.array_equal(gi, oi) and np.array_equal(gd, od)    # lower index first, both at 1.0
    assert gi[0, 0] != first_visited and gd[0, 0] == gd[0, 1] == np.float32(1.0)
    # the reference's own acceptance criterion between its backends: index equal OR distance equal
    assert gi[0, 0] == first_visited or gd[0, 0] == d[first_visited]
    # ... and the exact-pair goldens hold no tie: brute force over the bunny pair, float L2_Simple
    src, tgt = bunny["bun0"][:, :3].astype(np.float32), bunny["bun4"][:, :3].astype(np.float32)
    bi, bd = orc.knn_bruteforce(tgt, src, 2)
    assert not np.any(bd[:, 0] == bd[:, 1])
    assert np.array_equal(bi[:, 0], np.asarray(golden["correspondences_original"])[:, 1])


@pytest.mark.parametrize("n", [4095, 4096, 4097, 16384, 16385, 65536 + 17, 300_001])
def test_knn_index_build_segment_boundaries(gpu, orc, n):
    # The index build cuts segments above 4096 points by radix selection + partition (ties at a quartile are
    # split by count) and orders the rest inside one workgroup: sizes around the 4096 / 16384 / 65536 segment
    # boundaries, with partial last segments, on data full of equal coordinates -- a lattice (every splitter is a
    # tie), a cloud with one constant axis pair (zero-bit key range in later rounds) and many exact duplicates.
    rng = np.random.default_rng(n)
    lattice = np.stack([rng.integers(0, 40, n), rng.integers(0, 40, n), rng.integers(0, 3, n)], 1).astype(np.float32) * 0.25
    line = np.zeros((n, 3), np.float32)
    line[:, 0] = rng.normal(size=n).astype(np.float32)
    line[:, 1] = 0.5
    dup = rng.uniform(-1, 1, (max(n // 7, 1), 3)).astype(np.float32)[rng.integers(0, max(n // 7, 1), n)]
    for name, pts in (("lattice", lattice), ("line", line), ("duplicates", dup)):
        qry = (pts[rng.integers(0, n, 2000)] + rng.normal(scale=0.05, size=(2000, 3))).astype(np.float32)
        tree = build_tree(gpu, pts)
        assert tree.size() == n
        gi, gd = tree.nearestKSearch(qry, 4)
        oi, od = orc.KdTree(pts).knn(qry, 4)
        assert np.array_equal(gd, od), (name, n)
        assert np.array_equal(gi, oi), (name, n)
        # the same cloud again on the warm context (recycled allocations), with a few non-finite records mixed in
        bad = pts.copy()
        bad[rng.integers(0, n, 5)] = np.nan
        ok = np.isfinite(bad).all(1)
        gi2, gd2 = build_tree(gpu, bad).nearestKSearch(qry, 4)
        oi2, od2 = orc.KdTree(bad).knn(qry, 4)
        assert np.array_equal(gd2, od2) and np.array_equal(gi2, oi2), (name, n)
        assert ok[gi2[gi2 >= 0]].all()


def test_knn_duplicates_and_nonfinite(gpu, orc):
    rng = np.random.default_rng(3)
    pts = rng.normal(0, 1, (5000, 3)).astype(np.float32)
    pts[100:200] = pts[0:100]            # exact duplicates -> ties
    pts[7] = np.nan                      # dropped (kdtree_flann.hpp:443-452)
    pts[4999, 1] = np.inf
    qry = rng.normal(0, 1, (1000, 3)).astype(np.float32)
    qry[5] = np.nan                      # no neighbours
    tree = build_tree(gpu, pts)
    assert tree.size() == 4998
    for k in (1, 8):
        gi, gd = tree.nearestKSearch(qry, k)
        oi, od = orc.knn_bruteforce(pts, qry, k)
        assert np.array_equal(gi, oi) and np.array_equal(gd, od)
        assert np.all(gi[5] == -1) and np.all(np.isinf(gd[5]))


def test_knn_k_larger_than_cloud_and_tiny_clouds(gpu, orc):
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 15, 16, 17, 63, 64, 65, 1025):
        pts = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        qry = rng.uniform(0, 1, (70, 3)).astype(np.float32)
        for k in (1, 8, 40):
            gi, gd = build_tree(gpu, pts).nearestKSearch(qry, k)
            oi, od = orc.knn_bruteforce(pts, qry, k)
            assert np.array_equal(gi, oi), (n, k)
            assert np.array_equal(gd, od), (n, k)


def test_knn_empty_inputs(gpu):
    tree = build_tree(gpu, np.zeros((0, 4), np.float32))
    assert tree.size() == 0
    idx, d2 = tree.nearestKSearch(np.zeros((3, 4), np.float32), 2)
    assert np.all(idx == -1) and np.all(np.isinf(d2))
    tree = build_tree(gpu, np.random.default_rng(1).uniform(0, 1, (10, 3)).astype(np.float32))
    idx, d2 = tree.nearestKSearch(np.zeros((0, 3), np.float32), 2)
    assert idx.shape == (0, 2)


def test_knn_with_indices_subset(gpu, orc):
    # KdTreeFLANN::setInputCloud(cloud, indices): results index the ORIGINAL cloud
    rng = np.random.default_rng(11)
    pts = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    sel = np.sort(rng.choice(3000, 1000, replace=False)).astype(np.int32)
    qry = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    gi, gd = build_tree(gpu, pts, sel).nearestKSearch(qry, 4)
    oi, od = orc.knn_bruteforce(pts[sel], qry, 4)
    assert np.array_equal(gi, sel[oi]) and np.array_equal(gd, od)


def test_knn_strided_pointnormal_records(gpu, orc):
    rng = np.random.default_rng(12)
    rec = rng.uniform(0, 1, (2000, 12)).astype(np.float32)  # 48-byte pcl::PointNormal-like records
    qry = rng.uniform(0, 1, (300, 12)).astype(np.float32)
    gi, gd = build_tree(gpu, rec).nearestKSearch(qry, 8)
    oi, od = orc.knn_bruteforce(rec[:, :3], qry[:, :3], 8)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_knn_synthetic_surface_200k(gpu, orc):
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(200_000)
    tree = build_tree(gpu, tgt)
    otree = orc.KdTree(tgt)
    for k in (1, 8):
        gi, gd = tree.nearestKSearch(src, k)
        oi, od = otree.knn(src, k)
        assert np.array_equal(gi, oi), k
        assert np.array_equal(gd, od), k


def test_knn_far_queries_and_clustered_target(gpu, orc):
    # queries far outside the target's bounding box, a target with a dense cluster + outliers
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.normal(0, 1e-3, (20000, 3)), rng.uniform(-50, 50, (200, 3))]).astype(np.float32)
    qry = np.concatenate([rng.uniform(-200, 200, (500, 3)), rng.normal(0, 2e-3, (500, 3))]).astype(np.float32)
    gi, gd = build_tree(gpu, pts).nearestKSearch(qry, 8)
    oi, od = orc.KdTree(pts).knn(qry, 8)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_knn_device_resident_torch_buffers(gpu, orc):
    import torch
    rng = np.random.default_rng(21)
    pts = rng.uniform(0, 1, (50000, 4)).astype(np.float32)
    qry = rng.uniform(0, 1, (10000, 4)).astype(np.float32)
    tp, tq = torch.from_numpy(pts).cuda(), torch.from_numpy(qry).cuda()
    gi, gd = build_tree(gpu, tp).nearestKSearch(tq, 8)
    assert gi.is_cuda and gd.is_cuda
    oi, od = orc.KdTree(pts).knn(qry, 8)
    assert np.array_equal(gi.cpu().numpy(), oi) and np.array_equal(gd.cpu().numpy(), od)


# ------------------------------------------------------------------------------------------------
# CorrespondenceEstimation
# ------------------------------------------------------------------------------------------------
def test_correspondences_bunny_golden(gpu, bunny, golden):
    # test/registration/test_registration_api.cpp:83-104 -- 397 exact pairs
    import pcl_amd
    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputSource(xyz1(bunny["bun0"]))
    ce.setInputTarget(xyz1(bunny["bun4"]))
    q, m, d = ce.determineCorrespondences()
    gold = np.asarray(golden["correspondences_original"], np.int32)
    assert np.array_equal(q, gold[:, 0]) and np.array_equal(m, gold[:, 1])


def test_correspondences_max_distance(gpu, orc, bunny):
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    src[11, 0] = np.nan  # non-finite source points are skipped (correspondence_estimation.hpp:173-174)
    otree = orc.KdTree(tgt)
    for md in (0.002, 0.01, 0.05):
        ce = pcl_amd.CorrespondenceEstimation(gpu)
        ce.setInputSource(src)
        ce.setInputTarget(tgt)
        q, m, d = ce.determineCorrespondences(md)
        oq, om, od = otree.correspondences(src, md)
        assert np.array_equal(q, oq) and np.array_equal(m, om) and np.array_equal(d, od), md
        assert 0 < len(q) < 397


# ------------------------------------------------------------------------------------------------
# ICP
# ------------------------------------------------------------------------------------------------
def run_icp_pair(gpu, orc, tgt, src, mode, normals=None, **kw):
    import pcl_amd
    cls = pcl_amd.IterativeClosestPointWithNormals if mode == 1 else pcl_amd.IterativeClosestPoint
    icp = cls(gpu)
    icp.setInputTarget(tgt)
    if normals is not None:
        icp.setTargetNormals(normals)
    icp.setInputSource(src)
    icp.setMaximumIterations(kw["max_iterations"])
    if "max_correspondence_distance" in kw:
        icp.setMaxCorrespondenceDistance(kw["max_correspondence_distance"])
    if "transformation_epsilon" in kw:
        icp.setTransformationEpsilon(kw["transformation_epsilon"])
    icp.align()
    ref = orc.icp_align(orc.KdTree(tgt), tgt, src, mode=mode, tgt_normals=normals, record=True, **kw)
    return icp, ref


def test_icp_bunny_golden_and_oracle(gpu, orc, bunny, golden):
    # test/registration/test_registration.cpp:236-270
    g = golden["icp_bunny"]
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    icp, ref = run_icp_pair(gpu, orc, tgt, src, 0, max_iterations=g["max_iterations"],
                            transformation_epsilon=g["transformation_epsilon"],
                            max_correspondence_distance=g["max_correspondence_distance"])
    T = icp.getFinalTransformation()
    assert np.all(np.abs(T[:3] - np.asarray(g["rows"])) <= np.asarray(g["tol"])), T
    assert T[3].tolist() == [0, 0, 0, 1]
    assert icp.hasConverged()
    # vs the oracle: same iteration count, final 4x4 within 1e-5 Frobenius (north_star tolerance)
    assert icp.nr_iterations_ == ref["iterations"]
    assert icp.getConvergenceState() == ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE",
                                         "NO_CORRESPONDENCES", "FAILURE")[ref["state"]]
    assert np.linalg.norm(T.astype(np.float64) - ref["T"]) < 1e-5


def test_icp_per_iteration_correspondences_bit_exact(gpu, orc, bunny):
    # drive the fused iteration by hand with the ORACLE's per-iteration transforms: every
    # iteration's matches must equal the oracle's bit for bit (same float transform order)
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    ref = orc.icp_align(orc.KdTree(tgt), tgt, src, mode=0, max_iterations=12,
                        max_correspondence_distance=0.05, transformation_epsilon=1e-9, record=True)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setMaxCorrespondenceDistance(0.05)
    icp.reset()
    T_prev = np.eye(4, dtype=np.float32)
    for it in range(ref["iterations"]):
        sums = icp.iterate(T_prev)
        q, m, d = icp.fetchCorrespondences()
        row = ref["per_iter_match"][it]
        assert np.array_equal(q, np.nonzero(row >= 0)[0]), it
        assert np.array_equal(m, row[row >= 0]), it
        assert int(sums[28]) == len(q)
        T_prev = ref["per_iter_T"][it]
        # the host closed form agrees with the oracle's estimate for this iteration (fp64 sums vs
        # the oracle's float sums: 1e-5)
        assert np.abs(icp.solve(sums) - T_prev).max() < 1e-5, it


def test_icp_translation_recovery(gpu, bunny):
    # test/registration/test_registration.cpp:161-195
    import pcl_amd
    src = xyz1(bunny["bun0"])
    tgt = src.copy()
    tgt[:, 2] += np.float32(0.2)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setMaximumIterations(50)
    out = icp.align(want_output=True)
    T = icp.getFinalTransformation()
    assert np.abs(T[:3, :3] - np.eye(3)).max() < 2e-3 and np.abs(T[:3, 3] - [0, 0, 0.2]).max() < 2e-3
    assert np.abs(out[:, :3] - tgt[:, :3]).max() < 5e-3


def test_icp_with_normals_bunny(gpu, orc, bunny):
    # test/registration/test_registration.cpp:272-318: NormalEstimation(k=10) + ICPWithNormals
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    tree = build_tree(gpu, tgt)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(tgt)
    ne.setSearchMethod(tree)
    ne.setKSearch(10)
    nrm = ne.compute()
    onrm, nan = orc.KdTree(tgt).normals(tgt, 10)
    assert ne.nan_count == nan == 0
    assert np.abs(np.sum(nrm[:, :3] * onrm[:, :3], axis=1)).min() > 1 - 1e-5
    icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
    icp.setSearchMethodTarget(tree)
    icp.setInputSource(src)
    icp.setMaximumIterations(50)
    icp.setTransformationEpsilon(1e-8)
    icp.align()
    ref = orc.icp_align(orc.KdTree(tgt), tgt, src, mode=1, tgt_normals=onrm, max_iterations=50,
                        transformation_epsilon=1e-8)
    assert icp.hasConverged() and icp.nr_iterations_ == ref["iterations"]
    T = icp.getFinalTransformation()
    assert np.linalg.norm(T.astype(np.float64) - ref["T"]) < 1e-5
    out = orc.transform_cloud(T, src, order=1)
    _, d2 = orc.KdTree(tgt).knn(out, 1)
    assert float(d2.mean()) < 1e-3  # fitness bar of the reference test


def test_icp_point_to_plane_lls_sums_match_oracle(gpu, orc):
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(50_000)
    otree = orc.KdTree(tgt)
    onrm, _ = otree.normals(tgt, 8, viewpoint=(0, 0, 10))
    icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
    icp.setInputTarget(tgt)
    icp.setTargetNormals(onrm)
    icp.setInputSource(src)
    icp.reset()
    sums = icp.iterate(np.eye(4, dtype=np.float32), max_dist=0.1)
    q, m, d = otree.correspondences(src, 0.1)
    T, osums, used = orc.lls_point_to_plane(src, tgt, onrm, q, m)
    assert int(sums[28]) == len(q) == used
    assert np.allclose(sums[:27], osums, rtol=1e-11, atol=1e-13)   # fp64 sums, different order
    assert abs(sums[27] - d.astype(np.float64).sum()) <= 1e-12 * len(q)
    assert np.abs(icp.solve(sums) - T).max() < 1e-6


@pytest.mark.parametrize("mode", [0, 1])
def test_icp_synthetic_100k_vs_oracle(gpu, orc, mode):
    # BASELINE.json configs 2/3 at a size the oracle finishes in seconds
    import pcl_amd
    tgt, src, T_gt = pcl_amd.synth.icp_pair(100_000)
    otree = orc.KdTree(tgt)
    normals = otree.normals(tgt, 8, viewpoint=(0, 0, 10))[0] if mode == 1 else None
    kw = dict(max_iterations=20, max_correspondence_distance=0.1, transformation_epsilon=1e-10)
    icp, ref = run_icp_pair(gpu, orc, tgt, src, mode, normals=normals, **kw)
    T = icp.getFinalTransformation().astype(np.float64)
    assert icp.nr_iterations_ == ref["iterations"]
    assert np.linalg.norm(T - ref["T"]) < 1e-5, np.linalg.norm(T - ref["T"])
    # and it actually registers the clouds (point-to-point slides slowly along the surface: after
    # 20 iterations it is only part of the way, point-to-plane is there in a handful)
    assert np.linalg.norm(T - T_gt) < (2e-3 if mode == 1 else 2e-2)
    # Last-iteration correspondences: the GPU solved every iteration from fp64 tree-reduced sums,
    # the oracle from its own (float for umeyama / serial double for LLS) sums, so the two working
    # clouds differ in the last float bits and a few near-equidistant matches may flip.  (Bit-exact
    # per-iteration parity under IDENTICAL transforms is test_icp_per_iteration_* / *_driven_*.)
    q, m, d = icp.fetchCorrespondences()
    row = ref["per_iter_match"][ref["iterations"] - 1]
    assert np.array_equal(q, np.nonzero(row >= 0)[0])
    assert np.mean(m == row[row >= 0]) > 0.999


@pytest.mark.parametrize("mode", [0, 1])
def test_icp_synthetic_driven_by_oracle_transforms_bit_exact(gpu, orc, mode):
    # same clouds, but every GPU iteration is fed the ORACLE's transform: all matches bit-exact
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(100_000)
    otree = orc.KdTree(tgt)
    normals = otree.normals(tgt, 8, viewpoint=(0, 0, 10))[0] if mode == 1 else None
    ref = orc.icp_align(otree, tgt, src, mode=mode, tgt_normals=normals, record=True, max_iterations=6,
                        max_correspondence_distance=0.1, transformation_epsilon=1e-10)
    cls = pcl_amd.IterativeClosestPointWithNormals if mode == 1 else pcl_amd.IterativeClosestPoint
    icp = cls(gpu)
    icp.setInputTarget(tgt)
    if normals is not None:
        icp.setTargetNormals(normals)
    icp.setInputSource(src)
    icp.reset()
    T_prev = np.eye(4, dtype=np.float32)
    for it in range(ref["iterations"]):
        sums = icp.iterate(T_prev, max_dist=0.1)
        q, m, d = icp.fetchCorrespondences()
        row = ref["per_iter_match"][it]
        assert np.array_equal(q, np.nonzero(row >= 0)[0]), it
        assert np.array_equal(m, row[row >= 0]), it
        # float-sum umeyama (mode 0) carries ~1e-5 noise at 1e5 points; LLS sums are double
        assert np.abs(icp.solve(sums) - ref["per_iter_T"][it]).max() < (2e-5 if mode == 0 else 1e-6), it
        T_prev = ref["per_iter_T"][it]


@pytest.mark.parametrize("ns", [1, 5, 64, 300, 2000, 9000])
def test_icp_sparse_source_against_a_large_target(gpu, orc, ns):
    # A source that is SPARSE against the target (a small scan against a large map, spread over it) is searched with
    # fewer points per wavefront (search.hip: search_fill_of -- 64, 32, ... 1 consecutive points of the source's kd order,
    # so that a wavefront's box stays compact): same correspondences as any other source, in the launch that starts the
    # alignment and in the seeded ones, host-driven and in the device-driven loop, with a non-finite point in the source.
    import pcl_amd
    tgt, src_all, _ = pcl_amd.synth.icp_pair(150_000)
    rng = np.random.default_rng(ns)
    src = np.ascontiguousarray(src_all[rng.permutation(len(src_all))[:ns]])
    if ns >= 64:
        src[7, 2] = np.nan
    otree = orc.KdTree(tgt)
    normals = otree.normals(tgt, 8, viewpoint=(0, 0, 10))[0]
    for mode in (0, 1):
        cls = pcl_amd.IterativeClosestPointWithNormals if mode == 1 else pcl_amd.IterativeClosestPoint
        icp = cls(gpu)
        icp.setInputTarget(tgt)
        if mode == 1:
            icp.setTargetNormals(normals)
        icp.setInputSource(src)
        icp.reset()
        T = np.eye(4, dtype=np.float32)
        cur = src.copy()
        for it in range(4):                       # the launch without seeds, then seeded ones
            sums = icp.iterate(T, max_dist=0.1)
            cur = orc.transform_cloud(T, cur, order=mode)
            oq, om, od = otree.correspondences(cur, 0.1)
            q, m, d = icp.fetchCorrespondences()
            assert np.array_equal(q, oq) and np.array_equal(m, om), (ns, mode, it)
            assert np.array_equal(d.view(np.uint32), od.view(np.uint32)), (ns, mode, it)
            assert int(sums[28]) == len(oq)
            if len(oq) < 3:
                break
            T = icp.solve(sums)
        if ns >= 300:                             # the device-driven loop: same iteration count, the 4x4 within the contract
            kw = dict(max_iterations=15, max_correspondence_distance=0.1, transformation_epsilon=1e-10)
            icp2, ref = run_icp_pair(gpu, orc, tgt, src, mode, normals=normals if mode == 1 else None, **kw)
            assert icp2.nr_iterations_ == ref["iterations"]
            assert np.linalg.norm(icp2.getFinalTransformation().astype(np.float64) - ref["T"]) < 1e-5
            # getFitnessScore searches the same sparse source (impl/registration.hpp:132-168)
            Tf = icp2.getFinalTransformation()
            want, _ = otree.fitness_score(src, Tf, 1e-4)
            assert abs(icp2.getFitnessScore(1e-4) - want) <= 1e-6 * abs(want)


def test_icp_guess_and_repeated_align(gpu, orc, bunny):
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    th = 0.05
    G = np.eye(4, dtype=np.float32)
    G[0, 0] = G[1, 1] = np.cos(th)
    G[0, 1] = -np.sin(th)
    G[1, 0] = np.sin(th)
    G[:3, 3] = (0.01, -0.02, 0.005)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setMaximumIterations(30)
    icp.setMaxCorrespondenceDistance(0.05)
    icp.setTransformationEpsilon(1e-8)
    conv = orc.new_convergence()
    for rep in range(2):  # the criteria's previous-MSE memory persists across align() calls
        icp.align(guess=G)
        ref = orc.icp_align(orc.KdTree(tgt), tgt, src, mode=0, guess=G, conv=conv, max_iterations=30,
                            max_correspondence_distance=0.05, transformation_epsilon=1e-8)
        assert icp.nr_iterations_ == ref["iterations"], rep
        assert np.linalg.norm(icp.getFinalTransformation().astype(np.float64) - ref["T"]) < 1e-5


def test_icp_not_enough_correspondences(gpu, bunny):
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    src[:, 0] += 10.0
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setMaxCorrespondenceDistance(0.01)
    icp.align()
    assert not icp.hasConverged() and icp.getConvergenceState() == "NO_CORRESPONDENCES"
    assert icp.nr_iterations_ == 0


def test_point_to_plane_requires_normals(gpu, bunny):
    import pcl_amd
    icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
    icp.setInputTarget(xyz1(bunny["bun4"]))
    icp.setInputSource(xyz1(bunny["bun0"]))
    with pytest.raises(pcl_amd.PclHipError):
        icp.align()


def test_transform_cloud_orders_bit_exact(gpu, orc):
    import pcl_amd
    rng = np.random.default_rng(9)
    pts = rng.normal(0, 1, (10000, 4)).astype(np.float32)
    pts[3, 1] = np.nan
    T = pcl_amd.synth.ground_truth_transform().astype(np.float32)
    for cls, order in ((pcl_amd.IterativeClosestPoint, 0), (pcl_amd.IterativeClosestPointWithNormals, 1)):
        out = cls(gpu).transformCloud(pts, T)
        ref = orc.transform_cloud(T, pts, order=order)
        assert np.array_equal(out[:, :3], ref[:, :3], equal_nan=True), order


# ------------------------------------------------------------------------------------------------
# NormalEstimation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 15, 40])
def test_normals_vs_oracle(gpu, orc, k):
    import pcl_amd
    tgt, _, _ = pcl_amd.synth.icp_pair(60_000)
    tgt[17] = np.nan
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(tgt)
    ne.setKSearch(k)
    ne.setViewPoint(0, 0, 10)
    nrm = ne.compute()
    onrm, nan = orc.KdTree(tgt).normals(tgt, k, viewpoint=(0, 0, 10))
    assert ne.nan_count == nan == 1 and np.all(np.isnan(nrm[17]))
    ok = ~np.isnan(onrm[:, 0])
    # float eigen-solve with device atan2f/cosf/sinf vs libm: direction within 1e-5 (|dot| >= 1-1e-5
    # after unit length), same orientation after the viewpoint flip, curvature to 1e-5 absolute
    dots = np.sum(nrm[ok, :3] * onrm[ok, :3], axis=1)
    assert dots.min() > 1 - 1e-5, dots.min()
    assert np.abs(nrm[ok, 3] - onrm[ok, 3]).max() < 1e-5
    assert np.allclose(np.linalg.norm(nrm[ok, :3], axis=1), 1, atol=1e-5)


def test_normals_bunny_translation_invariance(gpu, bunny):
    # test/features/test_normal_estimation.cpp:287-312
    import pcl_amd
    cloud = xyz1(bunny["bun0"])
    shifted = cloud.copy()
    shifted[:, :3] += np.array([123, -45, 98], np.float32)
    outs = []
    for c, vp in ((cloud, (0, 0, 0)), (shifted, (123, -45, 98))):
        ne = pcl_amd.NormalEstimation(gpu)
        ne.setInputCloud(c)
        ne.setKSearch(15)
        ne.setViewPoint(*vp)
        outs.append(ne.compute())
    assert np.all(np.abs(np.sum(outs[0][:, :3] * outs[1][:, :3], axis=1)) >= 1 - 1e-4)


def test_normals_too_few_neighbours(gpu):
    import pcl_amd
    pts = np.random.default_rng(2).uniform(0, 1, (2, 3)).astype(np.float32)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(pts)
    ne.setKSearch(8)
    nrm = ne.compute()
    assert np.all(np.isnan(nrm)) and ne.nan_count == 2


# ------------------------------------------------------------------------------------------------
# VoxelGrid
# ------------------------------------------------------------------------------------------------
def test_voxelgrid_bunny_golden(gpu, orc, bunny, golden):
    # test/filters/test_filters.cpp:566-596
    import pcl_amd
    g = golden["voxelgrid_bun0"]
    cloud = xyz1(bunny["bun0"])
    vg = pcl_amd.VoxelGrid(gpu)
    vg.setInputCloud(cloud)
    vg.setLeafSize(g["leaf"])
    out = vg.filter()
    assert len(out) == g["count"]
    assert np.array_equal(out, orc.voxelgrid(cloud, g["leaf"])[0])
    vg.setFilterFieldName("z")
    vg.setFilterLimits(g["z_min"], g["z_max"])
    out = vg.filter()
    assert len(out) == g["count_z"]
    assert np.allclose(out[0, :3], g["first_z"], atol=g["tol"])
    assert np.allclose(out[-1, :3], g["last_z"], atol=g["tol"])


def test_voxelgrid_pointnormal_and_downsample_all_data(gpu, orc):
    # VoxelGrid<PointNormal> (test/filters/test_filters.cpp:598-687 runs it on bun0 with normals):
    # setDownsampleAllData(true) -> CentroidPoint accumulators (accumulators.hpp:68-127: xyz and curvature
    # averaged, the normal = normalised sum); (false) -> only xyz, the rest zero (voxel_grid.hpp:790-799)
    import os
    import pcl_amd
    root = os.path.dirname(os.path.abspath(__file__))
    cloud, dense = pcl_amd.loadPCDFile(os.path.join(root, "golden", "pcd", "bun0.pcd"), with_normals=True)
    assert cloud.shape == (397, 12) and dense
    want_xyz, ids = orc.voxelgrid(cloud, 0.02)
    assert len(want_xyz) == 103
    # the whole record, exactly: tests/voxelgrid_restatement.py (float32 sums in ascending input order, the normal the sum
    # over its float norm, the curvature's mean; pinned without a GPU by tests/test_voxelgrid_restatement.py)
    import voxelgrid_restatement as vr
    for all_data in (True, False):
        vg = pcl_amd.VoxelGrid(gpu)
        vg.setInputCloud(cloud)
        vg.setLeafSize(0.02)
        vg.setDownsampleAllData(all_data)
        assert vg.getDownsampleAllData() == all_data
        out = vg.filter()
        assert out.shape == (103, 12)
        assert np.array_equal(out[:, :4], want_xyz)                  # the coordinates do not depend on the option
        ref = vr.voxelgrid(cloud, 0.02, downsample_all_data=all_data)
        assert np.array_equal(ref["ids"], ids)
        assert vr.same_bytes(out, ref["out"]), vr.first_difference(out, ref["out"])
        if not all_data:
            assert not out[:, 4:].any()
            continue
        assert np.all(np.abs(np.linalg.norm(out[:, 4:7].astype(np.float64), axis=1) - 1.0) < 1e-6)
        assert not out[:, 7].any() and not out[:, 9:].any()
    # device-resident PointNormal clouds take the same path
    import torch
    vg = pcl_amd.VoxelGrid(gpu)
    vg.setInputCloud(torch.from_numpy(cloud).cuda())
    vg.setLeafSize(0.02)
    dev = vg.filter().cpu().numpy()
    vg2 = pcl_amd.VoxelGrid(gpu)
    vg2.setInputCloud(cloud)
    vg2.setLeafSize(0.02)
    assert np.array_equal(dev, vg2.filter())


def test_voxelgrid_synthetic_bit_exact(gpu, orc):
    import pcl_amd
    tgt, _, _ = pcl_amd.synth.icp_pair(300_000)
    tgt[5] = np.nan
    for leaf, minpts in ((0.01, 0), (0.05, 0), (0.01, 6)):
        vg = pcl_amd.VoxelGrid(gpu)
        vg.setInputCloud(tgt)
        vg.setLeafSize(leaf)
        vg.setMinimumPointsNumberPerVoxel(minpts)
        out = vg.filter()
        ref, _ = orc.voxelgrid(tgt, leaf, min_points_per_voxel=minpts)
        assert out.shape == ref.shape and np.array_equal(out, ref), (leaf, minpts)


def test_voxelgrid_leaf_layout(gpu, orc, bunny):
    # setSaveLeafLayout (voxel_grid.h:316, impl/voxel_grid.hpp:752-787): layout[cell id] = position of the cell's
    # centroid in the output, -1 for empty cells and for cells dropped by min_points_per_voxel; cell ids follow
    # getMinBoxCoordinates / getDivisionMultiplier.  Checked against the voxel ids recomputed here with the
    # reference's float expressions (:713-718) and against the oracle's centroids.
    import pcl_amd
    rng = np.random.default_rng(11)
    big = np.ones((200_000, 4), np.float32)
    big[:, :3] = rng.uniform(-1, 1, (200_000, 3)).astype(np.float32) * np.float32([1.0, 0.7, 0.2])
    for cloud, leaf, min_pts in ((xyz1(bunny["bun0"]), 0.02, 0), (big, 0.05, 0), (big, 0.03, 3)):
        vg = pcl_amd.VoxelGrid(gpu)
        vg.setInputCloud(cloud)
        vg.setLeafSize(leaf)
        vg.setMinimumPointsNumberPerVoxel(min_pts)
        vg.setSaveLeafLayout(True)
        out = vg.filter()
        ref, ref_ids = orc.voxelgrid(cloud, leaf, min_points_per_voxel=min_pts)
        assert np.array_equal(out[:, :3], ref[:, :3])
        layout = vg.getLeafLayout()
        mn, div, mul = vg.getMinBoxCoordinates(), vg.getNrDivisions(), vg.getDivisionMultiplier()
        assert len(layout) == int(div[0]) * int(div[1]) * int(div[2])
        assert np.array_equal(mul, [1, div[0], div[0] * div[1]])
        assert np.array_equal(vg.getMaxBoxCoordinates(), mn + div - 1)
        inv = np.float32(1.0) / np.float32(leaf)
        ijk = np.floor(cloud[:, :3] * inv).astype(np.int64)
        assert np.array_equal(ijk.min(0), mn) and np.array_equal(ijk.max(0), mn + div - 1)
        ids = ((ijk - mn) * mul.astype(np.int64)).sum(1)
        cnt = np.bincount(ids, minlength=len(layout))
        kept = cnt >= max(min_pts, 1)
        assert np.array_equal(layout >= 0, kept)                             # exactly the kept cells
        assert np.array_equal(layout[kept], np.arange(kept.sum()))           # output order = ascending cell id
        assert len(out) == kept.sum()
        # the centroid a point's cell maps to lies in that cell (up to rounding of the mean at a cell face)
        pick = rng.integers(0, len(cloud), 200)
        for i in pick:
            j = vg.getCentroidIndex(cloud[i])
            assert j == layout[ids[i]]
            if j >= 0:
                assert np.all(np.abs(np.floor(out[j, :3] * inv) - ijk[i]) <= 1)
        assert vg.getCentroidIndexAt(mn - 1) == -1
        # without the flag nothing is kept
        vg.setSaveLeafLayout(False)
        vg.filter()
        assert len(vg.getLeafLayout()) == 0


def test_voxelgrid_overflow_refused(gpu):
    import pcl_amd
    pts = np.random.default_rng(4).uniform(-1000, 1000, (100, 3)).astype(np.float32)
    vg = pcl_amd.VoxelGrid(gpu)
    vg.setInputCloud(pts)
    vg.setLeafSize(1e-4)
    with pytest.raises(pcl_amd.PclHipError) as e:
        vg.filter()
    assert e.value.status == -5


# ------------------------------------------------------------------------------------------------
# rejectors + reciprocal correspondences
# ------------------------------------------------------------------------------------------------
def test_rejectors_bunny_goldens(gpu, bunny, golden):
    # test/registration/test_registration_api.cpp:131-380 on the device chain
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])

    def run(rej):
        ce = pcl_amd.CorrespondenceEstimation(gpu)
        ce.setInputSource(src)
        ce.setInputTarget(tgt)
        q, m, d = ce.determineCorrespondences(rejectors=[rej])
        return np.stack([q, m], 1)

    r = pcl_amd.CorrespondenceRejectorDistance()
    r.setMaximumDistance(golden["rej_dist_max_dist"])
    assert np.array_equal(run(r), np.asarray(golden["correspondences_dist"]))
    r = pcl_amd.CorrespondenceRejectorMedianDistance()
    r.setMedianFactor(golden["rej_median_factor"])
    assert np.array_equal(run(r), np.asarray(golden["correspondences_median_dist"]))
    assert abs(r.getMedianDistance() - golden["rej_median_distance"]) < 1e-4
    assert np.array_equal(run(pcl_amd.CorrespondenceRejectorOneToOne()), np.asarray(golden["correspondences_one_to_one"]))
    r = pcl_amd.CorrespondenceRejectorTrimmed()
    r.setOverlapRatio(golden["rej_trimmed_overlap"])
    assert np.array_equal(run(r), np.asarray(golden["correspondences_trimmed"]))


def test_reciprocal_correspondences_bunny_golden(gpu, bunny, golden):
    # test/registration/test_registration_api.cpp:107-128 -- 53 exact pairs
    import pcl_amd
    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputSource(xyz1(bunny["bun0"]))
    ce.setInputTarget(xyz1(bunny["bun4"]))
    q, m, d = ce.determineReciprocalCorrespondences()
    gold = np.asarray(golden["correspondences_reciprocal"], np.int32)
    assert np.array_equal(q, gold[:, 0]) and np.array_equal(m, gold[:, 1])


def test_rejector_chain_and_reciprocal_vs_oracle_50k(gpu, orc):
    import pcl_amd
    from oracle import rejectors as rej
    tgt, src, _ = pcl_amd.synth.icp_pair(50_000)
    chain_gpu = [pcl_amd.CorrespondenceRejectorMedianDistance(), pcl_amd.CorrespondenceRejectorOneToOne(),
                 pcl_amd.CorrespondenceRejectorTrimmed()]
    chain_gpu[0].setMedianFactor(2.0)
    chain_gpu[2].setOverlapRatio(0.8)
    for reciprocal in (False, True):
        ce = pcl_amd.CorrespondenceEstimation(gpu)
        ce.setInputSource(src)
        ce.setInputTarget(tgt)
        q, m, d = ce.determineCorrespondences(0.1, rejectors=chain_gpu, reciprocal=reciprocal)
        otree = orc.KdTree(tgt)
        if reciprocal:
            oq, om, od = otree.reciprocal_correspondences(orc.KdTree(src), src, tgt, 0.1)
        else:
            oq, om, od = otree.correspondences(src, 0.1)
        oq, om, od, _ = rej.reject_median_distance(oq, om, od, 2.0)
        oq, om, od = rej.reject_one_to_one(oq, om, od)
        oq, om, od = rej.reject_trimmed(oq, om, od, 0.8)
        assert np.array_equal(q, oq) and np.array_equal(m, om) and np.array_equal(d, od), reciprocal
        assert 0 < len(q) < 50_000


@pytest.mark.parametrize("n_same", [0, 1, 700, 3000])
def test_trimmed_and_median_on_tied_distances(gpu, orc, n_same):
    # correspondence_rejection_trimmed.cpp:53-58 orders by distance; equal distances (here: source points that ARE target
    # points, distance 0, and a lattice of equal offsets) are ordered by the query index -- the selection's tie passes
    import pcl_amd
    from oracle import rejectors as rej
    rng = np.random.default_rng(5 + n_same)
    tgt = np.ones((3000, 4), np.float32)
    tgt[:, :3] = rng.integers(0, 64, (3000, 3)).astype(np.float32)       # lattice: many equal squared distances
    src = tgt[rng.permutation(3000)].copy()
    src[n_same:, :3] += rng.choice(np.array([0.0, 0.25, 0.5], np.float32), (3000 - n_same, 3))
    for ratio in (0.1, 0.5, 0.9):
        for kind in ("trimmed", "median"):
            ce = pcl_amd.CorrespondenceEstimation(gpu)
            ce.setInputSource(src)
            ce.setInputTarget(tgt)
            if kind == "trimmed":
                r = pcl_amd.CorrespondenceRejectorTrimmed()
                r.setOverlapRatio(ratio)
            else:
                r = pcl_amd.CorrespondenceRejectorMedianDistance()
                r.setMedianFactor(2.0 * ratio)
            q, m, d = ce.determineCorrespondences(rejectors=[r])
            oq, om, od = orc.KdTree(tgt).correspondences(src)
            if kind == "trimmed":
                oq, om, od = rej.reject_trimmed(oq, om, od, ratio)
            else:
                oq, om, od, med = rej.reject_median_distance(oq, om, od, 2.0 * ratio)
                assert r.getMedianDistance() == med
            # Trimmed hands its list back ordered by distance; ties by query index on both sides
            assert np.array_equal(q, oq) and np.array_equal(m, om) and np.array_equal(d, od), (kind, ratio)


def test_icp_with_rejectors_vs_oracle(gpu, orc, bunny):
    # test/registration/test_registration.cpp:336-382 style: ICP + median + one-to-one rejectors
    import pcl_amd
    from oracle import rejectors as rej
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setMaximumIterations(30)
    icp.setMaxCorrespondenceDistance(0.05)
    icp.setTransformationEpsilon(1e-8)
    r1 = pcl_amd.CorrespondenceRejectorMedianDistance()
    r1.setMedianFactor(4.0)
    icp.addCorrespondenceRejector(r1)
    icp.addCorrespondenceRejector(pcl_amd.CorrespondenceRejectorOneToOne())
    icp.align()
    ref = rej.icp_with_filters(orc, tgt, src, 0,
                               rejectors=[lambda q, m, d: rej.reject_median_distance(q, m, d, 4.0),
                                          rej.reject_one_to_one],
                               max_iterations=30, max_correspondence_distance=0.05, transformation_epsilon=1e-8)
    assert icp.nr_iterations_ == ref["iterations"]
    assert np.linalg.norm(icp.getFinalTransformation().astype(np.float64) - ref["T"]) < 1e-5
    # reciprocal ICP
    icp2 = pcl_amd.IterativeClosestPoint(gpu)
    icp2.setInputTarget(tgt)
    icp2.setInputSource(src)
    icp2.setMaximumIterations(30)
    icp2.setMaxCorrespondenceDistance(0.05)
    icp2.setTransformationEpsilon(1e-8)
    icp2.setUseReciprocalCorrespondences(True)
    icp2.align()
    ref2 = rej.icp_with_filters(orc, tgt, src, 0, reciprocal=True, max_iterations=30,
                                max_correspondence_distance=0.05, transformation_epsilon=1e-8)
    assert icp2.nr_iterations_ == ref2["iterations"]
    assert np.linalg.norm(icp2.getFinalTransformation().astype(np.float64) - ref2["T"]) < 1e-5


# ------------------------------------------------------------------------------------------------
# radiusSearch
# ------------------------------------------------------------------------------------------------
def test_radius_search_sac_plane_golden(gpu):
    # test/kdtree/test_kdtree.cpp:292-330 + kdtree_unit_test_results.xml: 3283 exact neighbour lists
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "sac_plane_radius.npz"))
    cloud = z["cloud"]
    off, idx, d2 = build_tree(gpu, cloud).radiusSearch(cloud, float(z["radius"]))
    assert np.array_equal(off.astype(np.int64), z["offsets"])
    assert np.array_equal(idx, z["indices"])
    assert np.all(d2 < np.float32(0.02 * 0.02))


def test_radius_search_vs_bruteforce(gpu):
    from oracle import rejectors as rej
    rng = np.random.default_rng(31)
    pts = rng.uniform(0, 1, (4000, 3)).astype(np.float32)
    pts[50:60] = pts[40:50]        # duplicates -> ties
    pts[7] = np.nan
    qry = rng.uniform(-0.05, 1.05, (500, 3)).astype(np.float32)
    qry[3] = np.nan
    tree = build_tree(gpu, pts)
    for radius, max_nn in ((0.05, 0), (0.12, 0), (0.12, 7), (1e-4, 0), (3.0, 25)):
        off, idx, d2 = tree.radiusSearch(qry, radius, max_nn)
        ooff, oidx, od2 = rej.radius_search_bruteforce(pts, qry, radius, max_nn)
        assert np.array_equal(off, ooff), (radius, max_nn)
        assert np.array_equal(idx, oidx), (radius, max_nn)
        assert np.array_equal(d2, od2), (radius, max_nn)
    off, idx, d2 = tree.radiusSearch(np.zeros((0, 3), np.float32), 0.1)
    assert len(off) == 1 and len(idx) == 0


@pytest.mark.parametrize("nq", [1, 40, 700])
def test_radius_search_few_queries_against_a_large_index(gpu, nq):
    # the sparse layout of a batch (fewer queries per wavefront, api.hip: sparse_layout) in the radius search: the padding
    # slots count into a dump slot and fill nothing -- same CSR lists as the brute force, with a non-finite query and max_nn
    from oracle import rejectors as rej
    import pcl_amd
    rng = np.random.default_rng(100 + nq)
    tgt, _, _ = pcl_amd.synth.icp_pair(60_000)
    pts = np.ascontiguousarray(tgt[:, :3])
    qry = (pts[rng.integers(0, len(pts), nq)] + rng.normal(scale=0.005, size=(nq, 3))).astype(np.float32)
    if nq >= 40:
        qry[11] = np.nan
    tree = build_tree(gpu, pts)
    for radius, max_nn in ((0.02, 0), (0.05, 9)):
        off, idx, d2 = tree.radiusSearch(qry, radius, max_nn)
        ooff, oidx, od2 = rej.radius_search_bruteforce(pts, qry, radius, max_nn)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and np.array_equal(d2, od2), (nq, radius, max_nn)


# ------------------------------------------------------------------------------------------------
# Registration::getFitnessScore
# ------------------------------------------------------------------------------------------------
def test_fitness_score_known_answer(gpu):
    # test/registration/test_registration.cpp:198-229: (0 + 0 + 0 + 0.25) / 4 = 0.0625
    import pcl_amd
    src = np.asarray([(0, 0, 0), (0, 1, 0), (0, 0, 1), (10, 0, 0)], np.float32)
    tgt = np.asarray([(0, 0, 0), (0, 1, 0), (0, 0, 1), (10, 0, 0.5)], np.float32)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(xyz1(tgt))
    icp.setInputSource(xyz1(src))
    assert icp.getFitnessScore(1.0, transform=np.eye(4)) == pytest.approx(0.0625, abs=1e-4)
    assert icp.fitness_points == 4
    # max_range is compared with the SQUARED distance (impl/registration.hpp:157): 0.25 > 0.2 drops point 3
    assert icp.getFitnessScore(0.2, transform=np.eye(4)) == 0.0
    assert icp.fitness_points == 3
    assert icp.getFitnessScore(-1.0, transform=np.eye(4)) == np.finfo(np.float64).max


def test_fitness_score_icp_translated(gpu, bunny):
    # test/registration/test_registration.cpp:161-195
    import pcl_amd
    src = xyz1(bunny["bun0"])
    tgt = src.copy()
    tgt[:, 2] += np.float32(0.2)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.setMaximumIterations(50)
    icp.align()
    assert icp.hasConverged()
    assert icp.getFitnessScore() < 1e-6
    T = icp.getFinalTransformation()
    assert np.allclose(np.diag(T)[:3], 1.0, atol=2e-3)
    assert np.allclose(T[:3, 3], (0.0, 0.0, 0.2), atol=2e-3)


def test_fitness_score_vs_oracle(gpu, orc):
    import pcl_amd
    from pcl_amd import synth
    tgt = synth.gaussian_surface(60_000, synth.TARGET_SEED)
    src = synth.gaussian_surface(50_000, synth.SOURCE_SEED)
    src[7, 0] = np.nan  # skipped (impl/registration.hpp:151-152)
    T = synth.ground_truth_transform().astype(np.float32)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    tree = build_tree(gpu, tgt)
    icp.setSearchMethodTarget(tree)
    icp.setInputSource(src)
    otree = orc.KdTree(tgt)
    for max_range in (np.finfo(np.float64).max, 2e-4, 1e-5):
        want, nr = otree.fitness_score(src, T, max_range)
        got = icp.getFitnessScore(max_range, transform=T)
        assert icp.fitness_points == nr
        assert got == pytest.approx(want, rel=1e-12)  # fp64 sums, different summation order
    # the score does not disturb an alignment in progress
    icp.reset()
    s0 = icp.iterate(np.eye(4, dtype=np.float32), max_dist=0.1)
    icp.getFitnessScore(transform=T)
    q0 = icp.fetchCorrespondences()
    icp.reset()
    s1 = icp.iterate(np.eye(4, dtype=np.float32), max_dist=0.1)
    q1 = icp.fetchCorrespondences()
    assert np.array_equal(s0, s1) and all(np.array_equal(a, b) for a, b in zip(q0, q1))


# ------------------------------------------------------------------------------------------------
# transformation estimators on explicit pairs + the symmetric objective
# ------------------------------------------------------------------------------------------------
def _quadric_with_normals():
    # the test surface of test/registration/test_registration_api.cpp:469-518 and :663-712
    xs = np.arange(-5.0, 5.0001, 0.5, dtype=np.float32)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    x, y = X.ravel(), Y.ravel()
    z = np.float32(0.1) * x ** 2 + np.float32(0.2) * x * y - np.float32(0.3) * y + np.float32(1.0)
    n = np.stack([-0.2 * x - 0.2, 0.6 * y - 0.2, np.ones_like(x)], 1).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.stack([x, y, z, np.ones_like(x)], 1).astype(np.float32), n


def test_estimators_known_answers_and_oracle(gpu, orc, golden):
    # test/registration/test_registration_api.cpp:383-424 (SVD), :469-518 (LLS), :663-712 (symmetric LLS)
    import pcl_amd
    src, sn = _quadric_with_normals()
    G = np.asarray(golden["lls_ground_truth"], np.float32)
    tgt, tn = orc.transform_cloud(G, src, order=1, normals=sn)
    # point-to-plane LLS
    T, sums = pcl_amd.estimateRigidTransformation(gpu, pcl_amd.POINT_TO_PLANE, src, tgt, tgt_normals=tn)
    To, so, used = orc.lls_point_to_plane(src, tgt, tn)
    assert np.abs(T - G).max() < golden["lls_tol"]
    assert sums[28] == used == 441
    assert np.allclose(sums[:27], so, rtol=1e-11, atol=1e-13)   # fp64 sums, different summation order
    assert np.abs(T - To).max() < 1e-6
    # symmetric LLS (tolerance of the reference test: 1e-2)
    for flip, enforce in ((1.0, True), (-1.0, True)):
        T, sums = pcl_amd.estimateRigidTransformation(gpu, pcl_amd.SYMMETRIC, src, tgt, src_normals=sn,
                                                      tgt_normals=np.float32(flip) * tn,
                                                      enforce_same_direction_normals=enforce)
        To, so, used = orc.lls_symmetric(src, sn, tgt, np.float32(flip) * tn, enforce_same_direction=enforce)
        assert np.abs(T - G).max() < 1e-2
        assert sums[28] == used
        assert np.allclose(sums[:27], so, rtol=1e-11, atol=1e-13)
        assert np.abs(T - To).max() < 1e-6
    # SVD / umeyama: exact recovery of a rigid motion to 2e-6 (the reference tests 1e-6 on quaternion + t)
    T, sums = pcl_amd.estimateRigidTransformation(gpu, pcl_amd.POINT_TO_POINT, src, tgt)
    assert np.abs(T - orc.umeyama(src, tgt, acc_double=True)).max() < 2e-6
    # size mismatch is refused like the reference (transformation_estimation_svd.hpp:53-60)
    with pytest.raises(AssertionError):
        pcl_amd.estimateRigidTransformation(gpu, pcl_amd.POINT_TO_POINT, src, tgt[:-1])


def test_icp_symmetric_objective_vs_oracle(gpu, orc, bunny):
    # test/registration/test_registration.cpp:305-318 (setUseSymmetricObjective) on the bunny pair
    import pcl_amd
    from oracle import rejectors as rej
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    # normals of both clouds from the oracle so that both sides start from identical inputs
    tn, _ = orc.KdTree(tgt).normals(tgt, 15, viewpoint=(0, 0, 10))
    sn, _ = orc.KdTree(src).normals(src, 15, viewpoint=(0, 0, 10))
    tn = np.ascontiguousarray(tn[:, :3], np.float32)
    sn = np.ascontiguousarray(sn[:, :3], np.float32)
    for enforce in (True, False):
        icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
        icp.setInputTarget(tgt)
        icp.setTargetNormals(tn)
        icp.setInputSource(src)
        icp.setSourceNormals(sn)
        icp.setUseSymmetricObjective(True)
        assert icp.getUseSymmetricObjective()
        icp.setEnforceSameDirectionNormals(enforce)
        icp.setMaximumIterations(30)
        icp.setMaxCorrespondenceDistance(0.05)
        icp.setTransformationEpsilon(1e-8)
        icp.align()
        ref = rej.icp_with_filters(orc, tgt, src, 2, tgt_normals=tn, src_normals=sn, enforce_same_direction=enforce,
                                   max_iterations=30, max_correspondence_distance=0.05, transformation_epsilon=1e-8)
        assert icp.nr_iterations_ == ref["iterations"]
        assert np.linalg.norm(icp.getFinalTransformation().astype(np.float64) - ref["T"]) < 1e-5
        assert icp.hasConverged() == ref["converged"]
    # without source normals the symmetric objective is refused
    icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
    icp.setInputTarget(tgt)
    icp.setTargetNormals(tn)
    icp.setInputSource(src)
    icp.setUseSymmetricObjective(True)
    with pytest.raises(pcl_amd.PclHipError):
        icp.align()


# ------------------------------------------------------------------------------------------------
# NormalEstimation with setRadiusSearch
# ------------------------------------------------------------------------------------------------
def test_normals_radius_vs_oracle(gpu, orc, bunny):
    import pcl_amd
    from oracle import rejectors as rej
    cloud = xyz1(bunny["bun0"]).copy()
    cloud[11, 1] = np.nan                 # a dropped point: NaN normal, not a neighbour of anyone
    for radius in (0.01, 0.03):
        ne = pcl_amd.NormalEstimation(gpu)
        ne.setInputCloud(cloud)
        ne.setRadiusSearch(radius)
        ne.setViewPoint(0, 0, 10)
        got = ne.compute()
        want, nan = rej.normals_radius(orc, cloud, radius, viewpoint=(0, 0, 10))
        assert ne.nan_count == nan
        bad = np.isnan(want[:, 0])
        assert np.array_equal(np.isnan(got[:, 0]), bad)
        # same tolerance as the k-NN mode: device atan2f/cosf/sinf vs libm in the closed-form eigen solve
        dots = np.abs(np.sum(got[~bad, :3] * want[~bad, :3], axis=1))
        assert dots.min() >= 1 - 1e-5
        assert np.sign(np.sum(got[~bad, :3] * want[~bad, :3], axis=1)).min() > 0   # same orientation
        assert np.abs(got[~bad, 3] - want[~bad, 3]).max() < 1e-5
    # radius-mode normals feed point-to-plane ICP like the k-NN ones
    icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
    icp.setSearchMethodTarget(ne.tree)
    icp.setInputSource(xyz1(bunny["bun4"]))
    icp.setMaximumIterations(5)
    icp.align()
    assert icp.hasConverged()
    # both k and radius set: refused like Feature::initCompute (impl/feature.hpp:131-140)
    ne.setKSearch(5)
    with pytest.raises(ValueError):
        ne.compute()


def test_normals_radius_chunked_large(gpu, orc):
    # 300k-point surface, radius with ~50 neighbours: exercises the chunked key buffers; checked against the
    # k-NN path on the points whose radius neighbourhood is exactly their 8 nearest neighbours
    import pcl_amd
    from pcl_amd import synth
    cloud = synth.gaussian_surface(300_000, synth.TARGET_SEED)
    tree = build_tree(gpu, cloud)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(cloud)
    ne.setSearchMethod(tree)
    ne.setRadiusSearch(0.015)
    ne.setViewPoint(0, 0, 10)
    nr = ne.compute()
    assert np.isfinite(nr).all() and ne.nan_count == 0
    assert np.abs(np.linalg.norm(nr[:, :3], axis=1) - 1).max() < 1e-5
    # the surface is smooth: radius normals agree with the analytic normal direction within a few degrees
    ne2 = pcl_amd.NormalEstimation(gpu)
    ne2.setInputCloud(cloud)
    ne2.setSearchMethod(tree)
    ne2.setKSearch(30)
    ne2.setViewPoint(0, 0, 10)
    nk = ne2.compute()
    assert np.abs(np.sum(nr[:, :3] * nk[:, :3], axis=1)).mean() > 0.999
    # spot check against the oracle on a subset: neighbours by brute force on a 4000-point window
    sub = np.argsort(cloud[:, 0] + 10 * cloud[:, 1])[:1]  # deterministic seed point
    off, idx, d2 = tree.radiusSearch(cloud[sub], 0.015)
    cov, cen, cnt = orc.mean_and_covariance(cloud, idx[int(off[0]):int(off[1])])
    nx, ny, nz, curv = orc.solve_plane_parameters(cov)
    assert abs(abs(nx * nr[sub[0], 0] + ny * nr[sub[0], 1] + nz * nr[sub[0], 2]) - 1) < 1e-5
    assert abs(curv - nr[sub[0], 3]) < 1e-5


def test_weighted_point_to_plane_lls_vs_oracle(gpu, orc, golden):
    # TransformationEstimationPointToPlaneLLSWeighted (impl/transformation_estimation_point_to_plane_lls_weighted.hpp
    # :195-290): the LLS system with the target normal scaled by the pair's weight (float product, :227-229)
    import pcl_amd
    src, sn = _quadric_with_normals()
    G = np.asarray(golden["lls_ground_truth"], np.float32)
    tgt, tn = orc.transform_cloud(G, src, order=1, normals=sn)
    rng = np.random.default_rng(3)
    w = rng.uniform(0.1, 2.0, len(src)).astype(np.float32)
    T, sums = pcl_amd.estimateRigidTransformation(gpu, pcl_amd.POINT_TO_PLANE, src, tgt, tgt_normals=tn, weights=w)
    To, so, used = orc.lls_point_to_plane(src, tgt, (tn * w[:, None]).astype(np.float32))
    assert used == sums[28] == 441
    assert np.allclose(sums[:27], so, rtol=1e-11, atol=1e-13)
    assert np.abs(T - To).max() < 1e-6
    assert np.abs(T - G).max() < golden["lls_tol"]      # exact pairs: any positive weights recover the motion
    # unit weights are the unweighted estimator, bit for bit
    T1, s1 = pcl_amd.estimateRigidTransformation(gpu, pcl_amd.POINT_TO_PLANE, src, tgt, tgt_normals=tn,
                                                 weights=np.ones(len(src), np.float32))
    T0, s0 = pcl_amd.estimateRigidTransformation(gpu, pcl_amd.POINT_TO_PLANE, src, tgt, tgt_normals=tn)
    assert np.array_equal(s1, s0) and np.array_equal(T1, T0)


# ------------------------------------------------------------------------------------------------
# GICP covariances
# ------------------------------------------------------------------------------------------------
def test_gicp_covariances_vs_oracle(gpu, orc, bunny):
    # GeneralizedIterativeClosestPoint::computeCovariances, impl/gicp.hpp:70-147
    import pcl_amd
    from pcl_amd import synth
    for cloud, k in ((xyz1(bunny["bun0"]), 20), (synth.gaussian_surface(50_000, synth.TARGET_SEED), 20),
                     (synth.gaussian_surface(20_000, synth.SOURCE_SEED), 7)):
        cloud = cloud.copy()
        cloud[3, 2] = np.nan     # dropped from the index: NaN matrix
        tree = build_tree(gpu, cloud)
        got = tree.gicpCovariances(k, 0.001)
        want = orc.KdTree(cloud).gicp_covariances(cloud, k, 0.001)
        assert np.isnan(got[3]).all() and np.isnan(want[3]).all()
        ok = np.ones(len(cloud), bool)
        ok[3] = False
        # the matrix is I - (1 - eps) n n^T: both sides iterate a double Jacobi solve; the smallest direction of
        # a 20-point neighbourhood is well separated on these surfaces
        assert np.abs(got[ok] - want[ok]).max() < 1e-9
        w = np.linalg.eigvalsh(got[ok])
        assert np.allclose(w, [0.001, 1.0, 1.0], atol=1e-12)
    with pytest.raises(pcl_amd.PclHipError):
        build_tree(gpu, xyz1(bunny["bun0"])[:10]).gicpCovariances(20)
    with pytest.raises(pcl_amd.PclHipError):
        tree.gicpCovariances(33)


# ------------------------------------------------------------------------------------------------
# ties under seeding, and size-independent properties at the benchmark size
# ------------------------------------------------------------------------------------------------
def test_icp_lattice_ties_with_seeds_bit_exact(gpu, orc):
    # lattice target, source points exactly half-way between lattice points: every query has 2 or 4
    # equidistant targets; translations by exact binary fractions keep producing ties in later (seeded)
    # iterations.  Every iteration must pick the lowest index, like the oracle.
    import pcl_amd
    g = np.arange(48, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    tgt = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size, np.float32), np.ones(X.size, np.float32)], 1)
    rng = np.random.default_rng(2)
    perm = rng.permutation(len(tgt))          # original index order unrelated to position
    tgt = np.ascontiguousarray(tgt[perm])
    src = tgt.copy()
    src[:, 0] += np.float32(0.5)              # ties between (x, y) and (x+1, y)
    otree = orc.KdTree(tgt)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.reset()
    cur = src.copy()
    steps = [np.eye(4, dtype=np.float32)]
    for dx, dy in ((0.0, 0.5), (0.25, 0.0), (0.25, -0.5), (-1.0, 0.0), (0.0, 0.0), (0.5, 0.5)):
        T = np.eye(4, dtype=np.float32)
        T[0, 3], T[1, 3] = dx, dy
        steps.append(T)
    for it, T in enumerate(steps):
        icp.iterate(T, max_dist=10.0)
        q, m, d = icp.fetchCorrespondences()
        cur = orc.transform_cloud(T, cur, order=0)
        oq, om, od = otree.correspondences(cur, 10.0)
        bi, bd = orc.knn_bruteforce(tgt, cur, 1)      # the lowest-index rule, by brute force
        assert np.array_equal(om, bi[:, 0]), it
        assert np.array_equal(q, oq) and np.array_equal(m, om) and np.array_equal(d, od), it


# ------------------------------------------------------------------------------------------------
# mirrors of the reference's own end-to-end registration tests (property checks, no oracle)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
def test_reference_run_icp_with_normals(gpu, bunny, symmetric):
    # test/registration/test_registration.cpp:272-318 (runICPWithNormals, both objectives)
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    normals = {}
    for name, cloud in (("src", src), ("tgt", tgt)):
        ne = pcl_amd.NormalEstimation(gpu)
        ne.setInputCloud(cloud)
        ne.setKSearch(10)
        normals[name] = np.ascontiguousarray(ne.compute()[:, :3])
        assert ne.nan_count == 0
    reg = pcl_amd.IterativeClosestPointWithNormals(gpu)
    reg.setInputSource(src)
    reg.setSourceNormals(normals["src"])
    reg.setInputTarget(tgt)
    reg.setTargetNormals(normals["tgt"])
    reg.setUseSymmetricObjective(symmetric)
    reg.setMaximumIterations(50)
    reg.setTransformationEpsilon(1e-8)
    reg.setMaxCorrespondenceDistance(0.05)
    out = reg.align(want_output=True)
    assert len(out) == len(src)
    assert reg.hasConverged()
    assert reg.getFitnessScore() < 0.001


def _random_transform(rng, max_angle, max_trans):
    # sampleRandomTransform, test/registration/test_registration.cpp:321-333
    axis = rng.uniform(0, 1, 3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0, 1) * max_angle
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.uniform(0, 1, 3) * max_trans
    return T


def test_reference_icp_with_rejectors_random_global_transforms(gpu, bunny):
    # test/registration/test_registration.cpp:336-382 (median-distance rejector; the SaC rejector of that test is
    # outside the path): a fixed offset between the pair under random global poses is recovered to 1 cm / 0.1
    import pcl_amd
    from pcl_amd import synth
    rng = np.random.default_rng(0)
    source = xyz1(bunny["bun0"])
    for t in range(10):
        delta = _random_transform(rng, 0.0, 0.05)
        net = _random_transform(rng, 2 * np.pi, 10.0)
        src = synth.apply_rigid(np.linalg.inv(delta) @ net, source)
        tgt = synth.apply_rigid(net, source)
        reg = pcl_amd.IterativeClosestPoint(gpu)
        reg.setMaximumIterations(50)
        reg.setTransformationEpsilon(1e-8)
        reg.setMaxCorrespondenceDistance(0.15)
        rej = pcl_amd.CorrespondenceRejectorMedianDistance()
        rej.setMedianFactor(4.0)
        reg.addCorrespondenceRejector(rej)
        reg.setInputSource(src)
        reg.setInputTarget(tgt)
        reg.align()
        T = reg.getFinalTransformation()
        # src = delta^-1 (net p), tgt = net p  =>  the registration is delta itself (:372-379)
        assert np.abs(T[:3, 3] - delta[:3, 3]).max() < 1e-2, t        # "translation should be within 1cm"
        assert np.abs(T[:3, :3] - delta[:3, :3]).max() < 1e-1, t      # "rotation within .1"
        assert reg.hasConverged(), t


def test_reference_correspondences_with_cached_search_tree(gpu):
    # test/registration/test_correspondence_estimation.cpp:138-176: a search tree handed over with
    # force_no_recompute gives the same correspondences as the estimator's own tree
    import pcl_amd
    rng = np.random.default_rng(11)
    cloud1 = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    cloud2 = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputSource(cloud1)
    ce.setInputTarget(cloud2)
    q0, m0, d0 = ce.determineCorrespondences()
    tree2 = build_tree(gpu, cloud2)
    ce.setSearchMethodTarget(tree2, True)
    q1, m1, d1 = ce.determineCorrespondences()
    assert len(q0) == 50 and np.array_equal(q0, q1) and np.array_equal(m0, m1) and np.array_equal(d0, d1)
    # the same tree object serves several consumers (ICP + normals + another estimator) without a rebuild
    h = tree2.h.value
    ce2 = pcl_amd.CorrespondenceEstimation(gpu)
    ce2.setSearchMethodTarget(tree2, True)
    ce2.setInputSource(cloud1)
    q2, m2, d2 = ce2.determineCorrespondences()
    assert tree2.h.value == h and np.array_equal(m2, m0)


# ------------------------------------------------------------------------------------------------
# unseeded searches from a stand-off (the disc bounds of traverse.hpp), away from the unit cube
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,scale,standoff", [
    ((0.0, 0.0, 0.0), 1.0, 0.03),            # the bench geometry, a larger stand-off
    ((1000.0, -2000.0, 500.0), 1.0, 0.02),   # far from the origin: 6e-5 float spacing against 1e-3 point spacing
    ((0.0, 0.0, 0.0), 250.0, 4.0),           # metres-sized scene
    ((-3.0, 7.0, 1.0), 0.004, 1e-4),         # millimetre-sized scene
    ((0.0, 0.0, 0.0), 1.0, 0.3),             # stand-off of the size of the whole surface's relief
])
def test_cold_standoff_correspondences_bit_exact(gpu, orc, offset, scale, standoff):
    # first iteration of a registration (no seeds): every match and squared distance equals the oracle's k = 1 search
    import pcl_amd
    n = 150_000
    off = np.asarray(offset, np.float64)
    tgt = pcl_amd.synth.gaussian_surface(n, pcl_amd.synth.TARGET_SEED).astype(np.float64)
    src = pcl_amd.synth.gaussian_surface(n // 2, pcl_amd.synth.SOURCE_SEED).astype(np.float64)
    th = np.deg2rad(1.5)
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    src[:, :3] = src[:, :3] @ R.T + np.array([0.004, -0.007, 1.0]) * np.array([1, 1, standoff / scale])
    tgt_f = xyz1((tgt[:, :3] * scale + off).astype(np.float32))
    src_f = xyz1((src[:, :3] * scale + off).astype(np.float32))
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt_f)
    icp.setInputSource(src_f)
    icp.reset()
    icp.iterate(np.eye(4, dtype=np.float32), max_dist=1e6 * scale)
    q, m, d = icp.fetchCorrespondences()
    oi, od = orc.KdTree(tgt_f).knn(src_f, 1)
    assert np.array_equal(q, np.arange(len(src_f)))
    assert np.array_equal(m, oi[:, 0])
    assert np.array_equal(d, od[:, 0])


# ------------------------------------------------------------------------------------------------
# NormalEstimation with a search surface other than the input, and over an index subset
# (Feature::setSearchSurface / PCLBase::setIndices as NormalEstimation::computeFeature uses them)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 15, 40])
def test_normals_search_surface_vs_oracle(gpu, orc, k):
    import pcl_amd
    surface = pcl_amd.synth.gaussian_surface(120_000, pcl_amd.synth.TARGET_SEED)
    queries = pcl_amd.synth.gaussian_surface(15_000, pcl_amd.synth.SOURCE_SEED).copy()
    queries[:, 2] += np.float32(0.002)        # the queries are not surface points
    queries[33, 0] = np.inf                   # a non-finite query: NaN row (normal_3d.hpp:60-66)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(queries)
    ne.setSearchSurface(surface)
    ne.setKSearch(k)
    ne.setViewPoint(0.3, -0.2, 5)
    got = ne.compute()
    otree = orc.KdTree(surface)
    want, nan = otree.normals_at(surface, queries, k, viewpoint=(0.3, -0.2, 5))
    assert got.shape == (len(queries), 4) and ne.nan_count == nan == 1 and np.all(np.isnan(got[33]))
    ok = ~np.isnan(want[:, 0])
    dots = np.sum(got[ok, :3] * want[ok, :3], axis=1)   # same tolerances as test_normals_vs_oracle
    assert dots.min() > 1 - 1e-5, dots.min()
    assert np.abs(got[ok, 3] - want[ok, 3]).max() < 1e-5
    # an index subset of the input (with a repeated index): row j belongs to queries[indices[j]]
    ind = np.concatenate([np.arange(0, len(queries), 7), [5, 5]]).astype(np.int32)
    ne.setIndices(ind)
    sub = ne.compute()
    assert sub.shape == (len(ind), 4)
    assert np.array_equal(sub, got[ind], equal_nan=True)
    want_sub, _ = otree.normals_at(surface, queries, k, viewpoint=(0.3, -0.2, 5), indices=ind)
    assert np.array_equal(np.isnan(sub[:, 0]), np.isnan(want_sub[:, 0]))
    # an index subset with the input as its own surface equals the rows of the all-points run
    ne2 = pcl_amd.NormalEstimation(gpu)
    ne2.setInputCloud(surface)
    ne2.setKSearch(k)
    ne2.setViewPoint(0.3, -0.2, 5)
    full = ne2.compute()
    pick = np.arange(3, len(surface), 1001).astype(np.int32)
    ne2.setIndices(pick)
    part = ne2.compute()
    assert np.array_equal(part, full[pick], equal_nan=True)
    with pytest.raises(pcl_amd.PclHipError):     # an index outside the input cloud is refused, not read
        ne2.setIndices(np.array([0, len(surface)], np.int32))
        ne2.compute()


def test_normals_search_surface_radius_vs_oracle(gpu, orc, bunny):
    import pcl_amd
    from oracle import rejectors as rej
    surface = xyz1(bunny["bun0"])
    queries = xyz1(bunny["bun4"]).copy()
    queries[7, 2] = np.nan
    for radius in (0.01, 0.03):
        ne = pcl_amd.NormalEstimation(gpu)
        ne.setInputCloud(queries)
        ne.setSearchSurface(surface)
        ne.setRadiusSearch(radius)
        ne.setViewPoint(0, 0, 10)
        got = ne.compute()
        want, nan = rej.normals_radius_at(orc, surface, queries, radius, viewpoint=(0, 0, 10))
        assert ne.nan_count == nan
        bad = np.isnan(want[:, 0])
        assert np.array_equal(np.isnan(got[:, 0]), bad)
        dots = np.sum(got[~bad, :3] * want[~bad, :3], axis=1)
        assert dots.min() >= 1 - 1e-5
        assert np.abs(got[~bad, 3] - want[~bad, 3]).max() < 1e-5


def test_normals_radius_few_queries_on_a_large_surface(gpu, orc):
    # few queries against a large surface go through the sparse layout (fewer queries per wavefront): the padding slots'
    # NaN rows and their count are taken back -- rows and nan_count equal the oracle's, a non-finite query and a query
    # without neighbours among them
    import pcl_amd
    from oracle import rejectors as rej
    surface = pcl_amd.synth.gaussian_surface(60_000, pcl_amd.synth.TARGET_SEED)
    rng = np.random.default_rng(3)
    queries = surface[rng.integers(0, len(surface), 90)].copy()
    queries[:, :3] += rng.normal(scale=0.002, size=(90, 3)).astype(np.float32)
    queries[5, 1] = np.nan
    queries[6, 2] += np.float32(3.0)          # nothing within the radius
    for radius in (0.03, 0.06):
        ne = pcl_amd.NormalEstimation(gpu)
        ne.setInputCloud(queries)
        ne.setSearchSurface(surface)
        ne.setRadiusSearch(radius)
        ne.setViewPoint(0, 0, 10)
        got = ne.compute()
        want, nan = rej.normals_radius_at(orc, surface, queries, radius, viewpoint=(0, 0, 10))
        assert ne.nan_count == nan and nan >= 2
        bad = np.isnan(want[:, 0])
        assert np.array_equal(np.isnan(got[:, 0]), bad)
        dots = np.sum(got[~bad, :3] * want[~bad, :3], axis=1)
        assert dots.min() >= 1 - 1e-5
        assert np.abs(got[~bad, 3] - want[~bad, 3]).max() < 1e-5


@pytest.mark.parametrize("field,col,lo,hi", [("x", 0, -0.4, 0.25), ("z", 2, 0.02, 0.11), ("curvature", 8, 0.01, 0.03)])
@pytest.mark.parametrize("negative", [False, True])
def test_voxelgrid_filter_field_and_negative_limits(gpu, orc, field, col, lo, hi, negative):
    # the pass-through filter in front of the grid (voxel_grid.h:440-476, impl/voxel_grid.hpp:513-590,684-695): any
    # field of the point type, inside or outside the interval; centroids bit-exact against the oracle
    import pcl_amd
    n = 200_000
    cloud = np.zeros((n, 12), np.float32)
    cloud[:, :4] = pcl_amd.synth.gaussian_surface(n, pcl_amd.synth.TARGET_SEED)
    rng = np.random.default_rng(11)
    cloud[:, 4:7] = rng.normal(size=(n, 3)).astype(np.float32)
    cloud[:, 8] = rng.uniform(0, 0.05, n).astype(np.float32)
    cloud[::977, col] = np.nan if col > 2 else cloud[::977, col]   # a NaN field value passes both forms of the test
    vg = pcl_amd.VoxelGrid(gpu)
    vg.setInputCloud(cloud)
    vg.setLeafSize(0.01)
    vg.setFilterFieldName(field)
    vg.setFilterLimits(lo, hi)
    vg.setFilterLimitsNegative(negative)
    assert vg.getFilterFieldName() == field and vg.getFilterLimits() == (lo, hi) and vg.getFilterLimitsNegative() == negative
    out = vg.filter()
    want, _ = orc.voxelgrid(cloud, 0.01, limits=(lo, hi), field=col, negative=negative)
    assert len(want) > 1000 and np.array_equal(out[:, :4], want)
    if col <= 2 and not negative:   # every centroid lies inside the interval of its filter coordinate
        assert out[:, col].min() >= np.float32(lo) and out[:, col].max() <= np.float32(hi)
    # a field the point type does not have is refused (the reference logs "could not find field" and stops)
    vg4 = pcl_amd.VoxelGrid(gpu)
    vg4.setInputCloud(np.ascontiguousarray(cloud[:, :4]))
    vg4.setLeafSize(0.01)
    vg4.setFilterFieldName("curvature")
    with pytest.raises(ValueError):
        vg4.filter()
    # limits without a field name do nothing (voxel_grid.hpp:612-616: the filter is keyed on the name)
    vg5 = pcl_amd.VoxelGrid(gpu)
    vg5.setInputCloud(np.ascontiguousarray(cloud[:, :4]))
    vg5.setLeafSize(0.01)
    vg5.setFilterLimits(lo, hi)
    assert np.array_equal(vg5.filter(), orc.voxelgrid(cloud[:, :4], 0.01)[0])


def test_registration_options_through_the_criteria_object(gpu, bunny):
    # icp.getConvergeCriteria()->setFailureAfterMaximumIterations(true) (icp.h:180-184,
    # default_convergence_criteria.hpp:65-71): hitting the iteration limit is then a failure, not a convergence
    import pcl_amd
    def run(fail):
        icp = pcl_amd.IterativeClosestPoint(gpu)
        icp.setInputSource(xyz1(bunny["bun0"]))
        icp.setInputTarget(xyz1(bunny["bun4"]))
        icp.setMaximumIterations(3)
        cc = icp.getConvergeCriteria()
        cc.setFailureAfterMaximumIterations(fail)
        assert cc.getFailureAfterMaximumIterations() == fail and cc.getMaximumIterations() == 3
        assert cc.getRotationThreshold() == 0.99999 and cc.getAbsoluteMSE() == 1e-12
        icp.align()
        return icp
    a, b = run(False), run(True)
    assert a.hasConverged() and a.getConvergenceState() == "ITERATIONS"
    assert not b.hasConverged() and b.getConvergenceState() == "FAILURE_AFTER_MAX_ITERATIONS"
    assert b.getConvergeCriteria().getConvergenceState() == b.getConvergenceState()
    assert np.array_equal(a.getFinalTransformation(), b.getFinalTransformation())
    # stored-only options and list management of registration.h
    a.setRANSACIterations(7)
    a.setRANSACOutlierRejectionThreshold(0.2)
    assert a.getRANSACIterations() == 7 and a.getRANSACOutlierRejectionThreshold() == 0.2
    r1, r2 = pcl_amd.CorrespondenceRejectorDistance(), pcl_amd.CorrespondenceRejectorTrimmed()
    r1.setMaximumDistance(0.05)
    r2.setOverlapRatio(0.8)
    a.addCorrespondenceRejector(r1)
    a.addCorrespondenceRejector(r2)
    assert a.getCorrespondenceRejectors() == [r1, r2] and r1.getMaximumDistance() == 0.05 and r2.getOverlapRatio() == 0.8
    assert a.removeCorrespondenceRejector(0) and not a.removeCorrespondenceRejector(5)
    assert a.getCorrespondenceRejectors() == [r2]
    assert a.getMaximumIterations() == 3 and a.getClassName() == "IterativeClosestPoint"


# ------------------------------------------------------------------------------------------------
# the kd order itself (index_build.hip): what the start-level shortcut of the seeded searches relies on
# ------------------------------------------------------------------------------------------------
def _check_kd_cells(cloud, order):
    """Every aligned run of 16 * 2^k positions up to 256, and of 256 * 4^k above, is one cell of a kd partition: a run of
    at most 256 positions is cut in two along one axis (max of the first half <= min of the second), a larger one into four
    quarters separated, in order, along ONE axis (max of a quarter <= min of the next)."""
    n = len(order)
    assert sorted(order.tolist()) == sorted(set(order.tolist())) and len(order) == n
    pts = cloud[order, :3].astype(np.float64)
    n_pad = -(-n // 16) * 16
    run = 16
    # min / max of every 16-run (pads of the last leaf ignored)
    big = np.full((n_pad, 3), np.nan)
    big[:n] = pts
    lo = np.nanmin(big.reshape(-1, 16, 3), axis=1)
    hi = np.nanmax(big.reshape(-1, 16, 3), axis=1)

    def separated(lo_a, hi_a, lo_b, hi_b):  # some axis on which all of a lies at or below all of b
        return np.any(hi_a <= lo_b, axis=-1)
    level = 0
    while len(lo) > 1:
        fan = 2 if level < 4 else 4            # 16 -> 32 -> 64 -> 128 -> 256 by binary cuts, then four slabs per round
        m = len(lo) // fan * fan
        if m == 0:
            break
        L, H = lo[:m].reshape(-1, fan, 3), hi[:m].reshape(-1, fan, 3)
        ok = np.ones(len(L), bool)
        if fan == 2:
            ok &= separated(L[:, 0], H[:, 0], L[:, 1], H[:, 1])
        else:                                   # the same axis for the three cuts of a round
            ax_ok = np.ones((len(L), 3), bool)
            for j in range(3):
                ax_ok &= H[:, j] <= L[:, j + 1]
            ok &= np.any(ax_ok, axis=1)
        assert ok.all(), ("kd cells overlap at runs of %d positions" % (run * fan), int((~ok).sum()), len(ok))
        # the tail (an incomplete group of runs) is merged as it is
        tail_lo = [np.nanmin(lo[m:], axis=0)] if m < len(lo) else []
        tail_hi = [np.nanmax(hi[m:], axis=0)] if m < len(hi) else []
        lo = np.concatenate([np.nanmin(L, axis=1)] + ([np.asarray(tail_lo)] if tail_lo else []))
        hi = np.concatenate([np.nanmax(H, axis=1)] + ([np.asarray(tail_hi)] if tail_hi else []))
        run *= fan
        level += 1


@pytest.mark.parametrize("kind,n", [("surface", 70_001), ("surface", 300_000), ("uniform", 20_000), ("lattice", 30_000),
                                    ("tiny", 37), ("plane", 50_000),
                                    # the one-workgroup rounds with every top level and partly filled blocks
                                    ("uniform", 200), ("lattice", 700), ("uniform", 3000), ("lattice", 4096), ("uniform", 4097),
                                    ("lattice", 5000), ("surface", 16_385), ("lattice", 66_000)])
def test_kd_order_cells_are_a_kd_partition(gpu, kind, n):
    from pcl_amd import synth
    rng = np.random.default_rng(n)
    if kind == "surface":
        cloud = synth.gaussian_surface(n, synth.TARGET_SEED)
    elif kind == "uniform":
        cloud = np.ones((n, 4), np.float32)
        cloud[:, :3] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    elif kind == "lattice":                     # heavy ties at every cut
        cloud = np.ones((n, 4), np.float32)
        cloud[:, :3] = rng.integers(0, 12, (n, 3)).astype(np.float32)
    elif kind == "plane":                       # one axis without extent
        cloud = np.ones((n, 4), np.float32)
        cloud[:, :2] = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        cloud[:, 2] = 0.5
    else:
        cloud = np.ones((n, 4), np.float32)
        cloud[:, :3] = rng.normal(size=(n, 3)).astype(np.float32)
    tree = build_tree(gpu, cloud)
    order = tree.order()
    assert len(order) == n
    _check_kd_cells(cloud, order)


def test_kd_cells_of_64_points_are_patches_not_strips(gpu):
    # what a wavefront of queries pays for is the neighbourhood of its 64 points: the block kernel of the index build cuts
    # a 256-point cell in two, twice, so that a 64-point cell of a surface is an 8 x 8 patch of point spacings; four slabs
    # along one axis (the schedule until the end of round 4) made it a 16 x 4 strip and every search launch 6-18 % slower
    # (profiles/r04_seed_experiments_ab.txt).  Exactness does not depend on this; the headline does.
    rng = np.random.default_rng(64)
    for n in (50_000, 200_000):                 # both parities of the number of four-way rounds above the block kernel
        cloud = np.ones((n, 4), np.float32)
        cloud[:, :2] = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        cloud[:, 2] = 0.5
        order = build_tree(gpu, cloud).order()
        pts = cloud[order, :2].astype(np.float64)
        for run, limit in ((64, 2.0), (16, 2.0)):
            m = n // run * run
            cells = pts[:m].reshape(-1, run, 2)
            ext = cells.max(axis=1) - cells.min(axis=1)
            aspect = ext.max(axis=1) / np.maximum(ext.min(axis=1), 1e-12)
            assert np.median(aspect) < limit, (n, run, float(np.median(aspect)))


def test_context_options(gpu):
    # pclhip_ctx_set_option: the library's four tuning knobs (it reads no environment variable); unknown names and
    # negative values are refused, none of them changes a result (the served-groups / lookahead tests rely on that)
    import pcl_amd
    for name, value in (("served_groups", 0), ("served_groups", 1), ("icp_lookahead", 3), ("icp_lookahead", 1),
                        ("cache_mb", 1024), ("cache_mb", 16384)):
        gpu.setOption(name, value)
    with pytest.raises(pcl_amd.PclHipError, match="unknown option"):
        gpu.setOption("standoff", 0)
    with pytest.raises(pcl_amd.PclHipError, match="non-negative"):
        gpu.setOption("cache_mb", -1)


def test_normals_as_whole_records(gpu, bunny):
    # pclhip_normals_records: the normals of pclhip_normals laid out as whole output records (pcl::Normal: 32 bytes, normal
    # at +0, curvature at +16; other layouts alike), everything else zero, NaN for dropped points
    import ctypes as C
    from pcl_amd import _lib
    lib = _lib.load()
    cloud = xyz1(bunny["bun0"]).copy()
    cloud[5, 0] = np.nan
    tree = build_tree(gpu, cloud)
    n = len(cloud)
    vp = (C.c_float * 3)(0, 0, 10)
    ref = np.zeros((n, 4), np.float32)
    nan = C.c_uint64(0)
    _lib.check(lib.pclhip_normals(tree.h, 8, vp, C.c_void_p(ref.ctypes.data), 16, C.byref(nan)), gpu.h)
    for rec, noff, coff in ((32, 0, 16), (48, 16, 32), (16, 4, 0)):
        out = np.full((n, rec // 4), 7.0, np.float32)
        nan2 = C.c_uint64(0)
        _lib.check(lib.pclhip_normals_records(tree.h, 8, 0.0, vp, C.c_void_p(out.ctypes.data), rec, noff, coff, C.byref(nan2)), gpu.h)
        assert nan2.value == nan.value == 1
        got = np.concatenate([out[:, noff // 4:noff // 4 + 3], out[:, coff // 4:coff // 4 + 1]], axis=1)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))          # NaN rows included, bit for bit
        rest = np.ones(rec // 4, bool)
        rest[noff // 4:noff // 4 + 3] = False
        rest[coff // 4] = False
        assert np.all(out[:, rest] == 0.0)
    with pytest.raises(_lib.PclHipError):
        _lib.check(lib.pclhip_normals_records(tree.h, 8, 0.0, vp, C.c_void_p(out.ctypes.data), 32, 8, 16, C.byref(nan)), gpu.h)


def test_correspondences_as_records(gpu, orc, bunny):
    # pclhip_icp_fetch_correspondence_records: the kept pairs as 12-byte pcl::Correspondence records, compacted on the
    # device, in query order -- the same list pclhip_icp_fetch_correspondences assembles on the host
    import ctypes as C
    import pcl_amd
    from pcl_amd import _lib
    lib = _lib.load()
    src, tgt = xyz1(bunny["bun0"]).copy(), xyz1(bunny["bun4"])
    src[3, 1] = np.nan                                   # a query without a match: a gap in the dense arrays
    rec_t = np.dtype([("q", np.int32), ("m", np.int32), ("d", np.float32)])
    for chain in ((), ("median",), ("distance", "median")):
        icp = pcl_amd.IterativeClosestPoint(gpu)
        icp.setInputTarget(tgt)
        icp.setInputSource(src)
        for name in chain:
            r = pcl_amd.CorrespondenceRejectorMedianDistance() if name == "median" else pcl_amd.CorrespondenceRejectorDistance()
            if name == "median":
                r.setMedianFactor(1.2)
            else:
                r.setMaximumDistance(0.02)
            icp.addCorrespondenceRejector(r)
        icp.iterate(max_dist=0.05)
        q, m, d = icp.fetchCorrespondences()
        out = np.zeros(len(src), rec_t)
        cnt = C.c_uint64(0)
        _lib.check(lib.pclhip_icp_fetch_correspondence_records(icp.h, C.c_void_p(out.ctypes.data), len(out), C.byref(cnt)), gpu.h)
        assert cnt.value == len(q) and 0 < len(q) < len(src)
        got = out[:cnt.value]
        assert np.array_equal(got["q"], q) and np.array_equal(got["m"], m) and np.array_equal(got["d"].view(np.uint32), d.view(np.uint32))
        small = np.zeros(3, rec_t)                           # too small: the count comes back with ERR_OVERFLOW
        st = lib.pclhip_icp_fetch_correspondence_records(icp.h, C.c_void_p(small.ctypes.data), 3, C.byref(cnt))
        assert st == -5 and cnt.value == len(q)
    icp.addCorrespondenceRejector(pcl_amd.CorrespondenceRejectorOneToOne())   # re-orders the list: refused here
    icp.iterate(max_dist=0.05)
    assert lib.pclhip_icp_fetch_correspondence_records(icp.h, C.c_void_p(out.ctypes.data), len(out), C.byref(cnt)) != 0
