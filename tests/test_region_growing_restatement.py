"""The reformulation of RegionGrowing pinned without a GPU (tests/region_growing_restatement.py): the literal transcription
of the reference's flood and the two-phase, order-free formulation the kernels implement must give equal labels and
segment counts on 600 seeded random clouds (5 to 120 points, k from 2 to 8: density gradients, curvatures quantised into
ties, thresholds that make every point or no point a seed), on the roof and on the growing line; and the reference's own
criteria (test/segmentation/test_segmentation.cpp:103-112, 140-230) hold on bun0 with the oracle's normals."""
import numpy as np
import pytest

import region_growing_restatement as rr


def same(case, **kw):
    lists = rr.knn_lists(case["points"], case["k"], rr.selected(case["points"], kw.get("indices")))
    assert rr.near_threshold(case["normals"], lists, case["theta"]) == 0
    args = (case["points"], case["normals"], case["k"], case["theta"], case["curvature"])
    a = rr.literal(*args, lists=lists, **kw)
    stats = {}
    b = rr.two_phase(*args, lists=lists, stats=stats, **kw)
    assert len(a[0]) == len(b[0]) and a[2] == b[2]
    assert np.array_equal(a[1], b[1])
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    return a, stats


@pytest.mark.parametrize("block", range(6))
def test_literal_equals_two_phase_on_600_random_clouds(block):
    leftover = segments = 0
    for seed in range(block * 100, block * 100 + 100):
        (clusters, labels, _), stats = same(rr.random_case(seed))
        assert (labels >= 0).all() and len(clusters) >= 1
        leftover += stats["leftover"]
        segments += len(clusters)
    assert leftover > 0 and segments > 100  # both phases were at work in every block


def test_random_clouds_with_filters_indices_and_no_curvature_test():
    for seed in range(600, 660):
        case = rr.random_case(seed)
        n = len(case["points"])
        same(case, mn=2, mx=max(2, n // 3))
        same(case, indices=np.arange(0, n, 2))
        same(case, curvature_test=False)
        pts = case["points"].copy()
        pts[seed % n, seed % 3] = np.nan
        (_, labels, _), _ = same(dict(case, points=pts))
        assert labels[seed % n] == -1 and (np.delete(labels, seed % n) >= 0).all()


def test_roof():
    pts, nrm, which = rr.roof()
    case = dict(points=pts, normals=nrm, k=30, theta=rr.DEFAULT_THETA, curvature=rr.DEFAULT_CURVATURE)
    (clusters, labels, _), stats = same(case)
    assert len(clusters) == 2 and stats["leftover"] == 0
    assert len(set(labels[which == 0])) == 1 and len(set(labels[which == 1])) == 1
    assert labels[which == 0][0] != labels[which == 1][0]
    (cut, _, _), _ = same(dict(case, theta=np.deg2rad(0.3)))
    assert len(cut) > 4


def test_growing_line_is_directed():
    dense = rr.growing_line(lowest="dense")
    sparse = rr.growing_line(lowest="sparse")
    (a, _, _), _ = same(dict(points=dense[0], normals=dense[1], k=2, theta=rr.DEFAULT_THETA, curvature=rr.DEFAULT_CURVATURE))
    (b, _, _), _ = same(dict(points=sparse[0], normals=sparse[1], k=2, theta=rr.DEFAULT_THETA, curvature=rr.DEFAULT_CURVATURE))
    assert len(a) == 199 and len(b) == 1  # the edges point to the dense end: only the sparse end reaches everybody
    for level in (0.2, 0.001):  # phase 2 only (chosen and claimed alternate); no leftover at all
        line = rr.growing_line(lowest="sparse", level=level)
        (c, _, _), stats = same(dict(points=line[0], normals=line[1], k=2, theta=rr.DEFAULT_THETA,
                                     curvature=rr.DEFAULT_CURVATURE))
        assert stats["leftover"] == (200 if level > 0.05 else 0)
        assert len(c) == (100 if level > 0.05 else 1)


@pytest.fixture(scope="module")
def bun0_with_normals(bunny):
    from oracle import pcl_oracle as orc
    cloud = np.ascontiguousarray(bunny["bun0"][:, :3], np.float32)
    nrm, _ = orc.KdTree(cloud).normals(cloud, 10)
    return cloud, nrm


def test_reference_criteria_on_bun0(bun0_with_normals):
    cloud, nrm = bun0_with_normals
    assert np.isfinite(nrm).all()
    case = dict(points=cloud, normals=nrm, k=30, theta=rr.DEFAULT_THETA, curvature=rr.DEFAULT_CURVATURE)
    (clusters, labels, nc), _ = same(case)
    assert len(clusters) > 0 and nc == len(cloud) and (labels >= 0).all()  # RegionGrowingTest.Segment
    for fn in (rr.literal, rr.two_phase):
        assert fn(cloud, None)[0] == []                                     # SegmentWithoutNormals
        assert fn(cloud[:0], nrm[:0])[0] == []                              # SegmentEmptyCloud
        assert fn(cloud, nrm[:-1])[0] == []                                 # SegmentWithDifferentNormalAndCloudSize
        assert fn(cloud, nrm, k=0)[0] == []                                 # SegmentWithWrongThresholdParameters
