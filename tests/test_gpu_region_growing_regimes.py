"""RegionGrowing off the easy path, against the literal restatement as bytes (the recipe of
tests/test_gpu_region_growing.py: the 2-ulp guard first, two runs with equal bytes): a graph whose edges nearly all point
one way, the long dependency chain of the leftover rounds, curvature ties, coincident points beyond k, infinite
curvatures, a NaN normal, non-finite points, and one faceted cloud sized from the device's CU count."""
import numpy as np
import pytest

import region_growing_restatement as rr
from test_gpu_region_growing import check, gpu  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- 1. directed edges ------------------------------------------------------------------------------------------------------
def test_directed_line_lowest_curvature_at_either_end(gpu):  # noqa: F811
    """200 points, geometrically growing gaps, k = 2: the list of point i is (i, i - 1).  With the lowest curvature at the
    sparse end its seed reaches everybody; at the dense end nobody reaches a point of lower rank except 0 -> 1.  A
    symmetric treatment of the k-NN relation makes one segment of both."""
    pts, nrm = rr.growing_line(lowest="sparse")
    clusters, _, g = check(gpu, pts, nrm, k=2)
    assert len(clusters) == 1
    st = g.lastStats()
    assert 1 <= st["phase1_rounds"] < 200 and st["leftover"] == 0  # the shortcut works and the loop ends
    pts, nrm = rr.growing_line(lowest="dense")
    clusters, lab, g = check(gpu, pts, nrm, k=2)
    assert len(clusters) == 199 and lab[0] == lab[1] == 0
    assert 1 <= g.lastStats()["phase1_rounds"] < 200


# ---- 2. leftover rounds -----------------------------------------------------------------------------------------------------
def test_line_of_leftover_points_only(gpu):  # noqa: F811
    """every curvature above the threshold: phase 2 alone, chosen and claimed points alternate along one dependency chain"""
    pts, nrm = rr.growing_line(lowest="sparse", level=0.2)
    clusters, _, g = check(gpu, pts, nrm, k=2)
    assert [len(c) for c in clusters] == [2] * 100
    st = g.lastStats()
    assert st["leftover"] == 200 and 1 <= st["phase2_rounds"] <= 201 and st["unions"] == 0
    pts, nrm = rr.growing_line(lowest="dense", level=0.2)
    clusters, _, g = check(gpu, pts, nrm, k=2)
    assert g.lastStats()["leftover"] == 200


def test_line_without_leftover_points(gpu):  # noqa: F811
    pts, nrm = rr.growing_line(lowest="sparse", level=0.001)
    clusters, _, g = check(gpu, pts, nrm, k=2)
    st = g.lastStats()
    assert len(clusters) == 1 and st["leftover"] == 0 and st["phase2_rounds"] == 0


# ---- 3. special values ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet():
    return rr.wavy_sheet(1200, seed=23)


def clear(pts, nrm, k, theta):
    return rr.clear_theta(pts, nrm, k, theta)


def test_curvatures_quantised_to_four_values(gpu, sheet):  # noqa: F811
    pts, nrm = sheet
    q = nrm.copy()
    q[:, 3] = np.asarray([0.0, -0.0, 0.04, 0.06], np.float32)[np.arange(len(q)) % 4]  # (-0 ties with +0)
    clusters, _, g = check(gpu, pts, q, k=9, theta=clear(pts, q, 9, 0.08))
    assert len(clusters) > 3 and g.lastStats()["leftover"] > 0


def test_more_than_k_coincident_points(gpu, sheet):  # noqa: F811
    """40 copies of one point with k = 8: a copy's list holds the eight lowest copies, most lists do not hold their owner"""
    pts, nrm = sheet
    p, r = pts[:300].copy(), nrm[:300].copy()
    p[100:140] = p[100]
    clusters, lab, _ = check(gpu, p, r, k=8, theta=clear(p, r, 8, 0.15))
    assert (lab >= 0).all()


def test_infinite_curvatures(gpu, sheet):  # noqa: F811
    pts, nrm = sheet
    r = nrm.copy()
    r[5::50, 3] = np.inf   # last in the order, never expanders
    r[7::50, 3] = -np.inf  # first in the order, expanders
    clusters, lab, _ = check(gpu, pts, r, k=9, theta=clear(pts, r, 9, 0.08))
    assert (lab >= 0).all() and lab[7] == 0


def test_nan_normal_passes_the_smoothness_test(gpu, sheet):  # noqa: F811
    pts, nrm = sheet
    r = nrm.copy()
    r[3::40, 0] = np.nan
    clusters, lab, _ = check(gpu, pts, r, k=9, theta=clear(pts, r, 9, 0.08))
    assert (lab >= 0).all()  # NaN < c is false: such a point joins whoever lists it


def test_non_finite_points(gpu, sheet):  # noqa: F811
    pts, nrm = sheet
    p = pts.copy()
    bad = np.arange(4, len(p), 37)
    p[bad[0::3], 0] = np.nan
    p[bad[1::3], 1] = np.inf
    p[bad[2::3], 2] = -np.inf
    clusters, lab, _ = check(gpu, p, nrm, k=9, theta=clear(p, nrm, 9, 0.08))
    assert (lab[bad] == -1).all() and (np.delete(lab, bad) >= 0).all()


# ---- 4. every block of the list launch busy, some with a second group of queries ----------------------------------------------
def test_fullgrid_sheet(gpu):  # noqa: F811
    """The k-NN launch holds at most 8 resident blocks of 256 lanes per CU: 8 * 256 * CUs points fill every block it can
    have, 1,024 more give some a second group; the kernels of the segmentation itself run one lane per point over more
    than two thousand blocks.  The lists of the restatement come from the oracle's exact kd-tree here."""
    import torch
    from oracle import pcl_oracle as orc
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = 8 * 256 * cus + 1024
    pts, nrm, _ = rr.faceted_sheet(n, seed=31)  # (a continuum of dots would meet every float near the threshold here)
    lists, _ = orc.KdTree(pts).knn(pts, 6)
    print("fullgrid sheet: %d CUs -> %d points" % (cus, n))
    clusters, lab, g = check(gpu, pts, nrm, k=6, theta=0.1, lists=lists)
    st = g.lastStats()
    print("fullgrid sheet: %d segments, stats %r" % (len(clusters), st))
    assert len(clusters) > 100 and max(len(c) for c in clusters) > 256 and (lab >= 0).all()
    assert st["leftover"] > 0 and st["unions"] > 0
