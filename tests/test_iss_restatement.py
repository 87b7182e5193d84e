"""The numpy restatement of ISSKeypoint3D (tests/iss_restatement.py) held to the reference's own criterion and to closed
forms, without a GPU: what tests/test_gpu_iss*.py measure the device against."""
import numpy as np
import pytest

import iss_restatement as ir


def test_bun0_gives_the_reference_s_six_keypoints():
    """test/keypoints/test_iss_3d.cpp:56-101: bun0.pcd, resolution 0.0058329, radii 6 x and 4 x, gammas 0.975,
    min_neighbors 5 -> exactly six keypoints, within 1e-6 of its table, in its order"""
    pts = ir.load_bun0()
    ref = ir.restate(pts, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION, 0.975, 0.975, 5)
    assert ref["keypoints"].tolist() == ir.BUN0_RECORDS
    assert np.abs(pts[ref["keypoints"]].astype(np.float64) - ir.BUN0_KEYPOINTS.astype(np.float64)).max() <= 1e-6
    assert ir.unstable(ref) == 0 and not ref["excluded"].any()
    # ... and with the bound four times as wide
    assert ir.unstable(ir.restate(pts, 6 * ir.BUN0_RESOLUTION, 4 * ir.BUN0_RESOLUTION, widen=4.0)) == 0


def test_neighbourhood_is_strict_and_in_float():
    pts, _ = ir.lattice((9, 9, 9))
    centre = np.array([(4 * 9 + 4) * 9 + 4])
    assert (pts[centre] == 4).all()
    assert ir.hits(pts, centre, 3.0).sum() == 93                                                  # |v|^2 < 9
    assert ir.hits(pts, centre, float(np.nextafter(np.float32(3), np.float32(4)))).sum() == 123  # the shell of 30 comes in
    assert ir.hits(pts, centre, 1e-30).sum() == 0 and ir.hits(pts, centre, 3e-23).sum() == 1
    assert ir.hits(pts, centre, 1e30).sum() == 729
    pts[5] = np.nan
    assert not ir.hits(pts, centre, 1e30)[0, 5] and not ir.hits(pts, np.array([5]), 1e30).any()


@pytest.mark.parametrize("r", [2.0, 3.0, float(np.nextafter(np.float32(3), np.float32(4)))])
def test_cubic_lattice_closed_form(r):
    """C = s * I for an interior point: the ratios are 1, nothing there is salient"""
    shape = (9, 9, 9)
    pts, ijk = ir.lattice(shape)
    inner = ir.lattice_interior(ijk, shape, (1, 1, 1), [r])
    m, e = ir.lattice_closed_form((1, 1, 1), r)
    assert (m, e.tolist()) == {2.0: (27, [18.0] * 3), 3.0: (93, [146.0] * 3)}.get(r, (123, [236.0] * 3))
    ref = ir.restate(pts, r, r)
    assert inner.sum() >= 1 and (ref["m"][inner] == m).all() and (ref["eig"][inner] == e).all()
    assert (ref["sal"][inner] == 0).all() and (ref["trace"][inner] == e.sum()).all()
    # min_neighbors exactly m and m + 1
    assert (ir.restate(pts, r, r, min_neighbors=m)["eig"][inner] == e).all()
    assert (ir.restate(pts, r, r, min_neighbors=m + 1)["eig"] == 0).all()


def test_anisotropic_lattice_closed_form():
    """Spacings (1, 2, 4), radii 4.25 and 3: an interior point has m = 35 and C = diag(152, 124, 96) exactly, both ratios
    pass 0.975, every interior point carries s = 96, and equal saliencies all win: every point whose non-max ball is
    interior is a keypoint"""
    shape, spacing, rs, rn = (21, 13, 9), (1, 2, 4), 4.25, 3.0
    pts, ijk = ir.lattice(shape, spacing)
    m, e = ir.lattice_closed_form(spacing, rs)
    assert (m, e.tolist()) == (35, [152.0, 124.0, 96.0]) and ir.lattice_closed_form(spacing, rn)[0] == 15
    inner = ir.lattice_interior(ijk, shape, spacing, [rs])
    core = ir.lattice_interior(ijk, shape, spacing, [rs, rn])
    assert core.sum() == 27
    ref = ir.restate(pts, rs, rn)
    assert (ref["m"][inner] == 35).all() and (ref["eig"][inner] == e).all() and (ref["sal"][inner] == 96.0).all()
    assert (ref["m_nms"][inner] == 15).all()
    flag = np.zeros(len(pts), bool)
    flag[ref["keypoints"]] = True
    assert flag[core].all()
    assert not ref["own"][inner].any()  # 124 / 152 and 96 / 124 are far from 0.975
    # min_neighbors: 15 and 35 are the two counts
    for min_neighbors, salient, keys in ((15, True, True), (16, True, False), (35, True, False), (36, False, False)):
        ref = ir.restate(pts, rs, rn, min_neighbors=min_neighbors)
        assert (ref["sal"][inner] == 96.0).all() if salient else (ref["sal"] == 0).all()
        flag = np.zeros(len(pts), bool)
        flag[ref["keypoints"]] = True
        assert flag[core].all() if keys else not flag.any()


def test_degenerate_scatter():
    same = np.tile(np.float32((0.25, -1.5, 3.0)), (50, 1))
    ref = ir.restate(same, 0.5, 0.5)
    assert (ref["m"] == 50).all() and (ref["eig"] == 0).all() and (ref["sal"] == 0).all() and len(ref["keypoints"]) == 0
    k = np.arange(60, dtype=np.float32)
    line = np.stack([k, 2 * k, -k], axis=1)
    ref = ir.restate(line, 30.0, 30.0)
    live = ref["m"] >= 5
    assert live.all() and (np.abs(ref["eig"][:, 1:]) <= ref["B"][:, None]).all() and ref["own"].all()


def test_non_finite_records_and_rejected_points():
    pts = np.random.default_rng(2).random((200, 3), dtype=np.float32)
    pts[::4, 1] = np.nan
    ref = ir.restate(pts, 0.4, 0.3)
    bad = ~np.isfinite(pts).all(axis=1)
    assert bad.sum() == 50 and np.isnan(ref["eig"][bad]).all() and (ref["sal"][bad] == 0).all() and (ref["m"][bad] == 0).all()
    assert not np.isin(ref["keypoints"], np.nonzero(bad)[0]).any() and len(ref["keypoints"]) >= 1
    assert (np.diff(ref["keypoints"]) > 0).all()
    # a negative or non-finite third eigenvalue is not salient
    e = np.array([[3.0, 2.0, -1e-18], [3.0, 2.0, np.nan], [3.0, 2.0, 1.0], [1.0, 0.99, 0.5], [0.0, 0.0, 0.0]])
    assert ir.saliency_from(e, np.full(5, 9), 0.975, 0.975, 5).tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    assert ir.saliency_from(e, np.full(5, 4), 0.975, 0.975, 5).tolist() == [0.0] * 5


def test_unstable_band_is_reported():
    """a threshold placed on a point's own ratio makes that point, and whoever has it in its non-max ball, unstable"""
    pts = np.random.default_rng(4).random((300, 3), dtype=np.float32)
    ref = ir.restate(pts, 0.3, 0.2)
    assert ir.unstable(ref) == 0
    i = int(np.argmax(ref["sal"]))
    g21 = float(ref["eig"][i, 1] / ref["eig"][i, 0])
    ref2 = ir.restate(pts, 0.3, 0.2, g21=g21)
    assert ref2["own"][i] and ref2["excluded"][i] and ref2["excluded"].sum() > ref2["own"].sum() >= 1
