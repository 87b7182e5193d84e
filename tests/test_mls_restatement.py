"""The numpy restatement of MovingLeastSquares (tests/mls_restatement.py) held to the reference's own criterion and to closed
forms, without a GPU: what tests/test_gpu_mls*.py measure the device against.  It also sets the constant of the tolerance:
the restatement's own spread under neighbour order and formulation (test_order_spread_sets_the_allowance)."""
import numpy as np
import pytest

import iss_restatement as ir
import mls_restatement as mr


@pytest.fixture(scope="module")
def bun0():
    return mr.load_bun0()


def test_bun0_meets_the_reference_s_criterion(bun0):
    """test/surface/test_moving_least_squares.cpp:95-118: bun0.pcd, r = 0.03, order 2, normals on -> record 0 within 1e-3 of
    its table (the normal by its absolute value); every one of the 397 points is output"""
    ref = mr.restate(bun0, 0.03)
    assert len(ref["indices"]) == 397 and ref["fitted"].all() and ref["m"][0] == 46
    assert np.abs(ref["point"][0] - mr.BUN0_POINT0).max() <= 1e-3
    assert np.abs(np.abs(ref["normal"][0]) - mr.BUN0_ABS_NORMAL0).max() <= 1e-3
    assert abs(ref["curvature"][0] - mr.BUN0_CURVATURE0) <= 1e-3
    # ... with three digits to spare
    assert np.abs(ref["point"][0] - (0.00541651, 0.11346323, 0.04071545)).max() <= 1e-8
    assert np.abs(np.abs(ref["normal"][0]) - (0.11189406, 0.59490598, 0.79596896)).max() <= 1e-8
    assert abs(ref["curvature"][0] - 0.01201909) <= 1e-8


@pytest.mark.parametrize("r,outputs,fits,min_gap,max_cond", [(0.03, 397, 397, 0.055, 4984.0), (0.01, 380, 163, 3.7e-4, 1.5e7),
                                                             (0.0075, 234, 11, None, None)])
def test_bun0_conditioning(bun0, r, outputs, fits, min_gap, max_cond):
    ref = mr.restate(bun0, r)
    assert (len(ref["indices"]), int(ref["fitted"].sum())) == (outputs, fits)
    assert not ref["excluded"].any()
    if min_gap is not None:
        assert ref["gap"].min() == pytest.approx(min_gap, rel=0.02) and ref["cond"].max() == pytest.approx(max_cond, rel=0.02)
    assert (ref["kappa"] >= 1).all() and (ref["cond"][~ref["fitted"]] == 1).all()
    assert (ref["m"][ref["fitted"]] >= 6).all() and (ref["m"] >= 3).all()
    lead = np.argmax(np.abs(ref["plane_normal"]), axis=1)
    assert (ref["plane_normal"][np.arange(outputs), lead] > 0).all()  # the sign rule


def test_orders_and_methods_fall_back_to_the_plane(bun0):
    full = mr.restate(bun0, 0.01)
    for order, method in ((0, mr.SIMPLE), (1, mr.SIMPLE), (2, mr.NONE)):
        other = mr.restate(bun0, 0.01, order=order, method=method)
        assert np.array_equal(other["point"], full["plane_point"]) and np.array_equal(other["normal"], full["plane_normal"])
        assert np.array_equal(other["curvature"], full["curvature"]) and np.array_equal(other["indices"], full["indices"])
    moved = (full["point"] != full["plane_point"]).any(axis=1)
    assert np.array_equal(moved, full["fitted"])


def test_plane_lattice_closed_form():
    pts = mr.plane_lattice()
    for method in (mr.SIMPLE, mr.NONE):
        ref = mr.restate(pts, 2.5, method=method)
        assert len(ref["indices"]) == len(pts) and ref["fitted"].all()
        assert np.array_equal(ref["point"], pts.astype(np.float64))  # bitwise
        assert (ref["normal"] == [0.0, 0.0, 1.0]).all() and (ref["curvature"] == 0).all()
    assert ref["m"].max() == 21 and ref["m"].min() == 8  # |v|^2 < 6.25 in the plane: 21 offsets; 8 of them at a corner


def test_rotated_plane_lattice():
    """the lattice turned into general position and rounded to float32: every input lies within sqrt(3) * 2^-21 of the plane
    (half a float32 ulp of a coordinate below 16, per axis), and so does every output up to the fit's amplification of that
    noise (a weighted quadratic fit evaluated at its centre: a factor of 4 is allowed for it)"""
    rot = mr.rotation()
    pts = np.ascontiguousarray((mr.plane_lattice().astype(np.float64) @ rot.T).astype(np.float32))
    assert np.abs(pts).max() < 16
    ref = mr.restate(pts, 2.5)
    assert len(ref["indices"]) == len(pts) and not ref["excluded"].any()
    assert (ref["curvature"] < 2.0 ** -40).all()
    noise = np.sqrt(3.0) * 2.0 ** -21
    assert (np.abs(pts.astype(np.float64) @ rot[:, 2]) <= noise).all()
    assert (np.abs(ref["point"] @ rot[:, 2]) <= 4 * noise).all()
    assert (np.abs(np.abs(ref["normal"] @ rot[:, 2]) - 1.0) <= 1e-6).all()
    # against itself in the other formulation: within the bound
    other = mr.restate(pts, 2.5, one_pass=True, moments=True)
    assert (np.abs(other["point"] - ref["point"]).max(axis=1) <= ref["bound_point"]).all()


def test_axis_line_falls_back_bitwise():
    """C = diag(s, 0, 0) exactly: the u moments are exactly 0, so is a Cholesky pivot -- no fit, the output is the input"""
    pts = mr.axis_line()
    ref = mr.restate(pts, 6.5)
    assert len(ref["indices"]) == len(pts) and (ref["m"] >= 6).all() and not ref["fitted"].any()
    assert np.array_equal(ref["point"], pts.astype(np.float64)) and (ref["curvature"] == 0).all()
    assert (ref["gap"] == 0).all() and ref["excluded"].all()  # its normal is anybody's: held to this closed form instead
    for moments in (False, True):
        assert not mr.restate(pts, 6.5, one_pass=True, moments=moments)["fitted"].any()


def test_identical_points():
    pts = np.tile(np.float32([0.25, -1.5, 3.0]), (7, 1))
    ref = mr.restate(pts, 0.5)
    assert len(ref["indices"]) == 7 and (ref["m"] == 7).all() and not ref["fitted"].any()
    assert np.array_equal(ref["point"], pts.astype(np.float64)) and (ref["curvature"] == 0).all() and ref["excluded"].all()
    assert len(mr.restate(pts[:2], 0.5)["indices"]) == 0  # m = 2


def test_neighbour_count_edges():
    pts, size = mr.edge_groups()
    assert sorted(size.tolist()) == [1] + [2] * 2 + [3] * 3 + [5] * 5 + [6] * 6
    ref = mr.restate(pts, 1.0)
    assert np.array_equal(ref["m_all"], size) and np.array_equal(ref["indices"], np.nonzero(size >= 3)[0])
    assert np.array_equal(ref["fitted"], ref["m"] == 6) and not ref["excluded"].any()


def test_strict_bound_and_non_finite_records():
    pts, _ = ir.lattice((9, 9, 9))
    centre = (4 * 9 + 4) * 9 + 4
    for r, m in ((3.0, 93), (float(np.nextafter(np.float32(3), np.float32(4))), 123)):
        assert mr.restate(pts, r, rows=[centre])["m"].tolist() == [m]
    assert len(mr.restate(pts, 1e-30)["indices"]) == 0
    pts[5] = np.nan
    ref = mr.restate(pts, 1.1)  # |v|^2 < 1.21: the six axis neighbours
    assert 5 not in ref["indices"] and len(ref["indices"]) == 728
    assert ref["m"][np.searchsorted(ref["indices"], 4)] == 4  # (0, 0, 4): itself, (0, 0, 3), (1, 0, 4), (0, 1, 4) -- not 5


def test_almost_on_a_line():
    ref = mr.restate(mr.almost_on_line(), mr.ALMOST_ON_LINE_RADIUS)
    assert len(ref["indices"]) == 4 and np.isfinite(ref["point"]).all() and np.isfinite(ref["normal"]).all()
    assert not ref["excluded"].any() and not ref["fitted"].any()


def spread_clouds(bun0):
    import pcl_amd
    rng = np.random.default_rng(3)
    cube = rng.random((1025, 3), dtype=np.float32)
    sheet = np.ascontiguousarray(pcl_amd.synth.family_cloud("sheet", 600, seed=5)[:, :3])
    rot = np.ascontiguousarray((mr.plane_lattice().astype(np.float64) @ mr.rotation().T).astype(np.float32))
    r = 0.03
    return [("bun0 r=0.03", bun0, 0.03, None), ("bun0 r=0.01", bun0, 0.01, None), ("bun0 r=0.0075", bun0, 0.0075, None),
            ("bun0 s=r^2/4", bun0, r, r * r / 4), ("bun0 s=4r^2", bun0, r, 4 * r * r), ("cube 1025", cube, 0.1, None),
            ("cube 65", cube[:65], 0.6, None), ("cube 65 r=4", cube[:65], 4.0, None),
            ("sheet 600", sheet, 4 * ir.median_spacing(sheet), None), ("groups", mr.edge_groups()[0], 1.0, None),
            ("rotated plane", rot, 2.5, None), ("almost on a line", mr.almost_on_line(), mr.ALMOST_ON_LINE_RADIUS, None)]


def test_order_spread_sets_the_allowance(bun0):
    """8 random neighbour orders, two-pass against one-pass shifted sums, matrix product against moments: the restatement moves
    by at most a quarter of the bound with A = 32 on every cloud of the device tests, and excludes no more than 1 % of any.
    MEASURED_WORST_SPREAD in tests/mls_restatement.py and DESIGN.md row f-13 record the worst ratio printed here."""
    assert mr.SOLVER_ALLOWANCE == 32
    worst_all = 0.0
    for label, pts, r, sg in spread_clouds(bun0):
        worst, moved, base = mr.spread(pts, r, sg)
        print("%-18s records %4d, fitted %4d, excluded %d: worst |d| / bound point %.4f normal %.4f curvature %.4f; moved "
              "point %.3g normal %.3g" % ((label, len(base["indices"]), int(base["fitted"].sum()),
                                           int(base["excluded"].sum())) + tuple(worst) + tuple(moved)))
        assert base["excluded"].sum() <= 0.01 * len(base["indices"])
        worst_all = max(worst_all, float(worst.max()))
    print("worst ratio over all clouds: %.4f" % worst_all)
    assert worst_all <= mr.SPREAD_CAP
