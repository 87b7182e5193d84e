"""The MovingLeastSquares restatement far from the origin, without a GPU.  The cloud of tests/far_clouds.py moved by
(8192, -8192, 4096) has the same float coordinate differences as the unmoved one, so restate(unmoved) plus the shift is the
exact expectation for restate(moved) -- in exact arithmetic.  In float64 it depends on the formulation:

  query-relative     (p_j - q) - o with o = mean - q, q added once: normal and curvature stay within bound_unit, the point
                     within bound_point + far_point_term
  two-pass, one-pass both subtract a mean (or a centroid) that was rounded at the point's coordinates, 2^-40 here against
                     neighbour distances of 0.03: the fit sees every neighbour displaced by a common 1e-12 and the normal
                     leaves bound_unit.  This is why the kernel keeps its record relative to the query.

Measured worst |d| / bound (printed below; recorded next to MEASURED_WORST_SPREAD in tests/mls_restatement.py)."""
import numpy as np
import pytest

import far_clouds as fc
import mls_restatement as mr

RADII = (0.1, 0.06)
FORMS = {"two-pass": dict(), "one-pass": dict(one_pass=True), "query-relative": dict(query_relative=True)}


@pytest.fixture(scope="module")
def grid():
    return fc.grid_sheet()[0]


@pytest.fixture(scope="module")
def unmoved(grid):
    return {r: mr.restate(grid, r) for r in RADII}


def ratios(got, ref, shift, far):
    """-> worst |d| / bound of (point, normal, curvature); the point against bound_point + far"""
    keep = ~ref["excluded"]
    dp = np.abs(got["point"] - (ref["point"] + shift)).max(axis=1)[keep]
    dn = mr.normal_delta(got["normal"], ref["normal"])[keep]
    dc = np.abs(got["curvature"] - ref["curvature"])[keep]
    return (float((dp / (ref["bound_point"] + far)[keep]).max()), float((dn / ref["bound_unit"][keep]).max()),
            float((dc / ref["bound_unit"][keep]).max()))


def test_the_grid_is_what_the_cases_need(grid, unmoved):
    assert 1100 <= len(grid) <= 1200 and len(np.unique(grid, axis=0)) == len(grid)
    assert np.array_equal(grid * 1024, np.round(grid * 1024))
    for r in RADII:
        ref = unmoved[r]
        assert len(ref["indices"]) == len(grid) and ref["fitted"].mean() > 0.9 and not ref["excluded"].any()


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_moved_grid(grid, unmoved, form, r):
    ref = unmoved[r]
    far_cloud = fc.moved(grid)
    shift = np.asarray(fc.SHIFT, np.float64)
    got = mr.restate(far_cloud, r, **FORMS[form])
    assert np.array_equal(got["indices"], ref["indices"]) and np.array_equal(got["m"], ref["m"])
    assert np.array_equal(got["fitted"], ref["fitted"])
    far = mr.far_point_term(far_cloud, ref["indices"])
    assert np.array_equal(far, np.full(len(far), 2 * mr.U * np.abs(far_cloud).max(axis=1)))
    point, normal, curvature = ratios(got, ref, shift, far)
    print("moved grid r=%g %s: worst |d| / bound: point %.4f (against bound_point + far_point_term; %.1f against "
          "bound_point alone), normal %.4f, curvature %.4f" % (
              r, form, point, float((np.abs(got["point"] - (ref["point"] + shift)).max(axis=1) / ref["bound_point"]).max()),
              normal, curvature))
    if form == "query-relative":
        assert normal <= mr.SPREAD_CAP, "the query-relative form itself spreads beyond the cap: the allowance is NOT raised"
        assert max(point, normal, curvature) <= 1.0
        # near the origin the formulation is one more correct implementation: it agrees with the default within the bound
        near = mr.restate(grid, r, query_relative=True)
        assert max(ratios(near, ref, 0.0, mr.far_point_term(grid, ref["indices"]))) <= mr.SPREAD_CAP
    else:
        # the reason for the kernel's record relative to the query: a mean rounded at |q| = 8192 and subtracted again
        assert normal > 1.0 and curvature <= 1.0
        # one rounding of a double at the point already exceeds the point bound that scales with r alone
        assert float((far / 2 / ref["bound_point"]).max()) > 1.0


def test_clouds_tie_and_repeat():
    """what the device cases rely on, on the clouds alone: the moved grid has equal float squared distances among the ten
    nearest of some points (the k-NN tie rule is reached); far_raw repeats coordinates on every axis (equal keys in the index
    build) and its three axes have three different ulps"""
    pts = fc.moved(fc.grid_sheet(hole=True)[0])
    d = pts[:, None, :] - pts[None, :, :]
    d2 = np.sort((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)[:, :10]
    assert d2.dtype == np.float32 and (d2[:, 1:] == d2[:, :-1]).any(axis=1).sum() >= 10
    raw = fc.far_raw()[0]
    assert all(len(np.unique(raw[:, a])) < len(raw) - 20 for a in range(3))
    assert len({float(np.spacing(np.abs(raw[0, a]))) for a in range(3)}) == 3


def test_far_point_term_is_two_roundings():
    pts = np.array([[3.0, -5000.0, 7.0], [1.0, 2.0, -0.5], [0.0, 0.0, 0.0]], np.float32)
    assert np.array_equal(mr.far_point_term(pts, [0, 2, 1]), [2 * 2.0 ** -53 * 5000.0, 0.0, 2 * 2.0 ** -53 * 2.0])
    assert mr.far_point_term(pts, np.zeros(0, np.int32)).shape == (0,)
