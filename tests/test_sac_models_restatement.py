"""tests/sac_models_restatement.py on the reference's own criteria (test/sample_consensus/
test_sample_consensus_plane_models.cpp:319-397 with verifyPlaneSac's bounds), the sensitivity of its flags to the order of
the float sums, and the error of the polynomial that centres the scoring kernel's screen.  CPU tier."""
import math
import os

import numpy as np
import pytest

import sac_models_restatement as sm
import sac_restatement as sac

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETTINGS = [(ndw, thr) for ndw in (0.01, 0.1, 0.3) for thr in (0.03, 0.01)]


@pytest.fixture(scope="module")
def gold():
    cloud = np.ascontiguousarray(np.load(os.path.join(GOLD, "sac_plane_radius.npz"))["cloud"][:, :3], np.float32)
    normals = np.load(os.path.join(GOLD, "sac_plane_normals.npz"))["normals"]
    assert normals.shape == (len(cloud), 4) and normals.dtype == np.float32
    assert int(np.isnan(normals).sum()) == 60 and int(np.isnan(normals).any(axis=1).sum()) == 15
    return cloud, normals


def test_normal_plane_on_the_reference_cloud(gold):
    """SampleConsensusModelNormalPlane, RANSAC: ndw 0.01, threshold 0.03, 1,000 iterations; more than 2,000 inliers and
    coeff[0..2] / coeff[3] within 0.1 of (-0.8964, -0.5868, -1.208) before and after the refit"""
    cloud, normals = gold
    model = sm.Model(sm.NORMAL_PLANE, ndw=0.01)
    for seed in (1, 2):
        r = sm.segment(model, cloud, normals, 0.03, max_iterations=1000, seed=seed, refit=True)
        assert r["found"] and r["best_count"] > 2000 and len(r["first_inliers"]) == r["best_count"]
        assert r["in_band"] == 0
        for coeff in (r["coefficients"], r["refined"]):
            c = np.asarray(coeff, np.float64)
            assert np.abs(c[:3] / c[3] - np.array([-0.8964, -0.5868, -1.208])).max() < 0.1, (seed, c)
        bad = np.nonzero(np.isnan(normals).any(axis=1))[0]
        assert not np.isin(bad, r["first_inliers"]).any()  # a NaN normal or curvature: a NaN distance


def test_normal_parallel_plane_on_ten_coplanar_points():
    """SampleConsensusModelNormalParallelPlane, RANSAC: ten points with z = 0 and unit z normals, eps_angle 0.01: the true
    axis and one tilted by 0.01 (1 - 0.001) keep all ten, one tilted by 0.01 (1 + 0.001) keeps none -- whatever the draws"""
    rng = np.random.default_rng(0)
    cloud = np.column_stack([rng.integers(-100, 100, (10, 2)), np.zeros(10)]).astype(np.float32)
    normals = np.tile(np.array([[0, 0, 1, 0]], np.float32), (10, 1))
    eps, tilt = 0.01, 0.001
    axes = [(0, 0, 1), (0, math.sin(eps * (1 - tilt)), math.cos(eps * (1 - tilt))),
            (0, math.sin(eps * (1 + tilt)), math.cos(eps * (1 + tilt)))]
    for seed in (0, 1, 2):
        got = []
        for axis in axes:
            model = sm.Model(sm.NORMAL_PARALLEL_PLANE, axis=axis, eps_angle=eps)
            r = sm.segment(model, cloud, normals, 0.03, seed=seed)
            assert r["gate_band"] == 0 and r["in_band"] == 0
            got.append(len(r["first_inliers"]))
            if len(got) == 3:  # every trial fails the gate: iterations, not skips
                assert not r["found"] and r["iterations"] == 51 and all(not t["valid"] for t in r["trace"] if not t["skipped"])
        assert got == [10, 10, 0]


def test_order_of_the_float_sums_and_the_band(gold):
    """512 three-point hypotheses x the six settings: the flags on which the two orders of the float sums disagree (printed;
    a handful of 1,680,896 pairs) and the pairs inside the comparison band (none: the condition of every device test)"""
    cloud, normals = gold
    coeffs = sm.hypotheses(cloud, 512, seed=1)
    for ndw, thr in SETTINGS:
        model = sm.Model(sm.NORMAL_PLANE, ndw=ndw)
        ev = sm.evaluate(model, cloud, normals, coeffs, thr)
        flips = sm.order_sensitive(dict(model_type=sm.NORMAL_PLANE, ndw=ndw), cloud, normals, coeffs, thr)
        print("ndw %.2f threshold %.2f: %d order-sensitive flags, %d pairs in the band, best count %d"
              % (ndw, thr, flips, ev["in_band"], max(ev["counts"])))
        assert ev["in_band"] == 0 and flips <= 16 and max(ev["counts"]) > 50


def test_gates(gold):
    cloud, _ = gold
    z = np.array([[0, 0, 1, -1], [0, 0, -2, 3], [0, math.sin(0.2), math.cos(0.2), 0], [1, 0, 0, 0]], np.float32)
    # 9: the plane's normal within eps_angle of the axis, either sign, any length
    assert sm.Model(9, axis=(0, 0, 5), eps_angle=0.1).gate(z)[0].tolist() == [True, True, False, False]
    assert sm.Model(9, axis=(0, 0, 5), eps_angle=0.25).gate(z)[0].tolist() == [True, True, True, False]
    # 15: the plane runs along the axis: |axis . n| <= sin(eps_angle), the axis as given (not normalised)
    assert sm.Model(15, axis=(1, 0, 0), eps_angle=0.1).gate(z)[0].tolist() == [True, True, True, False]
    assert sm.Model(15, axis=(0, 1, 0), eps_angle=0.1).gate(z)[0].tolist() == [True, True, False, True]
    # 16: |axis . n| >= cos(eps_angle); eps_dist through the model only
    assert sm.Model(16, axis=(0, 0, 1), eps_angle=0.1).gate(z)[0].tolist() == [True, True, False, False]
    assert sm.Model(16, axis=(0, 0, 1), eps_angle=0.1, distance_from_origin=1.0, eps_dist=0.5).gate(z)[0].tolist() == \
        [True, False, False, False]
    # no eps_angle: no gate; a NaN passes every comparison
    for t in (0, 9, 11, 15, 16):
        assert sm.Model(t, axis=(0, 0, 1)).gate(z)[0].all()
        assert sm.Model(t, axis=(0, 0, 1), eps_angle=0.1).gate(np.full((1, 4), np.nan, np.float32))[0].all()
    # a gated segmentation finds the floor it is asked for and nothing else
    m = sm.Model(9, axis=(-0.8964, -0.5868, -1.208), eps_angle=0.05)
    r = sm.segment(m, cloud, None, 0.03, seed=1)
    assert r["found"] and r["best_count"] > 2000 and any(not t["valid"] for t in r["trace"]) and r["gate_band"] == 0
    assert all(t["count"] == 0 for t in r["trace"] if not t["valid"]) and r["skipped"] == 0


def test_zero_weight_is_the_euclidean_distance(gold):
    cloud, normals = gold
    coeffs = sm.hypotheses(cloud, 8, seed=2)
    flat = normals.copy()
    flat[:, 3] = 1.0  # curvature 1: weight 0
    for model, nrm in ((sm.Model(11, ndw=0.0), normals), (sm.Model(11, ndw=0.3), flat)):
        pts, n4, _ = sm.point_set(cloud, nrm)
        prepared = model.prepare(n4)
        ok = ~np.isnan(normals).any(axis=1)
        for c in coeffs:
            assert np.array_equal(model.within(pts, prepared, c, 0.03)[ok], sac.within(pts, c, 0.03)[ok])
            assert not model.within(pts, prepared, c, 0.03)[~ok].any()


def test_screen_polynomial():
    """|acos_poly(x) - acos(x)| in float32 over [0, 1]: a grid of 2^22 points, every float within 2^-12 of either end"""
    ends = np.arange(4097, dtype=np.float64) * 2.0 ** -24
    x = np.unique(np.concatenate([np.linspace(0, 1, 1 << 22), 1.0 - ends, ends * 2.0 ** -12]).astype(np.float32))
    err = np.abs(sm.acos_poly(x).astype(np.float64) - np.arccos(x.astype(np.float64)))
    print("largest error of the float polynomial: %.3g at x = %.9g" % (err.max(), x[err.argmax()]))
    assert err.max() < sm.SCREEN_D - 2e-6
    assert x.min() == 0.0 and x.max() == 1.0 and sm.acos_poly(np.float32(1.0)) == 0.0
