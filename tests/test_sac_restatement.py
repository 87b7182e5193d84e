"""tests/sac_restatement.py pinned: on the reference's own RANSAC plane criterion
(test/sample_consensus/test_sample_consensus_plane_models.cpp:66-103,229-241: sac_plane_test.pcd, threshold 0.03, more than
2,000 inliers, coefficients / d within 0.1 of the expected plane, the refined ones too), on the stopping rule with hand-made
count sequences, and on a plane in closed form.  CPU only."""
import os

import numpy as np
import pytest

import sac_restatement as sac

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXPECT = (-0.8964, -0.5868, -1.208)  # verifyPlaneSac: coeff[i] / coeff[3]


@pytest.fixture(scope="module")
def cloud():
    return np.ascontiguousarray(np.load(os.path.join(GOLD, "sac_plane_radius.npz"))["cloud"][:, :3], np.float32)


@pytest.mark.parametrize("seed,inliers,iterations", [(1, 2527, 8), (2, 2530, 8), (3, 2550, 8)])
def test_reference_plane_criterion(cloud, seed, inliers, iterations):
    r = sac.segment(cloud, 0.03, probability=0.99, seed=seed)
    assert r["found"] and r["skipped"] == 0
    print("seed %d: %d inliers of the winner, %d iterations, %d after the refit" %
          (seed, r["best_count"], r["iterations"], len(r["inliers"])))
    assert r["best_count"] == inliers and r["iterations"] == iterations
    assert r["best_count"] > 2000 and len(r["first_inliers"]) == r["best_count"]
    c = r["coefficients"].astype(np.float64)
    for i in range(3):
        assert abs(c[i] / c[3] - EXPECT[i]) < 0.1
    ref = r["refined"].astype(np.float64)
    assert ref is not None
    for i in range(2):
        assert abs(ref[i] / ref[3] - EXPECT[i]) < 0.1
    assert len(r["inliers"]) > 2000
    assert sorted(np.concatenate([r["inliers"], r["outliers"]]).tolist()) == list(range(len(cloud)))
    assert np.all(np.diff(r["inliers"]) > 0) and np.all(np.diff(r["outliers"]) > 0)


def test_rule_rising_best():
    # n = 100: a best of 50 gives k = log(0.01) / log(1 - 0.125) = 34.5; a best of 90 gives k = 3.5
    r = sac.replay_counts([(False, 10), (False, 50), (False, 20), (False, 90), (False, 95)], n=100)
    assert (r.iterations, r.best, r.best_trial, r.trials, r.done) == (4, 90, 3, 4, True)
    assert abs(r.k - np.log(0.01) / np.log(1 - 0.9 ** 3)) < 1e-12


def test_rule_late_tie_keeps_the_earliest():
    r = sac.replay_counts([(False, 30), (False, 30), (False, 30)] + [(False, 5)] * 200, max_iterations=6, n=100)
    assert r.best == 30 and r.best_trial == 0
    assert r.iterations == 7 and r.trials == 7 and r.done  # iterations > max_iterations


def test_rule_only_skips():
    r = sac.replay_counts([(True, 0)] * 1000, max_iterations=5, n=100)
    assert (r.skipped, r.iterations, r.best_trial, r.trials, r.done) == (50, 0, -1, 50, True)


def test_rule_max_iterations_and_zero_counts():
    r = sac.replay_counts([(False, 0)] * 1000, max_iterations=50, n=100)
    assert (r.iterations, r.trials, r.best_trial, r.done) == (51, 51, -1, True)  # a count of 0 is never a model
    r = sac.replay_counts([(True, 0), (False, 1), (True, 0), (False, 1)] + [(False, 1)] * 100, max_iterations=3, n=100)
    assert (r.iterations, r.skipped, r.trials, r.best_trial) == (4, 2, 6, 1)


def test_rule_everything_inside_stops_after_one():
    r = sac.replay_counts([(False, 100), (False, 100)], n=100)
    assert (r.iterations, r.trials, r.done) == (1, 1, True)  # p clamps to DBL_EPSILON: k = 0.13


def test_plane_z0_closed_form():
    g = np.arange(-4, 5, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size, np.float32)], 1)
    for s in ([0, 1, 9], [3, 40, 80], [80, 9, 0]):
        c, skipped = sac.plane_from_samples(*pts[s])
        assert not skipped
        assert c[0] == 0 and c[1] == 0 and abs(c[2]) == 1 and c[3] == 0
        assert np.signbit(c[3]) != np.signbit(c[2]) or c[3] == 0
        assert sac.count_within(pts, c, 1e-6) == len(pts)
    c, skipped = sac.plane_from_samples(pts[0], pts[1], pts[2])  # collinear
    assert skipped
    r = sac.segment(pts, 0.01, seed=5)
    assert r["found"] and r["best_count"] == len(pts) and r["iterations"] == 1
    assert abs(r["coefficients"][2]) == 1 and not r["coefficients"][:2].any()


def test_non_finite_sample_counts_zero_and_is_no_skip(cloud):
    p = cloud[:3].copy()
    p[1, 0] = np.nan
    c, skipped = sac.plane_from_samples(*p)
    assert not skipped and not np.isfinite(c).all()
    assert sac.count_within(cloud, c, 0.03) == 0
    assert sac.count_within(cloud, [0, 0, 1, np.inf], 0.03) == 0 and sac.count_within(cloud, [0, 0, 1, 0], 0.0) == 0


def test_unstable_flags_every_trial_far_from_the_origin():
    """The reading behind the instability cap of 0 in tests/test_gpu_sac_regimes.py: on the cloud shifted by
    (1000, -2000, 500) `unstable` flags EVERY scored trial (with |a x| + |b y| + |c z| + |d| in the thousands some point
    always lies within 4 * 2^-24 of that from the threshold), so there is no seed to change to and nothing to exclude: the
    device has to meet all of them bit for bit, which is what that module asserts.  On the unshifted scene it flags none
    of the trials here."""
    from test_gpu_sac import scene
    cloud = (scene(5000, seed=4).astype(np.float64) + np.array([1000.0, -2000.0, 500.0])).astype(np.float32)
    ref = sac.segment(cloud, 0.012, seed=2, optimize=False)
    assert (ref["trials"], ref["skipped"], ref["best_count"]) == (14, 0, 3319)
    assert all(sac.unstable(cloud, t["coefficients"], 0.012) for t in ref["trace"])
    near = scene(5000, seed=4)
    ref = sac.segment(near, 0.012, seed=2, optimize=False)
    flagged = sum(sac.unstable(near, t["coefficients"], 0.012) for t in ref["trace"] if not t["skipped"])
    print("unshifted: %d of %d trials flagged" % (flagged, ref["trials"]))
    assert flagged == 0
