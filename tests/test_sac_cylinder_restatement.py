"""tests/sac_cylinder_restatement.py pinned on the reference's own criteria (test/sample_consensus/
test_sample_consensus_quadric_models.cpp:400-497 on its 20 points, tests/golden/sac_cylinder_20.npz), its refit against
scipy's MINPACK (least_squares(method="lm")): the two CPU solvers of one objective, and its bisection for the Euclidean
exit against a walk over the neighbouring floats.  No GPU."""
import itertools
import os
import struct

import numpy as np
import pytest

import sac_cylinder_restatement as cy
from test_gpu_sac_cylinder import scene

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
# The largest componentwise difference measured between the restatement's refit and MINPACK over the cases below is
# 8.9e-12 (the fixture, seed 0; MINPACK stops on ftol = xtol = gtol = 1e-8, not at the minimum: its own Gauss-Newton step
# there is 8.9e-12, the restatement's 3e-14).  The bar is that figure with a margin of 8.
MINPACK_BAR = 8 * 8.9e-12


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLD, "sac_cylinder_20.npz"))
    return np.ascontiguousarray(g["cloud"], F), np.ascontiguousarray(np.column_stack([g["normals"], np.zeros(20)]), F)


def test_the_20_points_pair_by_pair(gold):
    """every one of the 190 samples: how many score 20, how near a distance comes to the threshold, and whether the order of
    the Vector3f sums shows in a flag"""
    cloud, normals = gold
    pts, raw, un, ids = cy.point_set(cloud, normals)
    model = cy.Model(0.1)
    full, nearest, coeffs = 0, np.inf, []
    for a, b in itertools.combinations(range(20), 2):
        c, skipped = cy.model_from_samples(pts[a], pts[b], raw[a], raw[b])
        assert not skipped and np.isfinite(c).all()
        mask, in_band = model.within(pts, un, c, 0.03)
        assert in_band == 0
        full += int(mask.sum() == 20)
        nearest = min(nearest, float(np.abs(model.distances(pts, un, c) - 0.03).min()))
        coeffs.append(c)
    differ = cy.order_sensitive(dict(ndw=0.1), cloud, normals, np.array(coeffs), 0.03)
    print("pairs scoring 20: %d of 190; nearest |distance - 0.03|: %.3g; flags that differ between the orders: %d"
          % (full, nearest, differ))
    assert full > 95            # a random pair is more likely than not a winner: what lets the reference's srand(0) run pass
    assert nearest > 1e-9       # no flag of the fixture hangs on the last bits
    assert differ == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_references_criteria(gold, seed):
    cloud, normals = gold
    pts, raw, un, ids = cy.point_set(cloud, normals)
    model = cy.Model(0.1)
    ref = cy.compute_model(model, cloud, normals, 0.03, seed=seed)
    assert ref["found"] and ref["in_band"] == 0 and len(ref["sample"]) == 2 and len(ref["inliers"]) == 20
    c = ref["coefficients"]
    assert len(c) == 7 and abs(c[0] + 0.5) < 1e-3 and abs(c[1] - 1.7) < 1e-3 and abs(c[6] - 0.5) < 1e-3
    own, iterations = cy.refit(pts[ref["inliers"]], c)
    fine = cy.rounded(own)
    assert abs(fine[6] - 0.5) < 1e-3 and 0 < iterations < 100
    d = model.distances(pts, un, fine)
    print("seed %d: sample %s, refined radius %.6f, distances[0] %.6f, the rest below %.3g"
          % (seed, ref["sample"], fine[6], d[0], np.abs(d[1:]).max()))
    assert abs(d[0] - 0.020) < 1e-3 and np.abs(d[1:]).max() < 1e-3
    assert cy.evaluate(model, cloud, normals, fine, 0.021)[0][0] == 20
    assert cy.evaluate(model, cloud, normals, fine, 0.019)[0][0] == 19


def minpack(P, start):
    from scipy.optimize import least_squares
    P = np.asarray(P, np.float64)
    fr = cy.frame(start, P)
    x0 = np.array([0.0, 0.0, 0.0, 0.0, float(F(start[6]))])
    r = least_squares(lambda x: cy.residuals(x, fr, P, jac=False)[0], x0, jac=lambda x: cy.residuals(x, fr, P)[1], method="lm")
    c = cy.coefficients_of(r.x, fr)
    c[3:6] /= np.linalg.norm(c[3:6])
    return c


def refit_cases(gold):
    cloud, normals = gold
    for seed in (0, 1, 2):
        ref = cy.compute_model(cy.Model(0.1), cloud, normals, 0.03, seed=seed)
        yield "fixture seed %d" % seed, cloud[ref["inliers"]], ref["coefficients"]
    for n, seed in ((3000, 11), (1500, 17), (700, 2)):
        c, nr = scene(n, seed=seed)
        ref = cy.compute_model(cy.Model(0.1), c, nr, 0.002, max_iterations=40, seed=5)
        yield "scene %d" % n, c[ref["inliers"]], ref["coefficients"]


def test_the_refit_against_minpack(gold):
    pytest.importorskip("scipy")
    worst = 0.0
    for name, P, start in refit_cases(gold):
        own, _ = cy.refit(P, start)
        other = minpack(P, start)
        diff = float(np.abs(own - other).max())
        print("%s: %d inliers, |refit - MINPACK| %.3g, Gauss-Newton steps %.3g and %.3g"
              % (name, len(P), diff, np.abs(cy.gn_step(P, own)).max(), np.abs(cy.gn_step(P, other)).max()))
        worst = max(worst, diff)
        assert np.abs(cy.gn_step(P, own)).max() < 1e-11
    assert worst <= MINPACK_BAR, worst


def test_a_refit_that_cannot_move():
    Z = np.array([0, 0, 0, 0, 0, 1, 0.5], F)
    on = np.array([(0.5, 0, 0), (0.5, 0, 0.25), (0.5, 0, 1.0)], F)
    assert cy.refit(on, Z)[0] is None                      # no residual: no step
    assert cy.refit(np.array([(0, 0, 0.5), (0, 0, -0.5), (0, 0, 0.125)], F), Z)[0] is None  # on the axis: 0 / 0


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


@pytest.mark.parametrize("ndw,thr", [(0.1, 0.03), (0.0, 0.01), (0.5, 1e-3), (0.3, 1e-30), (0.999, 5.0), (0.25, 1e-46),
                                     (0.0, 3.4e38), (0.1, -1.0), (0.1, 0.0)])
def test_the_bisection_of_the_euclidean_exit(ndw, thr):
    """e_out is the least float whose (1 - ndw) * double(e) exceeds the threshold: walk the floats around it"""
    edge = cy.e_out(ndw, thr)
    om = 1.0 - ndw
    assert not np.isnan(edge)
    b = bits(edge)
    for k in range(max(0, b - 64), min(0x7F800000, b + 64) + 1):
        e = struct.unpack("<f", struct.pack("<I", k))[0]
        assert (np.float64(om) * np.float64(e) > thr) == (k >= b), (k, b)
    if thr < 0:
        assert edge == 0


@pytest.mark.parametrize("ndw,thr", [(1.0, 0.05), (-0.5, 0.03), (1.5, 0.03), (float("nan"), 0.03), (0.1, float("inf")),
                                     (0.1, float("nan"))])
def test_no_exit(ndw, thr):
    assert np.isnan(cy.e_out(ndw, thr))


def test_the_replay_with_exponent_2():
    """k = log(1 - p) / log(1 - w^2): with 10 of 20 inliers 0.99 needs 17 iterations (16.008...), the plane's exponent 34.5"""
    r = cy.Replay(1000, 0.99, 20)
    n = 0
    while r.feed(False, 10):
        n += 1
    assert r.iterations == 17 and cy.Replay(1000, 0.99, 20, sample_size=3).sample_size == 3
    r3 = cy.Replay(1000, 0.99, 20, sample_size=3)
    while r3.feed(False, 10):
        pass
    assert r3.iterations == 35
