"""The cylinder's scoring pass, gate, skips and refit off their easy paths: the Euclidean exit one float either side of its
edge, pairs inside the shell on both sides of the threshold, lanes that mix the three outcomes, weights at and outside
[0, 1], degenerate samples, the gate in every state, a refit that cannot move, the device's whole grid.  Same contract and
the same band as tests/test_gpu_sac_cylinder.py, asserted empty first."""
import numpy as np
import pytest

import sac_cylinder_restatement as cy
from test_gpu_sac_cylinder import (AXIS, NTILE, RADIUS, TRUE, check, check_refit, evaluated, gpu, model_of,  # noqa: F401
                                   ransac_of, scene)

pytestmark = pytest.mark.gpu
F = np.float32
Z = np.array([0, 0, 0, 0, 0, 1, 0.5], F)  # the axis z through the origin, radius 0.5


def records(pts, nrm):
    pts, nrm = np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(nrm, np.float64).reshape(-1, 3)
    return np.ascontiguousarray(pts, F), np.ascontiguousarray(np.column_stack([nrm, np.zeros(len(nrm))]), F)


@pytest.mark.parametrize("ndw,thr", [(0.1, 0.03), (0.0, 0.01), (0.5, 1e-3), (1.0, 0.05)])
def test_the_euclidean_exit_at_its_edge(gpu, ndw, thr):
    """points (+-e, 0, z) with exactly radial normals against a cylinder of radius 0: dir = (+-e, 0, 0), its norm is e and
    the angle is 0, so the distance is wed exactly.  e walks the floats either side of e_out, the least float whose wed
    exceeds the threshold.  Then radius 0.5 with points 0.5 + k 2^-24: e = k 2^-24 exactly, across the same edge."""
    edge = cy.e_out(ndw, thr)
    if ndw == 1.0:
        assert np.isnan(edge)  # (1 - ndw = 0: wed is 0, nothing exits; e = inf, from a squared norm that overflows: NaN)
        es = np.array([1e-3, 0.5, 1e10, 1e30], F)
    else:
        es = [edge]
        for _ in range(3):
            es = [np.nextafter(es[0], F(0))] + es + [np.nextafter(es[-1], F(1))]
        es = np.array(es, F)
        om = 1.0 - ndw
        assert om * float(es[2]) <= thr < om * float(es[3]) and es[3] == edge
    pts = [(s * float(e), 0.0, 0.1 * i) for i, e in enumerate(es) for s in (1, -1)]
    nrm = [(s, 0.0, 0.0) for e in es for s in (1, -1)]
    cloud, normals = records(pts, nrm)
    zero = Z.copy()
    zero[6] = 0.0
    cnt = evaluated(gpu, cloud, normals, thr, dict(ndw=ndw), zero[None])
    assert cnt[0] == 6
    if ndw != 1.0:
        k0 = int(round(float(edge) * 2 ** 24))
        ks = np.arange(k0 - 4, k0 + 5)
        pts = [(s * (0.5 + k * 2.0 ** -24), 0.0, 0.01 * i) for i, k in enumerate(ks) for s in (1, -1)]
        cloud, normals = records(pts, [(s, 0.0, 0.0) for k in ks for s in (1, -1)])
        assert np.array_equal(cloud[::2, 0].astype(np.float64) - 0.5, ks * 2.0 ** -24)
        cnt = evaluated(gpu, cloud, normals, thr, dict(ndw=ndw), Z[None])
        assert 0 < cnt[0] < len(pts)


def shell(n, angle, seed=0, toward_axis=False):
    """points ON the cylinder Z whose normals all make `angle` with the radial direction"""
    rng = np.random.default_rng(seed)
    phi, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1, 1, n)
    radial = np.column_stack([np.cos(phi), np.sin(phi), np.zeros(n)])
    other = np.tile([0.0, 0.0, 1.0], (n, 1)) if toward_axis else np.column_stack([-np.sin(phi), np.cos(phi), np.zeros(n)])
    return records(np.column_stack([0.5 * radial[:, :2], z]), np.cos(angle) * radial + np.sin(angle) * other)


@pytest.mark.parametrize("angle", [0.0, 1e-3, 0.3, np.pi / 2])
def test_pairs_inside_the_shell_either_side_of_the_threshold(gpu, angle):
    """distance = ndw * angle + a wed of float rounding; thresholds a few 1e-7 either side of it"""
    n, ndw = 1000, 0.5
    cloud, normals = shell(n, angle, seed=7, toward_axis=angle > 1.0)
    model = cy.Model(ndw)
    pts, raw, un, ids = cy.point_set(cloud, normals)
    d = model.distances(pts, un, Z)
    mid = float(np.median(d))
    # (a float dot near 1 quantises a small angle: 1e-3 comes out between 9.1e-4 and 1.04e-3)
    assert np.abs(d - mid).max() < (1e-4 if angle == 1e-3 else 1e-6) and abs(mid - ndw * angle) < 2e-5
    seen = set()
    flip = Z.copy()
    flip[3:6] = (0, 0, -2)  # (the same cylinder: the direction is normalised again)
    for thr in (mid, float(d.min()), float(np.nextafter(d.max(), 4.0)), mid + 3e-7, mid - 3e-7):
        if thr <= 0.0:
            continue
        if cy.evaluate(model, cloud, normals, Z[None], thr)[2] != 0:  # a threshold ON a distance: step off it
            thr = thr * (1.0 + 1e-11)
        cnt = evaluated(gpu, cloud, normals, thr, dict(ndw=ndw), np.vstack([Z, flip]))
        assert cnt[0] == cnt[1]
        seen.add(int(cnt[0]))
    assert len(seen) >= (2 if angle > 0 else 1) and max(seen) == n


def test_lanes_mix_the_outcomes(gpu):
    """neighbouring points alternate between out by the Euclidean exit, inside, and inside the shell with a normal that the
    exact function rejects, over three tiles and a ragged tail"""
    n = 3 * NTILE + 77
    cloud, normals = shell(n, 0.0, seed=3)
    k = np.arange(n) % 3
    cloud[k == 0, :2] *= 2.0                     # out: e = 0.5
    normals[k == 2, :3] = (0, 0, 1)              # ask, then out: the angle is pi/2
    normals[5::101, 1] = np.nan
    cloud[7::103, 2] = np.nan
    coeffs = np.vstack([Z, [0, 0, 0, 0, 0, 1, 1.0], [0.01, 0, 0, 0, 0, 1, 0.5], [0, 0, 0, 1, 0, 0, 0.5]]).astype(F)
    for thr in (0.03, 0.2):
        cnt = evaluated(gpu, cloud, normals, thr, dict(ndw=0.1), coeffs)
        assert 0 < cnt[0] < n and cnt[1] > 0


@pytest.mark.parametrize("ndw", [0.0, 1.0, -0.5, 1.5])
def test_weights_at_and_outside_the_unit_interval(gpu, ndw):
    """outside [0, 1] there is no tier 1: the result is the restatement's literal two tests"""
    cloud, normals = scene(2 * NTILE + 9, seed=21)
    coeffs = np.vstack([TRUE, cy.hypotheses(cloud, normals, 69, seed=2)])
    for thr in (0.002, 0.05):
        cnt = evaluated(gpu, cloud, normals, thr, dict(ndw=ndw), coeffs)
        assert cnt[0] > 0 or ndw == 1.5
    got, ref = check(gpu, cloud[:600], normals[:600], 0.004, dict(ndw=ndw), seed=1, max_iterations=30)
    assert np.isnan(cy.e_out(ndw, 0.004)) == (ndw not in (0.0,))


# ---- skips ------------------------------------------------------------------------------------------------------------
def test_identical_points_are_skipped(gpu):
    cloud, normals = scene(12, seed=3, nan_every=0)
    cloud[1:9] = cloud[0]
    cloud[3, 0] = np.nextafter(cloud[0, 0], F(9))  # within FLT_EPSILON: still the same point (:59-68)
    got, ref = check(gpu, cloud, normals, 0.002, dict(ndw=0.1), seed=0, max_iterations=20)
    assert ref["skipped"] > 5 and any(t["skipped"] and t["samples"][1] == 3 for t in ref["trace"])
    assert all(t["count"] == 0 and not t["valid"] for t in got["trace"] if t["skipped"])


def test_radius_limits_end_the_call_at_the_skip_limit(gpu):
    cloud, normals = scene(400, seed=5, nan_every=0)
    keep = cloud[:, 2] != F(-0.3)  # (two points of the plane have parallel normals: a NaN radius, which no limit rejects)
    cloud, normals = np.ascontiguousarray(cloud[keep]), np.ascontiguousarray(normals[keep])
    mk = dict(ndw=0.1, radius_min=10.0, radius_max=11.0)
    got, ref = check(gpu, cloud, normals, 0.002, mk, seed=2, max_iterations=6)
    assert ref["skipped"] == 60 and got["stats"]["skipped"] == 60 and ref["iterations"] <= 6 and ref["trials"] >= 60
    mk = dict(ndw=0.1, radius_min=0.045, radius_max=0.055)
    got, ref = check(gpu, cloud, normals, 0.002, mk, seed=2, max_iterations=200)
    assert ref["found"] and ref["skipped"] > 0 and any(t["skipped"] for t in got["trace"][:ref["best_trial"]])


def test_parallel_normals(gpu):
    """denominator < 1e-8 (:106-109): sc = 0; with exactly parallel normals the direction is zero and the radius NaN: no
    skip, a trial that counts 0"""
    cloud, normals = scene(300, seed=9, nan_every=0)
    normals[:, :3] = (0, 0, 1)
    got, ref = check(gpu, cloud, normals, 0.01, dict(ndw=0.1), seed=0, max_iterations=12)
    assert not ref["found"] and ref["skipped"] == 0 and ref["iterations"] == 13
    assert all(np.isnan(t["coefficients"][6]) for t in ref["trace"])
    rng = np.random.default_rng(1)
    normals[:, :2] = rng.normal(0, 2e-5, (300, 2))  # |n1 x n2|^2 ~ 1e-9
    m = model_of(gpu, cloud, normals, dict(ndw=0.1))
    small = 0
    for s in ((0, 1), (5, 200), (17, 3), (250, 251)):
        want, skipped = cy.model_from_samples(cloud[s[0]], cloud[s[1]], normals[s[0]], normals[s[1]])
        ld = cy.cross(normals[s[0], :3], normals[s[1], :3])
        small += int(0 < cy.sm.dot3(ld, ld) < 1e-8)
        got = m.computeModelCoefficients(s)
        assert not skipped and got.tobytes() == want.tobytes()
    assert small == 4
    check(gpu, cloud, normals, 0.01, dict(ndw=0.1), seed=0, max_iterations=12)


# ---- the gate ---------------------------------------------------------------------------------------------------------
def test_the_gate(gpu):
    cloud, normals = scene(1200, seed=14)
    across = np.cross(AXIS, [0, 0, 1.0])
    got, ref = check(gpu, cloud, normals, 0.002, dict(ndw=0.1, axis=AXIS, eps_angle=0.05), seed=4, max_iterations=40)
    assert ref["found"] and any(not t["valid"] and not t["skipped"] for t in ref["trace"])
    got, ref = check(gpu, cloud, normals, 0.002, dict(ndw=0.1, axis=across, eps_angle=0.05), seed=4, max_iterations=40)
    assert all(t["count"] == 0 for t in ref["trace"] if not t["valid"])
    free, _ = check(gpu, cloud, normals, 0.002, dict(ndw=0.1, axis=across, eps_angle=0.0), seed=4, max_iterations=40)
    plain, _ = check(gpu, cloud, normals, 0.002, dict(ndw=0.1), seed=4, max_iterations=40)
    assert free["inliers"].tobytes() == plain["inliers"].tobytes() and all(t["valid"] or t["skipped"] for t in free["trace"])
    # the selections and the distances of an invalid model are empty
    m = model_of(gpu, cloud, normals, dict(ndw=0.1, axis=across, eps_angle=0.05))
    assert m.countWithinDistance(TRUE, 0.002) == 0 and len(m.selectWithinDistance(TRUE, 0.002)) == 0
    assert len(m.getDistancesToModel(TRUE)) == 0
    out = m.optimizeModelCoefficients(plain["inliers"], TRUE)
    assert out.tobytes() == TRUE.tobytes() and not m.lastOptimize()["refined"]
    coeffs = np.vstack([TRUE, cy.hypotheses(cloud, normals, 66, seed=3)])
    evaluated(gpu, cloud, normals, 0.002, dict(ndw=0.1, axis=AXIS, eps_angle=0.3, radius_min=0.04, radius_max=0.06), coeffs)


def test_radius_limits_that_the_refined_radius_leaves(gpu):
    """the unrefined winner passes the gate, the refined cylinder does not: an empty list, the refined coefficients"""
    cloud, normals = scene(1500, seed=17)
    mk = dict(ndw=0.1)
    for _ in range(8):  # (a limit skips other trials too and may change the winner: repeat until it stays)
        ref = cy.compute_model(cy.Model(**mk), cloud, normals, 0.002, max_iterations=40, seed=6)
        r0 = float(ref["coefficients"][6])
        own, _ = cy.refit(cloud[ref["inliers"]], ref["coefficients"])
        r1 = float(own[6])
        assert abs(r1 - r0) > 1e-6
        if not cy.Model(**mk).gate(cy.rounded(own))[0]:
            break
        mid = 0.5 * (r0 + r1)
        mk = dict(ndw=0.1, radius_min=mid, radius_max=1.0) if r0 > r1 else dict(ndw=0.1, radius_min=0.0, radius_max=mid)
    assert not cy.Model(**mk).gate(cy.rounded(own))[0] and cy.Model(**mk).gate(ref["coefficients"])[0]
    got, ref2 = check(gpu, cloud, normals, 0.002, mk, seed=6, max_iterations=40)
    assert ref2["found"] and ref2["coefficients"].tobytes() == ref["coefficients"].tobytes()
    inl, coeff, outl = got["ransac"].segment(True)
    assert got["ransac"].stats()["refined"] and len(inl) == 0 and len(outl) == len(cloud)
    assert abs(float(coeff[6]) - r1) < 1e-6 and not cy.Model(**mk).gate(coeff)[0]
    check_refit(cloud, got["inliers"], got["coefficients"], coeff)


# ---- a refit that cannot move -----------------------------------------------------------------------------------------
def test_the_refits_failures(gpu):
    pts = [(0.5, 0.0, 0.0), (0.5, 0.0, 0.25), (0.5, 0.0, 1.0), (0.0, 0.0, 0.5), (0.0, 0.0, -0.5), (0.0, 0.0, 0.125), (0.3, 0.4, 2)]
    cloud, normals = records(pts, [(1, 0, 0)] * len(pts))
    m = model_of(gpu, cloud, normals, dict(ndw=0.1))
    for inliers, why in (([0, 1, 2], "three collinear inliers ON the cylinder: no residual, no step"),
                         ([3, 4, 5], "inliers on the axis: the Jacobian divides by a distance of 0"),
                         ([0, 6], "two inliers: not more than the sample size (:282-286)"), ([], "no inlier")):
        out = m.optimizeModelCoefficients(np.array(inliers, np.int32), Z)
        assert out.tobytes() == Z.tobytes() and not m.lastOptimize()["refined"], why
        assert len(inliers) < 3 or cy.refit(cloud[inliers], Z)[0] is None, why


def test_fullgrid(gpu):
    """A block of the scoring kernel takes 2,048 points per tile and a CU holds at most 8 blocks of 256 threads, so whatever
    occupancy the runtime reports, (8 * CUs + 3) tiles give some blocks a second tile; 17 more points leave the last tile
    ragged.  (On the emulation, with its 32 blocks, the cases above reach a block's second tile already.)"""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = (8 * cus + 3) * NTILE + 17
    cloud, normals = scene(n, seed=1)
    off = TRUE.copy()
    off[6] = 0.08
    cnt = evaluated(gpu, cloud, normals, 0.002, dict(ndw=0.1), np.vstack([TRUE, off]))
    print("fullgrid scene: %d CUs -> %d points, counts %s" % (cus, n, cnt.tolist()))
    assert cnt[0] > n // 3 > cnt[1]
