"""GeneralizedIterativeClosestPoint off the path of tests/test_gpu_gicp.py, where every Newton step of every alignment
accepts alpha = 1 and every Mahalanobis matrix is built with R = I: the line search's other candidates and its two other
exits, the functor at the ten candidate states, the Mahalanobis matrices under a rotation, and gicp_cov_kernel away
from surfaces.

Every test first asserts ON THE RESTATEMENT (tests/gicp_restatement.py) that its input takes the branch it is meant for:
a condition on the input, so that a later change of an input cannot quietly empty a test."""
import numpy as np
import pytest

import gicp_restatement as rs
import ndt_restatement as ndt_rs
from test_gpu_gicp import make_gicp, xyz1

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


# ---- the line search ----------------------------------------------------------------------------------------------------
def line_search_parity(gpu, orc, tgt, src, label, guess=None, tolerance=None):
    """The device's alignment against the restatement's, step by step: `inner_iterations`, pair counts and f per outer
    iteration (f within 1e-12 relative: the bar of test_gicp_functor_vs_restatement for the same sums), the number of
    Newton steps that did not take alpha = 1, nr_iterations, hasConverged, and the final transformation within the 1e-5 of
    test_gpu_gicp._parity.  Returns the restatement's result."""
    reg = make_gicp(gpu, tgt, src)
    params = {}
    if tolerance is not None:
        reg.p.translation_gradient_tolerance = reg.p.rotation_gradient_tolerance = tolerance  # fields of the parameter block
        params = dict(translation_gradient_tolerance=tolerance, rotation_gradient_tolerance=tolerance)
    reg.align(guess)
    want = rs.gicp_align(orc, tgt, src, guess=guess, **params)
    alphas = [a for it in want["alphas"] for a in it]
    got_inner = [t["inner_iterations"] for t in reg.trace]
    r = reg.result
    f_err = max(abs(t["f"] - f) / abs(f) for t, f in zip(reg.trace, want["f"]))
    err = np.abs(reg.getFinalTransformation().astype(np.float64) - want["T"].astype(np.float64)).max()
    print("%s: %d outer iterations, inner %s (restated %s); %d Newton steps, %d of them at alpha = 1 (restated %d and %d; "
          "alpha < 1: %s, no candidate: %d); worst |f - f_restated| / f = %.3g; |T - T_restated|_max = %.3g" %
          (label, r.nr_iterations, got_inner, want["inner"], r.newton_steps, r.newton_steps_alpha_one, len(alphas),
           sum(a == 1.0 for a in alphas), sorted(set(a for a in alphas if 0 < a < 1), reverse=True),
           sum(a < 0 for a in alphas), f_err, err))
    assert [t["correspondences"] for t in reg.trace] == want["correspondences"]
    assert got_inner == want["inner"], (got_inner, want["inner"])
    assert r.newton_steps == len(alphas)
    assert r.newton_steps - r.newton_steps_alpha_one == sum(a != 1.0 for a in alphas)
    assert reg.nr_iterations_ == want["nr_iterations"] and reg.hasConverged() == want["converged"]
    assert len(reg.trace) == len(want["f"])
    for t, f in zip(reg.trace, want["f"]):
        assert abs(t["f"] - f) <= 1e-12 * abs(f), (t["f"], f)
    assert err < 1e-5, err
    return want, alphas


def test_gicp_line_search_from_a_guess(gpu, orc, bunny):
    """The first alignment in which a candidate other than x - delta decides a Newton step: the bunny from a guess 0.3 rad
    away.  gicp_eval_kernel<10>'s candidates 1.., the host's choice among them (`won > 0`) and the second gradient pass
    through gicp_dfddf that follows such a step.  A wrong candidate value changes `won`, hence x, f and the inner counts.
    Emulation: 10 Newton steps, 1 of them at alpha = 1/2; worst |f - f_restated| / f = 2.8e-15."""
    guess = ndt_rs.convert_transform([0.02, -0.01, 0.01, 0.3, -0.2, 0.25])
    want, alphas = line_search_parity(gpu, orc, xyz1(bunny["bun4"]), xyz1(bunny["bun0"]), "bunny from a guess", guess=guess)
    assert any(0 < a <= 0.5 for a in alphas)


def test_gicp_line_search_tight_tolerances_bunny(gpu, orc, bunny):
    """Gradient tolerances of 1e-9 keep the Newton iteration going until the line search fails: steps at alpha down to
    1/64 (`won` up to 6) and the first steps on which no candidate lowers f (`won < 0`: the inner loop ends).
    Emulation: 36 steps, 10 at alpha < 1, 6 with no candidate, inner counts [9, 7, 8, 4, 4, 4], identical on both sides."""
    want, alphas = line_search_parity(gpu, orc, xyz1(bunny["bun4"]), xyz1(bunny["bun0"]), "bunny, tolerances 1e-9",
                                      tolerance=1e-9)
    assert sum(0 < a < 1 for a in alphas) >= 3 and sum(a < 0 for a in alphas) >= 2 and min(a for a in alphas if a > 0) <= 1 / 16


def test_gicp_line_search_tight_tolerances_sheet(gpu, orc):
    """The same on the synthetic sheet at 2^13 points (emulation: 7 steps, 2 at alpha < 1, 2 with no candidate)."""
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(1 << 13)
    want, alphas = line_search_parity(gpu, orc, tgt, src, "sheet 2^13, tolerances 1e-9", tolerance=1e-9)
    assert sum(0 < a < 1 for a in alphas) >= 1 and sum(a < 0 for a in alphas) >= 1


def test_gicp_functor_at_the_ten_candidates(gpu, orc, bunny):
    """The functor at the ten states x - 2^-j delta of the first Newton step, one by one.  The candidate values of
    gicp_eval_kernel<10> are not visible through the ABI (the line-search tests above cover them through `won`); this pins
    the f of gicp_dfddf (pclhip_gicp_evaluate) at exactly those states against the restatement's `functor`, on the pairs
    and the Mahalanobis matrices of the first outer iteration, within 1e-12 relative (all terms are positive)."""
    tgt, src = xyz1(bunny["bun4"]), xyz1(bunny["bun0"])
    reg = make_gicp(gpu, tgt, src, setMaximumIterations=1)
    reg.align()
    want = rs.gicp_align(orc, tgt, src, max_iterations=1)
    si, ti, _ = want["pairs"]
    assert reg.result.num_correspondences == len(si) > 0
    M = reg.mahalanobis()[si]
    p, q = src[si, :3], tgt[ti, :3]
    x, delta, f0 = want["first_step"]
    assert np.abs(delta).max() > 1e-4
    worst, values = 0.0, []
    for j in range(10):
        cx = x - 2.0 ** -j * delta
        f = reg.evaluate(cx)[0]
        ref = rs.functor(cx, p, q, M)
        values.append(ref)
        worst = max(worst, abs(f - ref) / ref)
        assert abs(f - ref) <= 1e-12 * ref, (j, f, ref)
    print("ten candidates: f0 = %.6g, f_j / f0 = %s, worst relative difference %.3g" %
          (f0, ["%.4f" % (v / f0) for v in values], worst))
    assert len(set(values)) == 10  # ten different states


# ---- Mahalanobis matrices under a rotation -------------------------------------------------------------------------------
def inverse_longdouble(A):
    A = A.astype(LD)
    a, b, c, d, e, f, g, h, i = (A[:, r, k] for r in range(3) for k in range(3))
    co = np.stack([np.stack([e * i - f * h, c * h - b * i, b * f - c * e], 1),
                   np.stack([f * g - d * i, a * i - c * g, c * d - a * f], 1),
                   np.stack([d * h - e * g, b * g - a * h, a * e - b * d], 1)], 1)
    det = a * co[:, 0, 0] + b * co[:, 1, 0] + c * co[:, 2, 0]
    return co / det[:, None, None]


def skew_guess(angle):
    axis = np.array([0.48, -0.6, 0.64])
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = (0.02, -0.01, 0.015)
    return T.astype(np.float32)


@pytest.mark.parametrize("outer", [1, 3])
def test_gicp_mahalanobis_rotated(gpu, orc, outer):
    """M = (C_t + R C_s R^T)^-1 of gicp_pack_kernel with R != I: from a guess of 0.3 rad about a skew axis, after one outer
    iteration (R = the guess's rotation) and after three (R = transformation_ * guess mixes both).  The suite's functor
    test has R = I, which a transposed R passes.  Against the restatement's M (1e-12 of max|M| per pair, the existing bar)
    and against a long-double inverse of C_t + R C_s R^T from the same covariances; the same long-double value built with
    R^T is far outside the bar, so the comparison is known to tell R from R^T."""
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(1 << 14)
    ct = orc.KdTree(tgt[:, :3]).gicp_covariances(tgt[:, :3], 20, 1e-3)
    cs = orc.KdTree(src[:, :3]).gicp_covariances(src[:, :3], 20, 1e-3)
    guess = skew_guess(0.3)
    reg = make_gicp(gpu, tgt, src, setMaximumIterations=outer, setSourceCovariances=cs, setTargetCovariances=ct)
    reg.align(guess)
    want = rs.gicp_align(orc, tgt, src, guess=guess, src_cov=cs, tgt_cov=ct, max_iterations=outer)
    si, ti, M_cpu = want["pairs"]
    assert reg.nr_iterations_ == want["nr_iterations"] == outer
    assert reg.result.num_correspondences == len(si) > 1000
    R = want["R"]
    # R is far from its transpose: 0.3 rad at first; after three iterations the optimiser has undone most of the guess
    # and R is the pair's own 0.03 rad
    assert np.abs(R - R.T).max() > (0.1 if outer == 1 else 0.02)
    if outer == 3:
        assert np.abs(R - guess[:3, :3].astype(np.float64)).max() > 0.1  # the optimiser's part is in it
    M = reg.mahalanobis()[si]
    scale = np.abs(M_cpu).max(axis=(1, 2))
    e_rs = (np.abs(M - M_cpu).max(axis=(1, 2)) / scale).max()
    cs3, ct3 = np.asarray(cs).reshape(-1, 3, 3), np.asarray(ct).reshape(-1, 3, 3)

    def reference(Rm):
        A = np.einsum("ij,njk,lk->nil", Rm.astype(LD), cs3[si].astype(LD), Rm.astype(LD)) + ct3[ti].astype(LD)
        return inverse_longdouble(A)
    M_ld = reference(R)
    e_ld = (np.abs(M - M_ld).max(axis=(1, 2)) / scale).astype(np.float64)
    e_t = (np.abs(M - reference(R.T)).max(axis=(1, 2)) / scale).astype(np.float64)
    print("%d outer iteration(s), %d pairs: worst |M - M_restated| / max|M| = %.3g, against the long-double inverse %.3g; "
          "with R^T in the reference: median %.3g, smallest %.3g" % (outer, len(si), e_rs, e_ld.max(), np.median(e_t), e_t.min()))
    assert np.all(np.abs(M - M_cpu) <= 1e-12 * scale[:, None, None])
    assert np.all(e_ld <= 1e-12)
    assert np.median(e_t) > 1e-3  # nine orders above the bar: a transposed R cannot pass


# ---- covariances away from surfaces ----------------------------------------------------------------------------------------
def jacobi3_longdouble(A, sweeps=14):
    """Eigenvalues (ascending) and eigenvectors (columns) of n symmetric 3x3 matrices: cyclic Jacobi, np.longdouble."""
    A = A.astype(LD).copy()
    n = len(A)
    V = np.tile(np.eye(3, dtype=LD), (n, 1, 1))
    one = LD(1)
    for _ in range(sweeps):
        for p in range(2):
            for q in range(p + 1, 3):
                apq = A[:, p, q]
                go = apq != 0
                safe = np.where(go, apq, one)
                theta = (A[:, q, q] - A[:, p, p]) / (2 * safe)
                t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + 1))
                t = np.where(go, t, LD(0))
                c = one / np.sqrt(t * t + 1)
                s = t * c
                for M in (A, V):
                    mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p], M[:, :, q] = c[:, None] * mp - s[:, None] * mq, s[:, None] * mp + c[:, None] * mq
                ap, aq = A[:, p, :].copy(), A[:, q, :].copy()
                A[:, p, :], A[:, q, :] = c[:, None] * ap - s[:, None] * aq, s[:, None] * ap + c[:, None] * aq
    w = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1)
    order = np.argsort(np.abs(w), axis=1)
    return np.take_along_axis(w, order, 1), np.take_along_axis(V, order[:, None, :], 2)


def covariances_longdouble(orc, cloud, k, eps):
    """computeCovariances (impl/gicp.hpp:70-147) from the oracle's neighbour lists in np.longdouble: float differences
    to the query, their mean and covariance, the direction of the smallest singular value n, I - (1 - eps) n n^T.
    Returns (matrices, relative gap (w1 - w0) / w_max of every point)."""
    p = np.ascontiguousarray(cloud[:, :3], np.float32)
    idx, _ = orc.KdTree(p).knn(p, k)
    d = (p[idx] - p[:, None, :]).astype(LD)
    mean = d.sum(1) / LD(k)
    cov = np.einsum("nki,nkj->nij", d, d) / LD(k) - mean[:, :, None] * mean[:, None, :]
    w, V = jacobi3_longdouble(cov)
    w = np.abs(w)
    nrm = V[:, :, 0]
    want = np.eye(3, dtype=LD)[None] - (LD(1) - LD(eps)) * nrm[:, :, None] * nrm[:, None, :]
    with np.errstate(all="ignore"):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], LD(1)), LD(0))
    return want, gap.astype(np.float64)


def cov_cube():
    return xyz1(np.random.default_rng(61).uniform(-1, 1, (8000, 3)).astype(np.float32))


def cov_lines(noise):
    rng = np.random.default_rng(62)
    parts = []
    for _ in range(20):
        a, b = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        if noise == 0:  # exactly collinear in float: along one axis
            b = a.copy()
            b[rng.integers(0, 3)] += 1.0
        t = np.sort(rng.uniform(0, 1, 400))[:, None]
        parts.append(a + t * (b - a) + rng.normal(0, noise, (400, 3)) if noise else a + t * (b - a))
    return xyz1(np.concatenate(parts).astype(np.float32))


def cov_repeated():
    sites = np.random.default_rng(63).uniform(-1, 1, (2700, 3)).astype(np.float32)
    return xyz1(np.repeat(sites, 3, axis=0))


def build_tree(gpu, cloud):
    import pcl_amd
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(cloud)
    return tree


# |error| / (2.2e-16 * w_max / (w_1 - w_0)) of the oracle's own double Jacobi against the long-double value, worst over the
# clouds and k below: 3.54 (cube, k = 5; printed by the test as it runs); times 4 for another sweep order
COV_C = 14.0


@pytest.mark.parametrize("k", [5, 20, 32])
def test_gicp_covariances_off_the_surface(gpu, orc, k):
    """gicp_cov_kernel where the smallest direction of a neighbourhood is NOT well separated (the suite compares it with
    the oracle on surfaces only, flat 1e-9): a uniform cube, noisy lines (needles: two small eigenvalues), every site three
    times.  The matrix is I - (1 - eps) n n^T and n is defined to eps / gap only, so per point
        |got - want| <= COV_C * 2.2e-16 * w_max / (w_1 - w_0)
    against a long-double evaluation from the oracle's neighbour lists.  COV_C = 4 * the same ratio of the oracle's own
    double Jacobi (measured 3.54 over these clouds; the emulation's kernel gives the oracle's ratios to three digits).
    Points with a relative gap under 1e-6 have no defined answer and are left out; the clouds are chosen so that these are
    at most 1 % (asserted on the reference alone).  Exactly collinear
    neighbourhoods and neighbourhoods of one repeated site have no defined n at all: only the properties are asserted
    there (symmetric to an ulp, finite, eigenvalues {eps, 1, 1} to 1e-12)."""
    eps = 1e-3
    clouds = [("cube", cov_cube(), True), ("noisy lines", cov_lines(2e-3), True), ("collinear", cov_lines(0), False),
              ("every site three times", cov_repeated(), k > 6)]
    for name, cloud, defined in clouds:
        got = build_tree(gpu, cloud).gicpCovariances(k, eps)
        # (a, b) and (b, a) are ((1 - eps) n_a) n_b and ((1 - eps) n_b) n_a, on the oracle's side too: an ulp of an entry <= 1
        assert np.isfinite(got).all() and np.abs(got - np.transpose(got, (0, 2, 1))).max() <= 2.3e-16, name
        w = np.linalg.eigvalsh(got)
        assert np.abs(w - np.array([eps, 1.0, 1.0])).max() <= 1e-12, name
        if not defined:
            print("k = %d, %s: properties only" % (k, name))
            continue
        want, gap = covariances_longdouble(orc, cloud, k, eps)
        keep = gap >= 1e-6
        left_out = float((~keep).mean())
        assert left_out <= 0.01, (name, left_out)
        bound = 2.2e-16 / gap[keep]
        oracle = orc.KdTree(cloud[:, :3]).gicp_covariances(cloud[:, :3], k, eps)
        c_orc = (np.abs(oracle[keep] - want[keep]).max(axis=(1, 2)).astype(np.float64) / bound).max()
        err = np.abs(got[keep] - want[keep]).max(axis=(1, 2)).astype(np.float64)
        c_dev = (err / bound).max()
        print("k = %d, %s: %.2f %% of the points left out (gap < 1e-6), smallest gap kept %.3g, worst |got - want| = %.3g, "
              "worst error / (2.2e-16 w_max / gap): device %.3g, oracle %.3g" %
              (k, name, 100 * left_out, gap[keep].min(), err.max(), c_dev, c_orc))
        assert np.all(err <= COV_C * bound), (name, c_dev)
