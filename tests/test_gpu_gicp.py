"""GeneralizedIterativeClosestPoint (registration/include/pcl/registration/gicp.h, impl/gicp.hpp) on the device: the
functor against its per-pair restatement, the reference's own test restated, parity with the CPU restatement of the
whole loop (tests/gicp_restatement.py), a 10M-point alignment, and the edges."""
import numpy as np
import pytest

import gicp_restatement as rs

pytestmark = pytest.mark.gpu


def xyz1(a):
    out = np.ones((len(a), 4), np.float32)
    out[:, :3] = a[:, :3]
    return out


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


def make_gicp(gpu, tgt, src, **params):
    import pcl_amd
    reg = pcl_amd.GeneralizedIterativeClosestPoint(gpu)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    for k, v in params.items():
        getattr(reg, k)(v)
    return reg


def test_gicp_defaults():
    import pcl_amd
    reg = pcl_amd.GeneralizedIterativeClosestPoint(pcl_amd.default_context())
    # gicp.h:136-152, 386-431
    assert reg.getMaximumIterations() == 200 and reg.getTransformationEpsilon() == 5e-4
    assert reg.getMaxCorrespondenceDistance() == 5.0 and reg.getCorrespondenceRandomness() == 20
    assert reg.getRotationEpsilon() == 2e-3 and reg.getMaximumOptimizerIterations() == 20
    assert reg.p.min_number_correspondences == 4 and reg.p.gicp_epsilon == 1e-3
    assert reg.p.translation_gradient_tolerance == 1e-2 and reg.p.rotation_gradient_tolerance == 1e-2


def test_gicp_functor_vs_restatement(gpu, orc):
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(1 << 17)
    # both sides take the oracle's covariances: the Mahalanobis matrices then differ only by the device's arithmetic
    ct = orc.KdTree(tgt[:, :3]).gicp_covariances(tgt[:, :3], 20, 1e-3)
    cs = orc.KdTree(src[:, :3]).gicp_covariances(src[:, :3], 20, 1e-3)
    reg = make_gicp(gpu, tgt, src, setMaximumIterations=1, setSourceCovariances=cs, setTargetCovariances=ct)
    reg.align()
    want = rs.gicp_align(orc, tgt, src, src_cov=cs, tgt_cov=ct, max_iterations=1)
    si, ti, M_cpu = want["pairs"]
    assert reg.result.num_correspondences == len(si) > 0
    M = reg.mahalanobis()[si]
    assert np.all(np.abs(M - M_cpu) <= 1e-12 * np.abs(M_cpu).max(axis=(1, 2))[:, None, None]), np.abs(M - M_cpu).max()
    p, q = src[si, :3], tgt[ti, :3]
    rng = np.random.default_rng(5)
    for _ in range(5):
        x = np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.1, 0.1, 3)])  # away from the optimum
        f, g, H = reg.evaluate(x)
        tf, tg, tH = rs.dfddf_terms(x, p, q, M)
        assert abs(f - tf.sum()) <= 1e-12 * np.abs(tf).sum()
        assert np.all(np.abs(g - tg.sum(0)) <= 1e-12 * np.abs(tg).sum(0))
        assert np.all(np.abs(H - tH.sum(0)) <= 1e-12 * np.abs(tH).sum(0) + 1e-300)
        assert np.abs(g).max() > 1e-3  # not all cancellation


def test_gicp_reference_test_restated(gpu, bunny):
    # test/registration/test_registration.cpp:602-660
    import pcl_amd
    src, tgt = xyz1(bunny["bun0"]), xyz1(bunny["bun4"])
    reg = make_gicp(gpu, tgt, src, setMaximumIterations=50, setTransformationEpsilon=1e-8)
    reg.align()
    assert reg.getFitnessScore() < 1e-4
    for it in range(4):
        force_cache, force_cache_reciprocal = bool(it // 2), bool(it % 2)
        tree = pcl_amd.KdTree(gpu)
        if force_cache:
            tree.setInputCloud(tgt)
        reg.setSearchMethodTarget(tree, force_cache)
        tree_recip = pcl_amd.KdTree(gpu)
        if force_cache_reciprocal:
            tree_recip.setInputCloud(src)
        reg.setSearchMethodSource(tree_recip, force_cache_reciprocal)
        reg.align()
        assert reg.getFitnessScore() < 1e-3
    # the guess case: asserted on reg_guess (the reference asserts on `reg` there)
    ax, ay, az = 0.25 * np.pi, 0.50 * np.pi, 0.33 * np.pi

    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        R = np.eye(3)
        i, j = [(1, 2), (0, 2), (0, 1)][axis]
        R[i, i] = R[j, j] = c
        R[i, j], R[j, i] = (-s, s) if axis != 1 else (s, -s)
        return R
    T = np.eye(4)
    T[:3, :3] = rot(0, ax) @ rot(1, ay) @ rot(2, az)
    T[:3, 3] = (0.1, 0.2, 0.3)
    T = T.astype(np.float32)
    ttgt = xyz1(rs.transform_se3(T, tgt[:, :3]))
    reg_guess = make_gicp(gpu, ttgt, src, setMaximumIterations=50, setTransformationEpsilon=1e-8)
    reg_guess.align(T)
    assert reg_guess.getFitnessScore() < 1e-4


def _parity(gpu, orc, tgt, src, guess=None, **params):
    reg = make_gicp(gpu, tgt, src, **{k: v for k, v in params.items() if k.startswith("set")})
    reg.align(guess)
    want = rs.gicp_align(orc, tgt, src, guess=guess, **{k: v for k, v in params.items() if not k.startswith("set")})
    got_corr = [t["correspondences"] for t in reg.trace]
    got_inner = [t["inner_iterations"] for t in reg.trace]
    assert got_corr == want["correspondences"], (got_corr, want["correspondences"])
    assert got_inner == want["inner"], (got_inner, want["inner"])
    assert reg.nr_iterations_ == want["nr_iterations"] and reg.hasConverged() == want["converged"]
    err = np.abs(reg.getFinalTransformation().astype(np.float64) - want["T"].astype(np.float64)).max()
    assert err < 1e-5, err
    return reg, want


def test_gicp_parity_bunny(gpu, orc, bunny):
    _parity(gpu, orc, xyz1(bunny["bun4"]), xyz1(bunny["bun0"]))


def test_gicp_parity_synth(gpu, orc):
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(1 << 17)
    reg, _ = _parity(gpu, orc, tgt, src)
    assert reg.result.eval_passes >= reg.result.newton_steps >= 1


def test_gicp_nan_source_points_skipped(gpu, orc, bunny):
    tgt, src = xyz1(bunny["bun4"]), xyz1(bunny["bun0"])
    src[[3, 50, 200]] = np.nan
    reg, want = _parity(gpu, orc, tgt, src)
    assert reg.trace[0]["correspondences"] <= len(src) - 3


def test_gicp_user_covariances_verbatim(gpu, orc, bunny):
    tgt, src = xyz1(bunny["bun4"]), xyz1(bunny["bun0"])
    rng = np.random.default_rng(1)

    def covs(n):
        A = rng.normal(size=(n, 3, 3)) * 0.1
        return np.einsum("nij,nkj->nik", A, A) + 0.01 * np.eye(3)
    cs, ct = covs(len(src)), covs(len(tgt))
    import pcl_amd
    reg = pcl_amd.GeneralizedIterativeClosestPoint(gpu)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    reg.setSourceCovariances(cs)
    reg.setTargetCovariances(ct)
    reg.align()
    want = rs.gicp_align(orc, tgt, src, src_cov=cs, tgt_cov=ct)
    assert reg.result.covariance_ms == 0.0  # nothing computed
    assert [t["correspondences"] for t in reg.trace] == want["correspondences"]
    assert [t["inner_iterations"] for t in reg.trace] == want["inner"]
    assert np.abs(reg.getFinalTransformation() - want["T"]).max() < 1e-5


def test_gicp_too_few_pairs(gpu, bunny):
    tgt, src = xyz1(bunny["bun4"]), xyz1(bunny["bun0"])
    reg = make_gicp(gpu, tgt, src, setMaxCorrespondenceDistance=1e-6)
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = (0.01, 0.0, -0.02)
    reg.align(guess)
    # NotEnoughPointsException ends the loop: converged_ false, final = previous_transformation_ (identity) * guess
    assert not reg.hasConverged() and reg.nr_iterations_ == 0
    assert np.array_equal(reg.getFinalTransformation(), guess)


def test_gicp_refusals(gpu, bunny):
    import pcl_amd
    reg = pcl_amd.GeneralizedIterativeClosestPoint(gpu)
    with pytest.raises(NotImplementedError, match="BFGS"):
        reg.useBFGS()
    with pytest.raises(NotImplementedError, match="setIndices"):
        reg.setIndices(np.arange(10))
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        reg.setCommunicator(object())
    reg.setInputTarget(xyz1(bunny["bun4"]))
    reg.setInputSource(xyz1(bunny["bun0"])[:10])  # fewer points than k_correspondences
    with pytest.raises(pcl_amd.PclHipError, match="k_correspondences"):
        reg.align()


def test_gicp_at_size_10m(gpu):
    import pcl_amd
    n = 10_000_000
    tgt, src, T_gt = pcl_amd.synth.icp_pair(n)
    reg = make_gicp(gpu, tgt, src)
    reg.align()
    first = reg.getFinalTransformation().copy()
    r1 = reg.result
    assert reg.hasConverged() and r1.covariance_ms > 0
    err = np.abs(first.astype(np.float64) - T_gt).max()
    assert err < 1e-3, err
    reg.align()
    assert reg.result.covariance_ms == 0.0  # cached
    assert np.array_equal(first, reg.getFinalTransformation())  # bitwise
    print("gicp 10M: %d outer, %d Newton iterations, %d passes (%d of %d steps at alpha = 1), cov %.1f ms, total %.1f / %.1f ms,"
          " search %.1f ms, |T - T_gt|_max %.3g" %
          (r1.nr_iterations, r1.newton_iterations, r1.eval_passes, r1.newton_steps_alpha_one, r1.newton_steps,
           r1.covariance_ms, r1.total_ms, reg.result.total_ms, r1.search_ms, err))
