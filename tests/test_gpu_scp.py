"""pclhip_feature_knn / pclhip_scp_* / pcl_amd.SampleConsensusPrerejective on the device against the numpy restatement
(tests/scp_restatement.py, the same draw function).

Feature k-NN: indices and distances bit for bit.  pclhip_scp_evaluate: inlier counts exactly those of a brute force over the
bit-exact moved cloud, errors within (count + 4) * 2^-24 relative of the float64 mean -- the bound of the reference's own
sequential float32 sum -- and bit-identical between two calls and between a batch and single calls.  The alignment through
its trace: samples, matches and rejected flags equal to the restatement's; T against float64 umeyama of the same pairs within
T_TOL (below); count and error equal to pclhip_scp_evaluate of the device's own T; the winner is the first minimum of the
trace under the acceptance rule; the inlier list is the brute force's for the winning T.

T_TOL.  The device runs scp_rotation (pcl_amd/csrc/scp.hpp: Jacobi on sigma^T sigma, double) where the restatement runs numpy's SVD; both
round to float32.  On well-conditioned pairs they agree to an ulp of float32 (6e-8 of an entry of R, |t| * 6e-8 of t); the
eigen-decomposition of sigma^T sigma squares the condition of a thin sample triangle, which the point-to-point ICP tests
allow for with 1e-5 on the 4x4 (smoke(), tests/test_gpu_loop.py).  Here: 1e-5 on the entries of R and 1e-5 * (1 + |t|_inf)
on t, for triangles whose smallest height is at least 5 % of their longest edge (thinner ones are skipped: their rotation
about the long edge is not determined to that precision by either solver).  With nr_samples == 2 the rotation about the edge
is free: there the test asks for a rigid motion that reaches the optimal residual."""
import os

import numpy as np
import pytest

import scp_restatement as sr

pytestmark = pytest.mark.gpu
ON_EMULATION = os.environ.get("PCLHIP_ALLOW_WAVESIM") == "1"
FLT_MAX = sr.FLT_MAX


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(np.float32)


# ---- feature k-NN --------------------------------------------------------------------------------------------------------
def knn_rows(nt, nq, D, seed):
    rng = np.random.default_rng(seed)
    t = rng.random((nt, D), dtype=np.float32)
    q = rng.random((nq, D), dtype=np.float32)
    if nt >= 15:
        t[7] = t[3]          # duplicated rows: the lower index wins
        t[11] = t[3]
        t[5, D // 2] = np.nan  # never a candidate
        t[9, 0] = np.inf
        q[0] = t[3]          # distance 0 to three rows
    q[min(2, nq - 1), D - 1] = np.nan  # a query without neighbours
    return t, q


@pytest.mark.parametrize("nt", [1, 15, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_feature_knn_bitwise(gpu, nt, k):
    import pcl_amd
    t, q = knn_rows(nt, 70, 33, 100 * nt + k)  # 70 queries: two waves, the second one partly filled
    idx, d2, cnt = pcl_amd.featureKSearch(gpu, t, q, k)
    ridx, rd2, rcnt = sr.feature_knn(t, q, k)
    assert np.array_equal(cnt, rcnt)
    assert cnt.max() == min(k, int(np.isfinite(t).all(axis=1).sum())) and cnt[2] == 0  # k > finite rows: clamped
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(d2), bits(rd2))
    if nt >= 15 and k >= 2:
        assert idx[0, 0] == 3 and idx[0, 1] == 7 and d2[0, 1] == 0.0


@pytest.mark.parametrize("D", [1, 8, 64])
def test_feature_knn_other_dimensions_and_device_buffers(gpu, D):
    import pcl_amd
    t, q = knn_rows(130, 9, D, D)
    ridx, rd2, rcnt = sr.feature_knn(t, q, 5)
    idx, d2, cnt = pcl_amd.featureKSearch(gpu, t, q, 5)
    assert np.array_equal(idx, ridx) and np.array_equal(bits(d2), bits(rd2)) and np.array_equal(cnt, rcnt)
    if not ON_EMULATION:
        import torch
        idx2, d22, cnt2 = pcl_amd.featureKSearch(gpu, torch.from_numpy(t).cuda(), torch.from_numpy(q).cuda(), 5)
        assert np.array_equal(idx2, idx) and np.array_equal(bits(d22), bits(d2)) and np.array_equal(cnt2, cnt)


def test_feature_knn_errors(gpu):
    import pcl_amd
    from pcl_amd import PclHipError
    t, q = knn_rows(20, 3, 33, 1)
    for bad_k in (0, 33):
        with pytest.raises(PclHipError) as e:
            pcl_amd.featureKSearch(gpu, t, q, bad_k)
        assert e.value.status == -1
    with pytest.raises(PclHipError) as e:
        pcl_amd.featureKSearch(gpu, np.zeros((4, 65), np.float32), np.zeros((1, 65), np.float32), 1)
    assert e.value.status == -1
    with pytest.raises(PclHipError) as e:  # no finite target row
        pcl_amd.featureKSearch(gpu, np.full((4, 33), np.nan, np.float32), q, 1)
    assert e.value.status == -4


# ---- pclhip_scp_evaluate ---------------------------------------------------------------------------------------------------
def surface(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * 2 - 1
    z = 0.3 * np.sin(2.1 * xy[:, 0]) * np.cos(1.7 * xy[:, 1]) + 0.2 * xy[:, 0] * xy[:, 1]
    return np.column_stack([xy, z]).astype(np.float32)


def make_scp(gpu, src, tgt, corr_dist, fs=None, ft=None):
    import pcl_amd
    s = pcl_amd.SampleConsensusPrerejective(gpu)
    s.setInputSource(src)
    s.setInputTarget(tgt)
    s.setMaxCorrespondenceDistance(corr_dist)
    if fs is not None:
        s.setSourceFeatures(fs)
        s.setTargetFeatures(ft)
    return s


def check_scores(src, tgt, Ts, corr_dist, cnt, err):
    for T, c, e in zip(Ts, cnt, err):
        inl, _, e64 = sr.get_fitness(src, tgt, T, corr_dist)
        assert int(c) == len(inl)
        if len(inl) == 0:
            assert e == FLT_MAX
        else:
            assert abs(float(e) - e64) <= (len(inl) + 4) * 2.0 ** -24 * e64


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 1000])
def test_evaluate_counts_exact_errors_bounded_bits_repeat(gpu, ns):
    tgt = surface(700, 5)
    rng = np.random.default_rng(ns)
    src = (tgt[rng.permutation(700)[:min(ns, 700)]] if ns <= 700 else surface(ns, 6))
    src = (src + rng.normal(0, 0.01, src.shape)).astype(np.float32)
    corr = 0.05
    Ts = [np.eye(4, dtype=np.float32), rigid(0, 0, 0, [50, 0, 0])]  # the identity; outside the target's box
    for _ in range(63):
        Ts.append(rigid(*rng.normal(0, 0.03, 3), rng.normal(0, 0.03, 3)))
    Ts = np.stack(Ts)
    s = make_scp(gpu, src, tgt, corr)
    cnt, err = s.evaluate(Ts)  # H = 65 in one call
    assert cnt[1] == 0 and err[1] == FLT_MAX
    check_scores(src, tgt, Ts, corr, cnt, err)
    cnt2, err2 = s.evaluate(Ts)  # two calls agree bit for bit
    assert np.array_equal(cnt, cnt2) and np.array_equal(bits(err), bits(err2))
    c2, e2 = s.evaluate(Ts[3:5])  # H = 2
    assert np.array_equal(c2, cnt[3:5]) and np.array_equal(bits(e2), bits(err[3:5]))
    for h in (0, 1, 2, 64):  # H = 1: a batch gives the bits of single calls
        c1, e1 = s.evaluate(Ts[h:h + 1])
        assert c1[0] == cnt[h] and bits(e1)[0] == bits(err)[h]
    s.setBatchSize(7)  # chunks that do not divide H
    c7, e7 = s.evaluate(Ts)
    assert np.array_equal(c7, cnt) and np.array_equal(bits(e7), bits(err))


def test_evaluate_identity_on_itself_and_the_strict_bound(gpu):
    tgt = surface(300, 9)
    s = make_scp(gpu, tgt, tgt, 0.05)
    cnt, err = s.evaluate(np.eye(4, dtype=np.float32)[None])
    assert cnt[0] == 300 and err[0] == 0.0  # all inliers, error 0
    # a point at exactly d2 == float(corr_dist^2) is no inlier: target at the origin, source at (0.5, 0, 0), distance 0.5
    origin = np.zeros((1, 3), np.float32)
    s = make_scp(gpu, np.array([[0.5, 0, 0]], np.float32), origin, 0.5)
    cnt, err = s.evaluate(np.eye(4, dtype=np.float32)[None])
    assert cnt[0] == 0 and err[0] == FLT_MAX
    s = make_scp(gpu, np.array([[np.nextafter(np.float32(0.5), np.float32(0)), 0, 0]], np.float32), origin, 0.5)
    cnt, err = s.evaluate(np.eye(4, dtype=np.float32)[None])
    assert cnt[0] == 1 and err[0] == np.nextafter(np.float32(0.5), np.float32(0)) ** 2
    # the default distance (sqrt(DBL_MAX): the float bound is +inf) scores everything
    s = make_scp(gpu, tgt[:50] + np.float32(3.0), tgt, np.sqrt(np.finfo(np.float64).max))
    cnt, err = s.evaluate(np.eye(4, dtype=np.float32)[None])
    assert cnt[0] == 50
    check_scores(tgt[:50] + np.float32(3.0), tgt, np.eye(4, dtype=np.float32)[None], np.sqrt(np.finfo(np.float64).max), cnt, err)


# ---- the alignment ---------------------------------------------------------------------------------------------------------
CORR = 0.04
T_GT = rigid(0.4, -0.3, 1.1, [0.5, -0.2, 0.3])


@pytest.fixture(scope="module")
def scene():
    """target: 260 surface points; source: 150 of them (with 0.002 of noise) + 40 strangers, moved by the inverse of T_GT (partial overlap), with
    random 33-float descriptors that match their target point up to noise"""
    rng = np.random.default_rng(42)
    tgt = surface(260, 1)
    ft = rng.random((260, 33), dtype=np.float32)
    pick = rng.permutation(260)[:150]
    strangers = (surface(40, 2) + np.float32([0.3, 2.5, 0.4])).astype(np.float32)
    pts = np.concatenate([tgt[pick], strangers])
    fs = np.concatenate([ft[pick] + rng.normal(0, 0.02, (150, 33)).astype(np.float32), rng.random((40, 33), dtype=np.float32)])
    inv = np.linalg.inv(T_GT.astype(np.float64))
    src = (pts.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3] + rng.normal(0, 0.002, pts.shape)).astype(np.float32)
    order = rng.permutation(len(src))
    return dict(src=np.ascontiguousarray(src[order]), tgt=tgt, fs=np.ascontiguousarray(fs[order]), ft=ft)


def run_align(gpu, sc, iters, ns=3, k=3, sim=0.8, frac=0.0, seed=5, guess=None, batch=None, trace=True, corr=CORR):
    s = make_scp(gpu, sc["src"], sc["tgt"], corr, sc["fs"], sc["ft"])
    s.setMaximumIterations(iters)
    s.setNumberOfSamples(ns)
    s.setCorrespondenceRandomness(k)
    s.setSimilarityThreshold(sim)
    s.setInlierFraction(frac)
    s.setSeed(seed)
    if batch:
        s.setBatchSize(batch)
    s.align(guess=guess, trace_capacity=iters if trace else 0)
    return s


def triangle_is_thick(p):
    e = [np.linalg.norm(p[i] - p[(i + 1) % 3]) for i in range(3)]
    area2 = np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0]))
    return max(e) > 0 and area2 / max(e) >= 0.05 * max(e)


def check_trace(gpu, sc, s, iters, ns, k, sim, frac, seed, guess=None):
    """everything the trace promises, against the restatement run on the device's own transforms"""
    src, tgt = sc["src"], sc["tgt"]
    assert len(s.trace) == iters
    dev_T = {t["iteration"]: t["transformation"] for t in s.trace}
    r = sr.align(src, tgt, sc["fs"], sc["ft"], max_iterations=iters, nr_samples=ns, k=k, similarity=sim, inlier_fraction=frac,
                 corr_dist=CORR, seed=seed, guess=guess, transforms=dev_T)
    worst_R = worst_t = 0.0
    for d, w in zip(s.trace, r["trace"]):
        assert d["iteration"] == w["iteration"] and d["samples"] == w["samples"] and d["matches"] == w["matches"]
        assert d["rejected"] == w["rejected"]
        if d["rejected"]:
            continue
        T, T64 = d["transformation"].astype(np.float64), w["T64"]
        if ns >= 3 and (ns > 3 or (triangle_is_thick(src[d["samples"]].astype(np.float64)) and
                                   triangle_is_thick(tgt[d["matches"]].astype(np.float64)))):
            worst_R = max(worst_R, np.abs(T[:3, :3] - T64[:3, :3]).max())
            worst_t = max(worst_t, np.abs(T[:3, 3] - T64[:3, 3]).max() / (1 + np.abs(T64[:3, 3]).max()))
        else:  # a free rotation: a rigid motion with the optimum's residual
            R = T[:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R) - 1) < 1e-5
            ps, pt = src[d["samples"]].astype(np.float64), tgt[d["matches"]].astype(np.float64)
            res = ((ps @ R.T + T[:3, 3] - pt) ** 2).sum()
            opt = ((ps @ T64[:3, :3].T + T64[:3, 3] - pt) ** 2).sum()
            assert res <= opt + 1e-5 * (pt ** 2).sum()
    print("umeyama: worst |R - R64| = %.3g, worst |t - t64| / (1 + |t|) = %.3g" % (worst_R, worst_t))
    assert worst_R <= 1e-5 and worst_t <= 1e-5
    # count and error: pclhip_scp_evaluate of the device's own T, bit for bit; the restatement's count exactly
    scored = [d for d in s.trace if not d["rejected"]]
    assert s.result.rejected == iters - len(scored) == r["rejected"]
    if scored:
        cnt, err = s.evaluate(np.stack([d["transformation"] for d in scored]))
        for d, c, e in zip(scored, cnt, err):
            assert d["inliers"] == int(c) and bits(d["error"])[()] == bits(e)[()]
        for d, w in zip(s.trace, r["trace"]):
            if not d["rejected"]:
                assert d["inliers"] == w["inliers"]
                if w["inliers"]:
                    assert abs(float(d["error"]) - w["error64"]) <= (w["inliers"] + 4) * 2.0 ** -24 * w["error64"]
    return r, scored


def winner_of(scored, n_src, frac, guess_score=None):
    """the first minimum under the acceptance rule (:284-293) -> (iteration or -1 / -2, error)"""
    best_it, lowest = -2, FLT_MAX
    if guess_score is not None and np.float32(guess_score[0]) / np.float32(n_src) >= np.float32(frac) and guess_score[1] < lowest:
        best_it, lowest = -1, guess_score[1]
    for d in scored:
        if np.float32(d["inliers"]) / np.float32(n_src) >= np.float32(frac) and d["error"] < lowest:
            best_it, lowest = d["iteration"], d["error"]
    return best_it, lowest


@pytest.mark.parametrize("ns,k", [(3, 3), (2, 2), (4, 1)])
def test_align_trace_against_the_restatement(gpu, scene, ns, k):
    iters, sim, frac, seed = 200, 0.8, 0.3, 5 + ns
    s = run_align(gpu, scene, iters, ns=ns, k=k, sim=sim, frac=frac, seed=seed)
    r, scored = check_trace(gpu, scene, s, iters, ns, k, sim, frac, seed)
    n = len(scene["src"])
    # the restatement's best and second-best eligible errors differ by more than the bound of the summation
    elig = sorted((w["error64"], w["inliers"]) for w in r["trace"]
                  if not w["rejected"] and np.float32(w["inliers"]) / np.float32(n) >= np.float32(frac))
    # (with two samples the rotation about the edge is free and an eligible hypothesis is rare: a single one has no rival)
    assert len(elig) >= (1 if ns == 2 else 2), "the scene must give eligible hypotheses"
    if len(elig) >= 2:
        assert elig[1][0] - elig[0][0] > 2 * (max(elig[0][1], elig[1][1]) + 4) * 2.0 ** -24 * elig[1][0]
    best_it, lowest = winner_of(scored, n, frac)
    assert s.hasConverged() and r["converged"]
    assert s.result.best_iteration == best_it == r["best_iteration"]
    assert bits(s.result.best_error)[()] == bits(lowest)[()]
    win = next(d for d in s.trace if d["iteration"] == best_it)
    assert np.array_equal(bits(s.getFinalTransformation()), bits(win["transformation"]))
    assert s.result.best_count == win["inliers"]
    # the inlier list: brute force for the winning T, ascending
    inl, _, _ = sr.get_fitness(scene["src"], scene["tgt"], win["transformation"], CORR)
    got = s.getInliers()
    assert np.array_equal(got, inl) and len(got) == win["inliers"]
    # ... and the pose is the scene's
    assert np.abs(s.getFinalTransformation() - T_GT).max() < 0.05
    out = s.align(want_output=True)
    assert np.array_equal(bits(out[:, :3]), bits(sr.transform_se3(s.getFinalTransformation(), scene["src"])))


def test_align_does_not_depend_on_the_batch_size(gpu, scene):
    a = run_align(gpu, scene, 100, batch=100, seed=3, frac=0.3)   # divides
    b = run_align(gpu, scene, 100, batch=7, seed=3, frac=0.3)     # does not
    c = run_align(gpu, scene, 100, seed=3, frac=0.3)              # one batch
    for x in (b, c):
        assert x.result.best_iteration == a.result.best_iteration and x.result.rejected == a.result.rejected
        assert bits(x.result.best_error)[()] == bits(a.result.best_error)[()]
        assert np.array_equal(bits(x.getFinalTransformation()), bits(a.getFinalTransformation()))
        assert np.array_equal(x.getInliers(), a.getInliers())
        assert [(t["samples"], t["matches"], t["rejected"], t["inliers"]) for t in x.trace] == \
               [(t["samples"], t["matches"], t["rejected"], t["inliers"]) for t in a.trace]
    again = run_align(gpu, scene, 100, batch=7, seed=3, frac=0.3, trace=False)  # without a trace: the same result
    assert again.result.best_iteration == a.result.best_iteration and again.result.trace_count == 0
    assert np.array_equal(again.getInliers(), a.getInliers())
    other = run_align(gpu, scene, 100, seed=4, frac=0.3)
    assert [t["samples"] for t in other.trace] != [t["samples"] for t in a.trace]


def test_align_guess_is_scored_first(gpu, scene):
    n = len(scene["src"])
    # a good guess, no iteration: it is the result
    s = run_align(gpu, scene, 0, guess=T_GT)
    cnt, err = s.evaluate(T_GT[None])
    assert s.hasConverged() and s.result.best_iteration == -1 and s.result.best_count == cnt[0] >= 150
    assert bits(s.result.best_error)[()] == bits(err)[0]
    assert np.array_equal(bits(s.getFinalTransformation()), bits(T_GT))
    inl, _, _ = sr.get_fitness(scene["src"], scene["tgt"], T_GT, CORR)
    assert np.array_equal(s.getInliers(), inl)
    # the guess takes part in the same comparison, ahead of iteration 0
    s = run_align(gpu, scene, 60, guess=T_GT, frac=0.3, seed=8)
    scored = [d for d in s.trace if not d["rejected"]]
    best_it, lowest = winner_of(scored, n, 0.3, guess_score=(cnt[0], err[0]))
    assert s.result.best_iteration == best_it and bits(s.result.best_error)[()] == bits(lowest)[()]
    # a guess that is isApprox(Identity, 0.01f) is not scored: no iteration, nothing accepted
    near = np.eye(4, dtype=np.float32)
    near[0, 3] = 0.005
    s = run_align(gpu, scene, 0, guess=near)
    assert not s.hasConverged() and s.result.best_iteration == -2 and np.array_equal(s.getFinalTransformation(), near)
    assert len(s.getInliers()) == 0 and s.align(guess=near, want_output=True) is None


def test_align_inlier_fraction_one_on_partial_overlap(gpu, scene):
    g = rigid(0.1, 0.2, 0.3, [1, 2, 3])
    s = run_align(gpu, scene, 80, frac=1.0, guess=g)
    assert not s.hasConverged() and s.result.best_iteration == -2
    assert np.array_equal(bits(s.getFinalTransformation()), bits(g))  # the final transformation is the guess
    assert len(s.getInliers()) == 0 and s.result.best_error == FLT_MAX
    assert any(not d["rejected"] for d in s.trace)  # hypotheses were scored, none was accepted


def test_align_one_and_zero_iterations(gpu, scene):
    s = run_align(gpu, scene, 0)
    assert not s.hasConverged() and s.result.iterations == 0 and s.result.rejected == 0 and len(s.trace) == 0
    assert np.array_equal(s.getFinalTransformation(), np.eye(4, dtype=np.float32))
    s = run_align(gpu, scene, 1, sim=0.0, seed=2)  # similarity 0: the pre-rejection is off
    check_trace(gpu, scene, s, 1, 3, 3, 0.0, 0.0, 2)
    d = s.trace[0]
    assert d["rejected"] == 0 and s.result.rejected == 0
    assert s.hasConverged() == (d["inliers"] > 0) and (not s.hasConverged() or s.result.best_iteration == 0)


def test_align_non_finite_feature_rows(gpu, scene):
    sc = dict(scene)
    sc["fs"] = scene["fs"].copy()
    sc["fs"][::3, 4] = np.nan  # a third of the source rows: their hypotheses count as rejected (2)
    sc["ft"] = scene["ft"].copy()
    sc["ft"][::5, 0] = np.nan  # never matched
    s = run_align(gpu, sc, 60, seed=11)
    r, _ = check_trace(gpu, sc, s, 60, 3, 3, 0.8, 0.0, 11)
    assert any(d["rejected"] == 2 for d in s.trace)
    assert all(m % 5 != 0 for d in s.trace for m in d["matches"] if m >= 0)


def test_align_error_returns(gpu, scene):
    import pcl_amd
    from pcl_amd import PclHipError

    def status(fn):
        with pytest.raises(PclHipError) as e:
            fn()
        return e.value.status

    s = make_scp(gpu, scene["src"], scene["tgt"], CORR)
    assert status(s.align) == -4                                  # no features at all
    s.setSourceFeatures(scene["fs"])
    assert status(s.align) == -4                                  # no target features
    s.setTargetFeatures(scene["ft"][:-1])
    assert status(s.align) == -4                                  # feature count != point count
    s.setTargetFeatures(scene["ft"])
    s.setSourceFeatures(scene["fs"][:-1])
    assert status(s.align) == -4
    s.setSourceFeatures(scene["fs"])
    s.setMaximumIterations(5)
    s.align()                                                     # complete: it runs
    for setter, bad in ((s.setInlierFraction, -0.1), (s.setInlierFraction, 1.5), (s.setSimilarityThreshold, 1.0),
                        (s.setSimilarityThreshold, -0.5), (s.setCorrespondenceRandomness, 0), (s.setCorrespondenceRandomness, -2),
                        (s.setCorrespondenceRandomness, 33), (s.setNumberOfSamples, len(scene["src"]) + 1),
                        (s.setNumberOfSamples, 9), (s.setNumberOfSamples, 0)):
        p = pcl_amd._lib.ScpParams.from_buffer_copy(s.p)
        setter(bad)
        assert status(s.align) == -1, (setter.__name__, bad)
        s.p = p
    s.align()
    tiny = make_scp(gpu, scene["src"][:2], scene["tgt"], CORR, scene["fs"][:2], scene["ft"])
    tiny.setMaximumIterations(3)
    assert status(tiny.align) == -1                               # 3 samples from 2 points
    tiny.setNumberOfSamples(2)
    tiny.align()
    nanf = make_scp(gpu, scene["src"], scene["tgt"], CORR, scene["fs"], np.full_like(scene["ft"], np.nan))
    assert status(nanf.align) == -4                               # no finite target row


def test_fitness_score_forwards(gpu, scene):
    s = run_align(gpu, scene, 0, guess=T_GT)
    score = s.getFitnessScore()
    d2 = sr.nearest_d2(sr.transform_se3(T_GT, scene["src"]), scene["tgt"]).astype(np.float64)
    assert abs(score - d2.mean()) <= 1e-6 * d2.mean()
    assert all(ms >= 0 for ms in s.lastMs())


# ---- the reference test's criterion ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bunny_on_device(gpu):
    import pcl_amd
    src, tgt, _ = sr.load_bunny_pair()
    feats = []
    for c in (src, tgt):
        tree = pcl_amd.KdTree(gpu)
        tree.setInputCloud(c)
        ne = pcl_amd.NormalEstimation(gpu)
        ne.setInputCloud(c)
        ne.setSearchMethod(tree)
        ne.setKSearch(10)
        ne.compute()
        f = pcl_amd.FPFHEstimation(gpu)
        f.setInputCloud(c)
        f.setSearchMethod(tree)
        f.setRadiusSearch(0.05)
        feats.append(f.compute())
    return src, tgt, feats[0], feats[1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bunny_criterion_of_the_reference_test(gpu, bunny_on_device, seed):
    src, tgt, fs, ft = bunny_on_device
    assert np.isfinite(fs).all() and np.isfinite(ft).all()
    s = make_scp(gpu, src, tgt, 0.1, fs, ft)  # the defaults: 5,000 iterations, 3 samples, similarity 0.6, randomness 2
    assert (s.getMaximumIterations(), s.getNumberOfSamples(), s.getCorrespondenceRandomness()) == (5000, 3, 2)
    assert s.getSimilarityThreshold() == np.float32(0.6) and s.getInlierFraction() == 0.0
    s.setSeed(seed)
    out = s.align(want_output=True)
    assert s.hasConverged() and len(out) == len(src)
    assert np.float32(len(s.getInliers())) / np.float32(len(src)) > np.float32(0.95)
    inl, _, _ = sr.get_fitness(src, tgt, s.getFinalTransformation(), 0.1)
    assert np.array_equal(s.getInliers(), inl)
