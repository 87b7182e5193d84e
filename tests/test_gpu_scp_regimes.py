"""pclhip_feature_knn / pclhip_scp_* off the path of tests/test_gpu_scp.py (at most 3 shares of 1,000 target rows, fresh
objects, finite points, 2 to 4 samples, 44-leaf targets): 16 shares of the target rows with empty and nearly empty ones
and ties across them, the feature-neighbour cache of ONE object across calls with other seeds, other k and new inputs,
non-finite source and target POINTS, 1 and 8 samples, coincident matches (sigma == 0), a transform holding a NaN, a trace
shorter than the run, and a target with three box levels.

The bars are those of tests/test_gpu_scp.py (check_trace, check_scores, T_TOL): k-NN bit for bit, inlier counts exact,
errors within (count + 4) * 2^-24 relative, T within 1e-5 under the thick-triangle rule."""
import numpy as np
import pytest

import scp_restatement as sr
from test_gpu_scp import CORR, FLT_MAX, T_GT, bits, check_scores, check_trace, make_scp, rigid, run_align, surface, winner_of
from test_gpu_scp import scene  # noqa: F401  (the module-scoped fixture: the same 190 source and 260 target points)

pytestmark = pytest.mark.gpu
DEFAULT_DISTANCE = np.sqrt(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


# ---- feature k-NN: 16 shares -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,nq,k,D", [(4160, 1, 32, 33), (4160, 64, 32, 33), (4097, 3, 8, 64), (8191, 5, 1, 33), (4160, 2, 32, 7)])
def test_feature_knn_sixteen_shares(gpu, nt, nq, k, D):
    """At most one wave of queries: the target rows are cut into 16 shares (pcl_amd/csrc/scp.hpp, feature_knn_splits: 16 x
    the CUs' number of blocks wanted, no share below 256 rows, 16 at the most).  nt = 4160 and 4097: shares of 320 rows,
    the last three empty; nt = 8191: 16 shares of 512, the last one a row short.  Rows 320..639 (all of share 1 at
    nt = 4160) are NaN but row 330: a share with one candidate where k = 32.  Rows 5, 700 and 4000 are one row and the
    first query is that row: a tie across three shares, the lower index first.  The last query is the last target row:
    its nearest neighbour sits at the end of the last share that holds rows."""
    import pcl_amd
    rng = np.random.default_rng(nt + 7 * nq + k)
    t = rng.random((nt, D), dtype=np.float32)
    q = rng.random((nq, D), dtype=np.float32)
    t[320:640] = np.nan
    t[330] = rng.random(D, dtype=np.float32)
    t[700] = t[4000] = t[5]
    q[nq - 1] = t[nt - 1]
    q[0] = t[5]
    idx, d2, cnt = pcl_amd.featureKSearch(gpu, t, q, k)
    ridx, rd2, rcnt = sr.feature_knn(t, q, k)
    assert (rcnt == k).all()
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(d2), bits(rd2))
    ties = [5, 700, 4000][:k]
    assert list(idx[0, :len(ties)]) == ties and (d2[0, :len(ties)] == 0).all()
    if nq > 1:
        assert idx[nq - 1, 0] == nt - 1 and d2[nq - 1, 0] == 0
    assert ((idx < 320) | (idx >= 640) | (idx == 330)).all()
    # the lone candidate of its share is found where it belongs: ask for it
    idx1, d21, _ = pcl_amd.featureKSearch(gpu, t, t[330:331], k)
    assert idx1[0, 0] == 330 and d21[0, 0] == 0


# ---- one object, many calls ----------------------------------------------------------------------------------------------------
def word(x):
    return int(bits(x).ravel()[0])


def snapshot(s):
    r = s.result
    return dict(best=r.best_iteration, error=word(r.best_error), T=bits(s.getFinalTransformation()).tolist(),
                inliers=s.getInliers().tolist(), rejected=r.rejected, converged=bool(r.converged), count=r.best_count,
                trace=[(t["iteration"], t["samples"], t["matches"], t["rejected"], t["inliers"], word(t["error"]),
                        bits(t["transformation"]).tolist()) for t in s.trace])


def test_one_object_many_calls(gpu, scene):
    """The feature-neighbour cache (have / need / nn_idx, k_cached): a call searches the rows its draws name that no call
    searched since the cache was last dropped (another k, new features, a new source), and every call gives what a fresh
    object gives."""
    src, tgt, fs, ft = scene["src"], scene["tgt"], scene["fs"], scene["ft"]
    n = len(src)
    inputs = dict(src=src, tgt=tgt, fs=fs, ft=ft)
    s = make_scp(gpu, src, tgt, CORR, fs, ft)
    s.setSimilarityThreshold(0.8)
    s.setInlierFraction(0.0)
    s.setNumberOfSamples(3)
    seen = set()
    cached_k = None
    searched = []
    scored = 0

    def call(iters, k, seed, trace_capacity=None):
        nonlocal seen, cached_k
        s.setMaximumIterations(iters)
        s.setCorrespondenceRandomness(k)
        s.setSeed(seed)
        s.align(trace_capacity=iters if trace_capacity is None else trace_capacity)
        if cached_k != k:
            seen, cached_k = set(), k
        drawn = {row for it in range(iters) for row in sr.select_samples(seed, it, 3, n)}
        assert s.result.knn_rows == len(drawn - seen), (s.result.knn_rows, len(drawn - seen))
        searched.append(len(drawn - seen))
        seen |= drawn
        fresh = run_align(gpu, inputs, iters, ns=3, k=k, sim=0.8, frac=0.0, seed=seed)
        return snapshot(s), snapshot(fresh)

    for iters, k, seed in ((20, 3, 1), (60, 3, 2), (60, 3, 2), (40, 5, 2), (40, 2, 9), (40, 1, 9)):
        got, want = call(iters, k, seed)
        assert got == want, (iters, k, seed)
        assert len(got["trace"]) == iters
        scored += sum(t[3] == 0 for t in got["trace"])
    assert scored > 0  # hypotheses were scored
    assert searched == [48, 90, 0, 90, 86, 86]  # a partly warm cache, a warm one, and three cold ones
    # new inputs under a warm cache: each drops it
    for setter, key, value in ((s.setTargetFeatures, "ft", np.ascontiguousarray(ft[::-1])),
                               (s.setSourceFeatures, "fs", np.ascontiguousarray(fs[::-1])),
                               (s.setInputSource, "src", np.ascontiguousarray(src[::-1]))):
        setter(value)
        inputs[key] = value
        seen, cached_k = set(), None
        got, want = call(40, 1, 9)
        assert got == want, key
        assert searched[-1] == 86
    # a trace shorter than the run, batches that do not divide it: records 0..9, the same result
    full = snapshot(s)
    s.setBatchSize(7)
    got, _ = call(40, 1, 9, trace_capacity=10)
    assert searched[-1] == 0
    assert s.result.trace_count == 10 and [t[0] for t in got["trace"]] == list(range(10))
    assert got["trace"] == full["trace"][:10]
    assert {key: v for key, v in got.items() if key != "trace"} == {key: v for key, v in full.items() if key != "trace"}


# ---- non-finite points -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def holed(scene):
    sc = dict(scene)
    sc["src"] = scene["src"].copy()
    sc["src"][::4, 1] = np.nan
    sc["tgt"] = scene["tgt"].copy()
    sc["tgt"][::6, 2] = np.inf
    return sc


@pytest.mark.parametrize("ns,k", [(3, 3), (1, 2), (8, 2)])
def test_align_non_finite_points(gpu, holed, ns, k):
    """A quarter of the source points and a sixth of the target points are not finite.  A match that is a dropped target
    record is kind 2 (tgt_rank == NO_INDEX); a NaN source point fails the polygon test (kind 1) and is no inlier."""
    iters, sim, seed = 80, 0.5, 20 + ns
    s = run_align(gpu, holed, iters, ns=ns, k=k, sim=sim, frac=0.0, seed=seed)
    r, scored = check_trace(gpu, holed, s, iters, ns, k, sim, 0.0, seed)
    kinds = {d["rejected"] for d in s.trace}
    print("ns = %d: kinds %s, %d scored" % (ns, sorted(kinds), len(scored)))
    assert kinds == {w["rejected"] for w in r["trace"]}
    if ns == 3:
        assert kinds == {0, 1, 2}
    dropped = {m for d in s.trace for m in d["matches"] if m >= 0 and m % 6 == 0}
    assert dropped and all(d["rejected"] == 2 for d in s.trace if any(m in dropped for m in d["matches"]))
    best_it, lowest = winner_of(scored, len(holed["src"]), 0.0)
    assert s.result.best_iteration == best_it == r["best_iteration"]
    assert bits(s.result.best_error)[()] == bits(lowest)[()]
    if best_it >= 0:
        win = next(d for d in s.trace if d["iteration"] == best_it)
        inl, _, _ = sr.get_fitness(holed["src"], holed["tgt"], win["transformation"], CORR)
        assert np.array_equal(s.getInliers(), inl) and not np.isnan(holed["src"][inl]).any()


def test_align_eight_samples_scored(gpu, scene):
    """(With non-finite points and similarity 0.5 no hypothesis of 8 samples survives, and none of 1 sample ever does: its
    one edge has length 0 on both sides.)  The clean scene without pre-rejection: every hypothesis is scored, its T is
    umeyama of 8 pairs."""
    iters, seed = 40, 31
    s = run_align(gpu, scene, iters, ns=8, k=1, sim=0.0, frac=0.0, seed=seed)
    r, scored = check_trace(gpu, scene, s, iters, 8, 1, 0.0, 0.0, seed)
    assert len(scored) == iters and all(len(set(d["samples"])) == 8 for d in s.trace)
    best_it, lowest = winner_of(scored, len(scene["src"]), 0.0)
    assert s.result.best_iteration == best_it == r["best_iteration"] and bits(s.result.best_error)[()] == bits(lowest)[()]


def test_evaluate_non_finite_points_at_the_default_distance(gpu, holed):
    """the bound is +inf: every finite source point is an inlier, a NaN one is not"""
    src, tgt = holed["src"], holed["tgt"]
    s = make_scp(gpu, src, tgt, DEFAULT_DISTANCE)
    Ts = np.stack([np.eye(4, dtype=np.float32), T_GT])
    cnt, err = s.evaluate(Ts)
    finite = int(np.isfinite(src).all(axis=1).sum())
    assert finite == 142 and list(cnt) == [finite, finite]
    check_scores(src, tgt, Ts, DEFAULT_DISTANCE, cnt, err)


# ---- degenerate estimates -----------------------------------------------------------------------------------------------------------
def test_coincident_matches_give_the_identity_rotation(gpu, scene):
    """One finite target feature row: k = 3 is clamped to 1 and every sample matches target point 17.  The three target
    points coincide, sigma is 0, and umeyama's rotation is the identity (scp_rotation's sigma == 0 branch)."""
    sc = dict(scene)
    sc["ft"] = np.full_like(scene["ft"], np.nan)
    sc["ft"][17] = scene["ft"][17]
    iters, seed = 30, 4
    s = run_align(gpu, sc, iters, ns=3, k=3, sim=0.0, frac=0.0, seed=seed)
    check_trace(gpu, sc, s, iters, 3, 3, 0.0, 0.0, seed)
    assert len(s.trace) == iters and s.result.rejected == 0
    eye = bits(np.eye(3, dtype=np.float32))
    for d in s.trace:
        assert d["rejected"] == 0 and d["matches"] == [17, 17, 17]
        T = d["transformation"]
        assert np.array_equal(bits(T[:3, :3]), eye) and np.array_equal(bits(T[3]), bits(np.float32([0, 0, 0, 1])))
        want_t = sc["tgt"][17].astype(np.float64) - sc["src"][d["samples"]].astype(np.float64).mean(axis=0)
        assert np.abs(T[:3, 3] - want_t).max() <= 1e-6


def test_evaluate_a_transform_holding_a_nan(gpu, scene):
    s = make_scp(gpu, scene["src"], scene["tgt"], CORR)
    Ts = np.stack([T_GT, T_GT, T_GT, T_GT])
    Ts[1, 0, 3] = np.nan   # x of every moved point
    Ts[2, 2, 0] = np.nan   # z of every moved point
    cnt, err = s.evaluate(Ts)
    assert list(cnt[1:3]) == [0, 0] and (err[1:3] == FLT_MAX).all()
    assert cnt[0] == cnt[3] >= 150 and bits(err)[0] == bits(err)[3]  # its neighbours in the batch are not touched
    check_scores(scene["src"], scene["tgt"], Ts[[0, 3]], CORR, cnt[[0, 3]], err[[0, 3]])


# ---- a target with three box levels -----------------------------------------------------------------------------------------------
DEEP_N = 16 * 4096 + 16 * 37 + 5


def test_evaluate_on_a_deep_target(gpu, monkeypatch):
    """66,133 target points: 4,134 leaves, more than the 4,096 that two levels of boxes hold.  The brute force computes
    the nearest distances once per transform (they do not depend on the correspondence distance)."""
    tgt = surface(DEEP_N, 3)
    assert len(tgt) == DEEP_N
    rng = np.random.default_rng(8)
    src = (tgt[rng.permutation(DEEP_N)[:333]] + rng.normal(0, 0.01, (333, 3))).astype(np.float32)
    src[100] = np.nan
    Ts = np.stack([np.eye(4, dtype=np.float32), rigid(0, 0, 0, [0.9, 0, 0]), rigid(0, 0, 0, [1.98, 0, 0]),
                   rigid(0.05, -0.04, 0.3, [0.02, -0.01, 0.03]), rigid(0, 0, 0, [0, 0, 0.02])])
    memo = {}
    brute = sr.nearest_d2

    def nearest_once(moved, target):
        key = moved.tobytes()
        if key not in memo:
            memo[key] = brute(moved, target)
        return memo[key]

    monkeypatch.setattr(sr, "nearest_d2", nearest_once)
    s = make_scp(gpu, src, tgt, 0.01)
    counts = {}
    for corr in (0.01, 0.05, DEFAULT_DISTANCE):
        s.setMaxCorrespondenceDistance(corr)
        cnt, err = s.evaluate(Ts)
        check_scores(src, tgt, Ts, corr, cnt, err)
        cnt2, err2 = s.evaluate(Ts)
        assert np.array_equal(cnt, cnt2) and np.array_equal(bits(err), bits(err2))
        counts[corr] = list(map(int, cnt))
    assert len(memo) == 5
    print("deep target: inliers per transform %s" % counts)
    # the regimes: most points within 0.05 under the identity, fewer within 0.01; the far shift leaves the target's box
    assert counts[0.05][0] >= 300 > counts[0.01][0] > 0 and counts[0.05][2] < counts[0.05][1] < counts[0.05][0]
    assert counts[DEFAULT_DISTANCE] == [332] * 5
