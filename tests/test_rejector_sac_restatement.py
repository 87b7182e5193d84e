"""tests/rejector_sac_restatement.py pinned on the reference's own numbers (tests/golden/rejector_sac_bun.json: the data of
test/registration/test_registration_api_data.h:815-1131) and on its parts: the score in the stated float32 order keeps
exactly the reference's 97 pairs under the reference's transform, the replay is sac_restatement.Replay without skips, and
the attempts loop hands out the draw of the first good attempt."""
import json
import os

import numpy as np

import rejector_sac_restatement as rr
import sac_restatement as sacr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bunny_pairs():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    f = json.load(open(os.path.join(ROOT, "tests", "golden", "rejector_sac_bun.json")))
    z = np.load(os.path.join(ROOT, "tests", "golden", "bunny.npz"))
    src = np.ascontiguousarray(z["bun0"][:, :3], F)
    tgt = np.ascontiguousarray(z["bun4"][:, :3], F)
    co = np.array(g["correspondences_original"], np.int32)
    return src, tgt, co, f


def test_the_fixture_holds_the_reference_numbers():
    _, _, co, f = bunny_pairs()
    assert f["rej_sac_max_dist"] == 0.01 and f["rej_sac_max_iter"] == 1000
    sac = np.array(f["correspondences_sac"])
    assert sac.shape == (97, 2) and np.array(f["transform_from_SAC"]).shape == (4, 4)
    assert len(co) == 397 and (np.diff(co[:, 0]) > 0).all()
    assert f["transform_from_SAC"][3] == [0.0, 0.0, 0.0, 1.0]


def test_the_score_keeps_the_reference_pairs_under_the_reference_transform():
    src, tgt, co, f = bunny_pairs()
    T = np.array(f["transform_from_SAC"], F)
    thr = f["rej_sac_max_dist"]
    s, t = src[co[:, 0]], tgt[co[:, 1]]
    d2 = rr.pair_d2(T, s, t).astype(np.float64)
    gap = float(np.abs(d2 - thr * thr).min()) / (thr * thr)
    print("nearest pair: %.4g of threshold^2 away" % gap)
    assert gap > 1e-3  # no rounding choice can move a pair across (the transform is printed to six digits)
    keep = rr.within(T, s, t, thr)
    assert int(keep.sum()) == 97 == rr.count_within(T, s, t, thr)
    assert co[keep].tolist() == f["correspondences_sac"]  # exactly the 97 golden pairs, in order


def test_replay_is_the_plane_replay_without_skips():
    rng = np.random.default_rng(11)
    for case in range(300):
        n = int(rng.integers(3, 500))
        max_it = int(rng.integers(0, 60))
        prob = float(rng.choice([0.5, 0.9, 0.99, 0.999999]))
        a, b = rr.Replay(max_it, prob, n), sacr.Replay(max_it, prob, n)
        hi = int(rng.integers(1, n + 1))
        for _ in range(200):
            c = int(rng.integers(0, hi + 1))
            ra, rb = a.feed(c), b.feed(False, c)
            assert ra == rb and a.done == b.done
            assert (a.iterations, a.best, a.best_trial, a.trials, a.k) == (b.iterations, b.best, b.best_trial, b.trials, b.k)
            if not ra:
                break
        assert a.done and b.skipped == 0


def test_replay_stops_as_the_rule_says():
    r = rr.Replay(1000, 0.99, 100)
    assert r.feed(0) and r.k == rr.DBL_MAX and r.best_trial == -1       # a count of 0 is no model
    assert r.feed(50) and r.best_trial == 1                             # k = log(0.01) / log(1 - 1/8) = 34.5
    assert abs(r.k - np.log(0.01) / np.log(1 - 0.125)) < 1e-12
    assert r.feed(50) and r.best_trial == 1                             # strict: the earliest wins
    assert not r.feed(100) and r.best_trial == 3 and r.iterations == 4  # w = 1: clamped to DBL_EPSILON, k < 1
    r = rr.Replay(0, 0.99, 100)
    assert not r.feed(3) and r.iterations == 1                          # max_iterations 0: one trial


def test_draws_are_distinct_ascending_and_keyed():
    seen = set()
    for trial in range(40):
        for attempt in (0, 1, 999):
            for n in (3, 4, 397):
                s = rr.draw_samples(5, trial, attempt, n)
                assert len(s) == 3 and s[0] < s[1] < s[2] and 0 <= s[0] and s[2] < n
                seen.add((tuple(s), n))
    assert len({k for k in seen if k[1] == 397}) > 100  # the key separates trials and attempts
    assert rr.draw_samples(5, 3, 2, 397) == rr.draw_samples(5, 3, 2, 397) != rr.draw_samples(6, 3, 2, 397)


def test_attempts_loop_returns_the_draw_of_the_first_good_attempt():
    """a list whose first k draws of a trial are bad must give the draw of attempt k"""
    n, seed, trial = 40, 9, 2
    want_k = 3
    draws = [rr.draw_samples(seed, trial, a, n) for a in range(want_k + 1)]
    good = draws[want_k]
    bad_sets = draws[:want_k]
    assert all(len(set(b) & set(good)) < 3 for b in bad_sets)
    # every point sits at the origin except the three of the good draw, which span a wide triangle; each earlier draw then
    # holds at least one pair of coincident points (edge 0), and the threshold (from the covariance) is far below the triangle
    pts = np.zeros((n, 3), F)
    pts[good[0]] = (10, 0, 0)
    pts[good[1]] = (0, 10, 0)
    pts[good[2]] = (0, 0, 10)
    thresh = rr.sample_dist_thresh(pts)
    assert 0 < thresh < 100
    for b in bad_sets:
        assert not rr.is_sample_good(pts[b[0]], pts[b[1]], pts[b[2]], thresh)
    s, attempts, found = rr.get_samples(pts, seed, trial, thresh)
    assert found and attempts == want_k + 1 and s == good
    # no good sample at all: 1,000 attempts, not found
    s, attempts, found = rr.get_samples(np.zeros((n, 3), F), seed, trial, rr.sample_dist_thresh(np.zeros((n, 3), F)))
    assert not found and attempts == rr.MAX_SAMPLE_CHECKS


def test_sample_distance_threshold():
    rng = np.random.default_rng(3)
    p = (rng.normal(0, 1, (500, 3)) * (3.0, 2.0, 0.5) + (10, -4, 2)).astype(F)
    ev = np.linalg.eigvalsh(np.cov(p.astype(np.float64).T, bias=True))
    want = (np.sqrt(ev).sum() / 3.0) ** 2
    got = rr.sample_dist_thresh(p)
    assert abs(got - want) <= 1e-4 * want
    q = p.copy()
    q[7] = np.nan  # a non-finite point is left out of the moments
    ev = np.linalg.eigvalsh(np.cov(np.delete(p, 7, axis=0).astype(np.float64).T, bias=True))
    assert abs(rr.sample_dist_thresh(q) - (np.sqrt(ev).sum() / 3.0) ** 2) <= 1e-4 * want
    assert rr.sample_dist_thresh(np.zeros((5, 3), F)) == 0.0
    assert rr.sample_dist_thresh(np.full((5, 3), np.nan, F)) == 0.0


def test_result_rules_and_the_bunny_run():
    src, tgt, co, f = bunny_pairs()
    # fewer than 3 pairs: the list as it is, the identity
    r = rr.reject(src, tgt, co[:2, 0], co[:2, 1], threshold=0.01)
    assert not r["has_model"] and r["remaining"].tolist() == [0, 1] and np.array_equal(r["T"], np.eye(4, dtype=F))
    # a threshold no pair meets: no model
    r = rr.reject(src, tgt, co[:, 0], co[:, 1], threshold=0.0, max_iterations=5)
    assert not r["has_model"] and len(r["remaining"]) == 397 and r["best_trial"] == -1 and r["iterations"] == 6
    # the reference's settings: the remaining list is the score of the returned T, a subset in order
    r = rr.reject(src, tgt, co[:, 0], co[:, 1], threshold=0.01, max_iterations=1000, seed=0)
    assert r["has_model"] and 3 <= len(r["remaining"]) == r["best_count"]
    assert (np.diff(r["remaining"]) > 0).all()
    keep = rr.within(r["T"], src[co[:, 0]], tgt[co[:, 1]], 0.01)
    assert np.array_equal(np.nonzero(keep)[0], r["remaining"])
    assert r["trace"][r["best_trial"]]["count"] == r["best_count"]
    assert all(t["attempts"] >= 1 for t in r["trace"]) and max(t["attempts"] for t in r["trace"]) > 1
    # given transforms replace the restatement's own
    r2 = rr.reject(src, tgt, co[:, 0], co[:, 1], threshold=0.01, max_iterations=1000, seed=0,
                   transforms={i: t["T"] for i, t in enumerate(r["trace"])})
    assert np.array_equal(r2["remaining"], r["remaining"]) and r2["iterations"] == r["iterations"]


def test_float_bound_agrees_with_within_on_the_floats_around_it():
    """rsac_float_bound restated: double(d2) < threshold * threshold  <=>  d2 <= float_bound(threshold), on the bound, on the
    floats either side of it and on 0, the denormals, FLT_MAX and inf"""
    top = np.finfo(F).max
    zero3 = np.zeros((1, 3), F)
    for thr in (0.0, 1e-30, 1e-20, 0.01, 0.25, 1e19, 1e30):
        b = rr.float_bound(thr)
        t2 = float(thr) * float(thr)
        around = [b]
        with np.errstate(all="ignore"):
            for _ in range(3):
                around = [np.nextafter(around[0], F(-np.inf))] + around + [np.nextafter(around[-1], F(np.inf))]
            for d2 in around + [F(0), F(1e-45), np.finfo(F).tiny, top, F(np.inf)]:
                assert (float(d2) < t2) == bool(d2 <= b), (thr, d2)
            assert float(b) < t2 or thr == 0.0
            assert float(np.nextafter(b, F(np.inf))) >= t2 or b == top
        # ... and through within(): a pair at distance sqrt(d2) along x under the identity, for the d2 that are float squares
        for root in (F(np.sqrt(b)) if b > 0 else F(0), F(thr) if thr < 1e19 else F(1e19)):
            with np.errstate(all="ignore"):
                d2 = F(root * root)
                got = bool(rr.within(np.eye(4, dtype=F), zero3, np.array([[root, 0, 0]], F), thr)[0])
            assert got == bool(d2 <= b) == (float(d2) < t2), (thr, root)
    assert rr.float_bound(0.0) == F(-1e-45) and rr.float_bound(1e-30) == 0 and rr.float_bound(1e30) == top
    assert np.isnan(rr.float_bound(float("nan")))


def test_thresholds_around_a_float():
    for v in (F(0.0625), F(1e-4), F(2.0 ** -140), np.finfo(F).max, F(0.0), F(1e-45), F(3.0), F(0.01) * F(0.01)):
        lo, hi = rr.thresholds_around(v)
        assert lo * lo <= float(v) < hi * hi and np.nextafter(lo, np.inf) == hi
        if v > 0:
            assert rr.float_bound(hi) == v and rr.float_bound(lo) == np.nextafter(v, F(-np.inf))
    assert rr.thresholds_around(F(0.0625))[0] == 0.25 and rr.thresholds_around(F(4.0))[0] == 2.0


def test_the_wrong_kernels_differ_from_the_contract_on_the_dense_scene():
    """the contracted and the reordered d2 are what tests/test_gpu_rejector_sac_regimes.py must be able to tell from the
    stated one: on its scene they move pairs across threshold^2, elsewhere they stay within a few ulps of it"""
    from test_gpu_rejector_sac_regimes import dense_scene
    for thr in (0.02, 0.05, 0.25):
        src, tgt, q, m, Ts = dense_scene(thr)
        assert Ts.shape == (70, 4, 4) and len({T.tobytes() for T in Ts}) == 70 and np.abs(Ts - Ts[0]).max() < 1e-5
        d2 = rr.pair_d2(Ts[0], src, tgt)
        for wrong in (rr.pair_d2_contracted, rr.pair_d2_reordered):
            w = wrong(Ts[0], src, tgt)
            assert (w != d2).any() and np.abs(w.astype(np.float64) - d2).max() <= 1e-4 * thr * thr
            flipped = (w.astype(np.float64) < thr * thr) != (d2.astype(np.float64) < thr * thr)
            print("threshold %g, %s: %d of %d pairs change sides under T" % (thr, wrong.__name__, int(flipped.sum()), len(q)))
        want = rr.counts_with(rr.pair_d2, Ts, src, tgt, thr)
        assert want.tolist() == [rr.count_within(T, src, tgt, thr) for T in Ts]
        assert (rr.counts_with(rr.pair_d2_contracted, Ts, src, tgt, thr) != want).any()
        assert (rr.counts_with(rr.pair_d2_reordered, Ts, src, tgt, thr) != want).any()
    # exact products and sums: nothing to contract, nothing to reorder
    s = np.array([[1, 2, 3], [0.5, -4, 8]], F)
    t = np.array([[2, 2, 2], [1, 1, 1]], F)
    I = np.eye(4, dtype=F)
    assert rr.pair_d2(I, s, t).tolist() == rr.pair_d2_contracted(I, s, t).tolist() == rr.pair_d2_reordered(I, s, t).tolist() \
        == [2.0, 74.25]
