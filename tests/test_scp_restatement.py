"""The numpy restatement of SampleConsensusPrerejective (tests/scp_restatement.py) pinned on what the reference lets one pin:
the selectSamples insertion rule (impl/sample_consensus_prerejective.hpp:96-117) on hand-written draws, thresholdEdgeLength
(correspondence_rejection_poly.h:320-338) at, just under and just over the threshold, and end to end the criterion of the
reference's own test (test/registration/test_sac_ia.cpp:140-209): bun0 moved by (100, 0, 0) and 90 degrees about z against
bun4, correspondence distance 0.1, 5,000 iterations, similarity 0.6, randomness 2 -> more than 95 % inliers.  The features
are the project's FPFH at r = 0.05 on k = 10 normals (the test's normal radius of 0.005 is under bun0's point spacing: no
finite normal, which the project's FPFH turns into NaN rows)."""
import numpy as np
import pytest

import fpfh_restatement as fr
import scp_restatement as sr

SEEDS = (1, 2, 3)


def test_draw_function_is_splitmix64():
    # seed 0, iteration 0, slot 0: the state is the golden-ratio increment, the output splitmix64's first for seed 0
    assert sr.draw_bits(0, 0, 0) == 0xE220A8397B1DCDAF
    assert sr.draw_bits(0, 0, 1) == 0x6E789E6AA1B965F4  # ... its second: the counter advanced by one
    assert sr.draw_bits(5, 3, 2) != sr.draw_bits(5, 2, 3)
    for n in (1, 2, 7, 397, 100000):
        v = [sr.draw_index(11, it, s, n) for it in range(50) for s in range(6)]
        assert min(v) >= 0 and max(v) < n
    v = np.array([sr.draw_index(3, it, 0, 10) for it in range(20000)])
    assert np.abs(np.bincount(v, minlength=10) / 20000.0 - 0.1).max() < 0.01


def test_select_samples_insertion_rule():
    # hand-written draws: draw j picks among the n - j indices not yet taken, counted in ascending order
    assert sr.insert_samples([5]) == [5]
    assert sr.insert_samples([5, 5, 5]) == [5, 6, 7]      # moved up past every earlier pick it reaches
    assert sr.insert_samples([5, 2, 3]) == [2, 4, 5]      # 2 goes in front; 3 -> 4 past the 2, in front of the 5
    assert sr.insert_samples([0, 0, 0, 0]) == [0, 1, 2, 3]
    assert sr.insert_samples([9, 0, 7]) == [0, 8, 9]      # 7 -> 8 past the 0, then in front of the 9
    assert sr.insert_samples([3, 3, 0, 1]) == [0, 2, 3, 4]
    rng = np.random.default_rng(0)
    for _ in range(300):
        n, c = int(rng.integers(1, 12)), 0
        c = int(rng.integers(1, min(n, 8) + 1))
        draws = [int(rng.integers(0, n - j)) for j in range(c)]
        s = sr.insert_samples(draws)
        free = list(range(n))
        want = []
        for d in draws:
            want.append(free.pop(d))
        assert s == sorted(want) and len(set(s)) == c and s[0] >= 0 and s[-1] < n
    for it in range(100):
        s = sr.select_samples(7, it, 3, 4)
        assert s == sorted(set(s)) and len(s) == 3 and s[-1] < 4


def test_threshold_edge_length_at_the_threshold():
    thr = np.float32(0.6)
    simsq = np.float32(thr * thr)
    one = np.float32(1.0)
    assert sr.edge_similar(simsq, one, simsq)                                   # at: kept (>=)
    assert not sr.edge_similar(np.nextafter(simsq, np.float32(0)), one, simsq)  # just under
    assert sr.edge_similar(np.nextafter(simsq, one), one, simsq)                # just over
    assert sr.edge_similar(one, simsq, simsq)                                   # the ratio is min / max either way
    assert not sr.edge_similar(np.float32(0), np.float32(0), simsq)             # 0 / 0: NaN, rejected
    # through the points: similarity 0.5 -> 0.25 on the squared lengths, exact in float32
    tgt = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    half = np.float32(0.5)
    for x, keep in ((half, True), (np.nextafter(half, np.float32(0)), False), (np.nextafter(half, one), True)):
        src = np.array([[0, 0, 0], [x, 0, 0]], np.float32)
        assert sr.threshold_polygon(src, tgt, 0.5) is keep
    # a triangle has three edges, the last one closes it; two points have ONE edge
    tri_t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    tri_s = np.array([[0, 0, 0], [1, 0, 0], [0, 0.4, 0]], np.float32)  # edge 2 -> 0: 0.16 < 0.25
    assert sr.threshold_polygon(tri_s[:2], tri_t[:2], 0.5)
    assert not sr.threshold_polygon(tri_s, tri_t, 0.5)
    assert sr.threshold_polygon(tri_s, tri_t, 0.3)


def test_feature_knn_ties_and_non_finite_rows():
    t = np.zeros((6, 33), np.float32)
    t[:, 0] = [3, 1, 1, np.nan, 2, 1]
    q = np.zeros((2, 33), np.float32)
    q[1, 5] = np.inf
    idx, d2, cnt = sr.feature_knn(t, q, 4)
    assert idx[0].tolist() == [1, 2, 5, 4] and d2[0].tolist() == [1, 1, 1, 4] and cnt[0] == 4  # ties: the lower index
    assert cnt[1] == 0 and idx[1].tolist() == [-1] * 4
    idx, d2, cnt = sr.feature_knn(t, q[:1], 8)
    assert cnt[0] == 5 and idx[0, :5].tolist() == [1, 2, 5, 4, 0] and idx[0, 5] == -1 and np.isinf(d2[0, 5])


def test_umeyama_and_fitness():
    rng = np.random.default_rng(1)
    s = rng.random((4, 3))
    a = 0.7
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    d = s @ R.T + [1, 2, 3]
    T = sr.umeyama(s, d)
    assert np.abs(T[:3, :3] - R).max() < 1e-12 and np.abs(T[:3, 3] - [1, 2, 3]).max() < 1e-12
    # strict bound: a point at exactly d2 == float(corr_dist^2) is no inlier
    inl, err, _ = sr.get_fitness(np.array([[0.5, 0, 0]], np.float32), np.zeros((1, 3), np.float32), np.eye(4), 0.5)
    assert len(inl) == 0 and err == sr.FLT_MAX
    inl, err, _ = sr.get_fitness(np.array([[0.25, 0, 0]], np.float32), np.zeros((1, 3), np.float32), np.eye(4), 0.5)
    assert inl.tolist() == [0] and err == np.float32(0.0625)
    assert sr.is_identity_guess(np.eye(4)) and not sr.is_identity_guess(T)


@pytest.fixture(scope="module")
def bunny_features():
    from oracle import pcl_oracle as orc
    src, tgt, _ = sr.load_bunny_pair()
    out = []
    for c in (src, tgt):
        nrm, _ = orc.KdTree(c).normals(c, 10)
        out.append(fr.restate(c, nrm[:, :3], 0.05)["fpfh32"])
    return src, tgt, out[0], out[1]


@pytest.mark.parametrize("seed", SEEDS)
def test_bunny_criterion_of_the_reference_test(bunny_features, seed):
    src, tgt, fs, ft = bunny_features
    assert np.isfinite(fs).all() and np.isfinite(ft).all()
    r = sr.align(src, tgt, fs, ft, max_iterations=5000, nr_samples=3, k=2, similarity=0.6, corr_dist=0.1, seed=seed)
    assert r["converged"]
    assert np.float32(len(r["inliers"])) / np.float32(len(src)) > np.float32(0.95)
    # the winner is the first minimum of the trace under the acceptance rule
    scored = [t for t in r["trace"] if not t["rejected"]]
    best = min(scored, key=lambda t: (t["error"], t["iteration"]))
    assert best["iteration"] == r["best_iteration"] and best["error"] == r["lowest_error"]
    assert r["rejected"] == 5000 - len(scored)
