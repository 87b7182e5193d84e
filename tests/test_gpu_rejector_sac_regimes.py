"""CorrespondenceRejectorSampleConsensus off its easy path: the inlier bound one double either side of a float, thousands of
pairs AT the bound against a kernel that contracts or reorders its sums, selection against count at the bound, every
hypotheses-per-pass edge, the device's whole grid, degenerate and far-away sources, the chain on a source subset, before and
after other rejectors and on lists of 0 and 2 pairs, device-memory inputs.  tests/test_gpu_rejector_sac.py keeps every scored
pair 1e-6 away from threshold^2; here the pairs sit on it, and the comparisons are exact all the same: include/pclhip.h
fixes the float expression ("in float without contraction ... counting and selecting use this one expression"), so the
numpy restatement (tests/rejector_sac_restatement.py) has to be met to the bit.  Whatever a case needs from its scene (pairs
within 1e-7 of the bound, variants that would differ, a NaN under permutation, a tie) is asserted on the CPU before the
first device call."""
import ctypes as C

import numpy as np
import pytest

import rejector_sac_restatement as rr
from test_gpu_rejector_sac import TILE, bits, bun, check_against_restatement, gpu, make, rigid, run_twice, scene  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
I4 = np.eye(4, dtype=F)
FLT_MAX = np.finfo(F).max
SCENE_T = rigid(0.3, -0.2, 0.5, (0.4, -0.3, 0.2))  # the transform of scene()


def as_float(b):
    return np.array([b], np.uint32).view(F)[0]


def word(x):
    return int(F(x).view(np.uint32))


def ulps_from(v, k):
    """the float k steps above (below) the positive float v; past the largest finite float: inf"""
    return as_float(word(v) + k) if word(v) + k <= word(FLT_MAX) else F(np.inf)


def paired(src, seed, mismatched=0.3, noise=0.002):
    """scene()'s target and list for a given source cloud"""
    rng = np.random.default_rng(seed)
    n = len(src)
    order = rng.permutation(n)
    tgt = np.empty((n, 3), F)
    tgt[order] = (src.astype(np.float64) @ SCENE_T[:3, :3].T + SCENE_T[:3, 3] + rng.normal(0, noise, (n, 3))).astype(F)
    m = order.astype(np.int32)
    bad = rng.random(n) < mismatched
    m[bad] = rng.integers(0, n, int(bad.sum()))
    return tgt, np.arange(n, dtype=np.int32), m


# ---- a. the inlier bound, one double either side ---------------------------------------------------------------------------------
def target_with_d2(w, axis, sign):
    """a target point t whose pair (0, t) has d2 == w exactly under the identity (p = 0, e = -t): the largest float a with
    fl(a a) <= w on `axis`, and the square root of what is missing on the next axis; w = inf: a component that overflows"""
    t = np.zeros(3, F)
    if not np.isfinite(w):
        t[axis] = sign * F(3e19)
        return t
    lo, hi = 0, word(np.inf)  # fl(lo lo) <= w < fl(hi hi)
    with np.errstate(all="ignore"):
        while hi - lo > 1:
            mid = (lo + hi) // 2
            a = as_float(mid)
            lo, hi = (mid, hi) if F(a * a) <= w else (lo, mid)
        for back in range(64):
            a = as_float(lo - back)
            rest = float(w) - float(F(a * a))
            t[:] = 0
            t[axis], t[(axis + 1) % 3] = sign * a, F(np.sqrt(rest))
            if rr.pair_d2(I4, np.zeros((1, 3), F), t[None])[0] == w:
                return t
    raise AssertionError("no target point with d2 == %r" % w)


def bound_pairs(v):
    """21 pairs whose d2 are the floats v - 3 ulp .. v + 3 ulp, three of each: the offset moves between x, y and z, the sign
    alternates -> (source (all zero), target, d2)"""
    want, pts = [], []
    for k in range(-3, 4):
        for axis in range(3):
            w = ulps_from(v, k)
            want.append(w)
            pts.append(target_with_d2(w, axis, -1.0 if (k + axis) % 2 else 1.0))
    tgt = np.ascontiguousarray(pts, F)
    return np.zeros_like(tgt), tgt, np.array(want, F)


BOUND_VALUES = {"tie": F(0.0625), "1e-4": F(1e-4), "denormal": F(2.0 ** -140), "flt_max": FLT_MAX}


@pytest.mark.parametrize("name", list(BOUND_VALUES))
def test_the_inlier_bound_one_double_either_side(gpu, name):
    v = BOUND_VALUES[name]
    src, tgt, want = bound_pairs(v)
    n = len(src)
    q = np.arange(n, dtype=np.int32)
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(rr.pair_d2(I4, src, tgt)), bits(want))      # the scene is what it claims to be
    t_lo, t_hi = rr.thresholds_around(v)
    assert t_lo * t_lo <= float(v) < t_hi * t_hi and np.nextafter(t_lo, np.inf) == t_hi
    at_v = int((want == v).sum())
    assert at_v == 3
    counts = {thr: rr.count_within(I4, src, tgt, thr) for thr in (t_lo, t_hi)}
    assert counts[t_hi] - counts[t_lo] == at_v == int((want <= v).sum()) - int((want < v).sum())
    assert rr.float_bound(t_lo) == ulps_from(v, -1) and rr.float_bound(t_hi) == v
    if name == "tie":
        assert t_lo == 0.25 and t_lo * t_lo == float(v)                         # the strict `<` on an exact tie
    if name == "denormal":
        assert 0 < float(v) < np.finfo(F).tiny and float(F(2.0 ** -70) * F(2.0 ** -70)) == float(v)
    if name == "flt_max":
        assert t_hi * t_hi > float(FLT_MAX) and int(np.isinf(want).sum()) == 9  # every finite d2 inside, no overflowed one
        assert counts[t_hi] == int(np.isfinite(want).sum()) == 12
    for thr in (t_lo, t_hi):
        r = make(gpu, src, tgt, thr)
        for _ in range(2):
            assert r.evaluate(I4[None], q, q).tolist() == [counts[thr]], (name, thr)


def test_threshold_zero_counts_no_coincident_pair(gpu):
    """d2 == 0 everywhere: the bound is the negative denormal under threshold 0 (0 < 0 is false) and 0 under 1e-30 (whose
    square, 1e-60, is far below the least float) -- a compare that flushed denormals would take both for 0"""
    src = scene(500, 3)[0]
    n = len(src)
    q = np.arange(n, dtype=np.int32)
    assert not rr.pair_d2(I4, src, src).any()  # p = s exactly under the identity
    assert word(rr.float_bound(0.0)) == 0x80000001 and word(rr.float_bound(1e-30)) == 0
    assert rr.count_within(I4, src, src, 0.0) == 0 and rr.count_within(I4, src, src, 1e-30) == n
    for thr, want in ((0.0, 0), (1e-30, n)):
        assert make(gpu, src, src, thr).evaluate(I4[None], q, q).tolist() == [want]


# ---- b. dense pairs at the bound against a contracted kernel -----------------------------------------------------------------------
DENSE_SEED = 1


def dense_scene(thr, seed=DENSE_SEED):
    """scene() without mismatches, every target point at distance thr from the image of its source point, and 70 transforms:
    the scene's own and 69 copies whose twelve entries are moved by up to 3 float ulps"""
    n = 2 * TILE + 77
    src = scene(n, seed, mismatched=0.0)[0]
    rng = np.random.default_rng(1000 + seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    tgt = (src.astype(np.float64) @ SCENE_T[:3, :3].T + SCENE_T[:3, 3] + u * thr).astype(F)
    Ts = np.repeat(SCENE_T.astype(F)[None], 70, axis=0)
    rows = Ts[1:, :3, :].view(np.int32)
    rows += rng.integers(-3, 4, rows.shape, dtype=np.int32)
    q = np.arange(n, dtype=np.int32)
    return src, tgt, q, q.copy(), Ts


@pytest.mark.parametrize("thr", [0.02, 0.05, 0.25])
def test_dense_pairs_at_the_bound(gpu, thr):
    src, tgt, q, m, Ts = dense_scene(thr)
    t2 = thr * thr
    d2 = rr.pair_d2(Ts[0], src, tgt).astype(np.float64)
    near = int((np.abs(d2 - t2) <= 1e-7 * t2).sum())
    want = rr.counts_with(rr.pair_d2, Ts, src, tgt, thr)
    contracted = rr.counts_with(rr.pair_d2_contracted, Ts, src, tgt, thr)
    reordered = rr.counts_with(rr.pair_d2_reordered, Ts, src, tgt, thr)
    print("threshold %g: %d pairs within 1e-7 of threshold^2; of 70 counts a contracted kernel changes %d, a reordered %d"
          % (thr, near, int((contracted != want).sum()), int((reordered != want).sum())))
    assert near >= 20
    assert (contracted != want).any() and (reordered != want).any()  # the suite sees either mistake on this scene
    assert 0 < want.min() and want.max() < len(q)
    r = make(gpu, src, tgt, thr)
    for _ in range(2):
        assert np.array_equal(r.evaluate(Ts, q, m).astype(np.int64), want)


# ---- c. selection equals count at the bound --------------------------------------------------------------------------------------
def test_selection_equals_count_at_the_bound(gpu):
    """max_iterations = 0 consumes exactly trial 0, whose T0 does not depend on the inlier threshold: thresholds either
    side of the median pair's d2 under T0 select and count through the scalar and the packed expression at the bound"""
    src, tgt, q, m = scene(1000, 61, mismatched=0.3, noise=0.01)
    s, t = src[q], tgt[m]
    out = run_twice(make(gpu, src, tgt, 0.05, 0, 2), q, m)
    assert out[4]["trials"] == 1 and not out[5][0]["no_sample"]
    T0 = out[5][0]["transformation"]
    with np.errstate(all="ignore"):
        d2 = rr.pair_d2(T0, s, t)
    finite = np.sort(d2[np.isfinite(d2)])
    v = finite[len(finite) // 2]
    ties = np.nonzero(d2 == v)[0]
    t_lo, t_hi = rr.thresholds_around(v)
    kept = {}
    for thr in (t_lo, t_hi):
        r = make(gpu, src, tgt, thr, 0, 2)
        rq, rm, pos, T, st, trace = run_twice(r, q, m)
        assert np.array_equal(bits(trace[0]["transformation"]), bits(T0)) and np.array_equal(bits(T), bits(T0))
        want = np.nonzero(rr.within(T0, s, t, thr))[0]
        assert np.array_equal(pos, want) and st["has_model"]
        assert len(pos) == st["best_count"] == trace[0]["count"] == int(r.evaluate(T0[None])[0])
        assert np.array_equal(rq, q[pos]) and np.array_equal(rm, m[pos])
        kept[thr] = pos
    assert len(ties) >= 1 and np.array_equal(np.setdiff1d(kept[t_hi], kept[t_lo]), ties)
    assert len(np.setdiff1d(kept[t_lo], kept[t_hi])) == 0


# ---- d. hypotheses per pass ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def near_transforms():
    """2,049 rigid transforms near the scene's own over 300 pairs, and the restatement's counts (computed once)"""
    src, tgt, q, m = scene(300, 11)
    rng = np.random.default_rng(12)
    Ts = np.stack([rigid(*(np.array([0.3, -0.2, 0.5]) + rng.normal(0, 0.004, 3)),
                         np.array([0.4, -0.3, 0.2]) + rng.normal(0, 0.004, 3)) for _ in range(2049)]).astype(F)
    return src, tgt, q, m, Ts, rr.counts_with(rr.pair_d2, Ts, src[q], tgt[m], 0.02)


@pytest.mark.parametrize("H", [255, 256, 257, 1023, 1024, 1025, 2049])
def test_hypotheses_per_pass(gpu, near_transforms, H):
    src, tgt, q, m, Ts, want = near_transforms
    assert len(set(want.tolist())) > 20  # the counts tell the hypotheses apart
    cnt = make(gpu, src, tgt, 0.02).evaluate(Ts[:H], q, m)
    assert np.array_equal(cnt.astype(np.int64), want[:H])


def test_a_run_through_every_batch_size_of_the_schedule(gpu):
    """every pair mismatched: 2,101 trials, the schedule 16, 32, ..., 1024, 69 against one of 1024, 1024, 53"""
    src, tgt, q, m = scene(300, 5, mismatched=1.0)
    outs = []
    for batch in (0, 1024):
        r = make(gpu, src, tgt, 0.02, 2100, 2, batch)
        out = run_twice(r, q, m)
        assert out[4]["trials"] == 2101 == out[4]["iterations"] and len(out[5]) == 2101
        outs.append(out)
    check_against_restatement(r, src, tgt, q, m, 0.02, 2100, 2, outs[0])
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3])) and a[4] == b[4]
    assert [x["count"] for x in a[5]] == [y["count"] for y in b[5]]
    assert all(np.array_equal(bits(x["transformation"]), bits(y["transformation"])) for x, y in zip(a[5], b[5]))


# ---- e. the whole grid -----------------------------------------------------------------------------------------------------------------
def test_fullgrid(gpu):
    """A block of the scoring kernel takes 2,048 pairs per tile and a CU holds at most 8 blocks of 256 threads, so whatever
    occupancy the runtime reports, (8 * CUs + 3) tiles give some blocks a second tile; 17 more pairs leave the last tile
    ragged.  The list walks a scene of 100,003 pairs round and round (evaluate takes a query index twice): the restatement
    scores each pair once, and an odd period puts no two tiles on the same pairs."""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n, period = (8 * cus + 3) * TILE + 17, 100003
    src, tgt, q0, m0 = scene(period, 8)
    walk = np.arange(n) % period
    q, m = q0[walk], m0[walk]
    far = I4.copy()
    far[:3, 3] = 50
    Ts = np.stack([SCENE_T.astype(F), rigid(0.3, -0.2, 0.5, (0.4, -0.3, 0.22)).astype(F), I4, far])
    inside = np.stack([rr.within(T, src[q0], tgt[m0], 0.02) for T in Ts])
    want = (n // period) * inside.sum(axis=1) + inside[:, :n % period].sum(axis=1)
    print("fullgrid scene: %d CUs -> %d pairs, counts %s" % (cus, n, want.tolist()))
    assert 0.6 * n < want[0] < 0.8 * n and want[2] < want[1] < want[0] and want[3] == 0
    cnt = make(gpu, src, tgt, 0.02).evaluate(Ts, q, m)
    assert np.array_equal(cnt.astype(np.int64), want)


# ---- f. the sample distance threshold ----------------------------------------------------------------------------------------------
COLLINEAR_NAN_SEED = 2      # the restatement's eigenvalues go negative here, in every order of the points
COLLINEAR_FINITE_SEED = 1   # ... and stay at or above 0 here


def collinear(seed, n=200):
    rng = np.random.default_rng(seed)
    a, d = rng.uniform(-2, 2, 3), rng.normal(size=3)
    return (a + rng.uniform(-3, 3, n)[:, None] * (d / np.linalg.norm(d))).astype(F)


def rigid_copy(src):
    return (src.astype(np.float64) @ SCENE_T[:3, :3].T + SCENE_T[:3, 3]).astype(F)


def test_a_nan_sample_threshold_makes_every_sample_bad(gpu):
    src = collinear(COLLINEAR_NAN_SEED)
    n = len(src)
    rng = np.random.default_rng(5)
    with np.errstate(all="ignore"):
        assert np.isnan(rr.sample_dist_thresh(src))
        for _ in range(20):  # no order of the double sums decides it
            assert np.isnan(rr.sample_dist_thresh(src[rng.permutation(n)]))
    tgt = rigid_copy(src)
    q = np.arange(n, dtype=np.int32)
    own = rr.reject(src, tgt, q, q, 0.02, 1000, seed=0)
    assert own["no_sample"] and own["trials"] == 1 and not own["has_model"]
    r = make(gpu, src, tgt, 0.02, 1000, 0)
    for _ in range(2):  # (not run_twice: it compares the statistics with ==, and this threshold is not equal to itself)
        rq, rm = r.getRemainingCorrespondences(q, q)
        T, st, trace = r.getBestTransformation(), r.lastStats(), r.trace()
        assert np.isnan(st["sample_dist_thresh"]) and st["no_sample"] and st["trials"] == 1 and not st["has_model"]
        assert st["best_trial"] == -1 and st["best_count"] == 0 and st["n"] == n == st["remaining"]
        assert len(trace) == 1 and trace[0]["attempts"] == 1000 and trace[0]["no_sample"] and trace[0]["count"] == 0
        assert trace[0]["samples"] == own["trace"][0]["samples"]
        assert np.array_equal(rq, q) and np.array_equal(rm, q) and np.array_equal(bits(T), bits(I4))
        assert len(r.getInliersIndices()) == 0


def degenerate_source(kind):
    if kind == "collinear":
        return collinear(COLLINEAR_FINITE_SEED, 600)
    rng = np.random.default_rng(17)
    flat = np.column_stack([rng.random((600, 2)) * (2.0, 1.5) + (3.0, -1.0), np.zeros(600)])
    if kind == "tilted":
        flat = flat @ rigid(0.4, 0.3, 0.0, (0, 0, 0))[:3, :3].T + (0.0, 0.0, 0.5)
    return flat.astype(F)


@pytest.mark.parametrize("kind", ["collinear", "planar", "tilted"])
def test_degenerate_sources_with_a_finite_sample_threshold(gpu, kind):
    """one or two eigenvalues at 0: the threshold within the module's 1e-5, the trace and the counts as everywhere (the
    helper compares no T of a thin triangle, and a collinear source has no other)"""
    src = degenerate_source(kind)
    tgt, q, m = paired(src, 23)
    thresh = rr.sample_dist_thresh(src[q])
    assert np.isfinite(thresh) and thresh > 0
    if kind == "planar":
        assert not src[:, 2].any()
    r = make(gpu, src, tgt, 0.02, 300, 1)
    out = run_twice(r, q, m)
    ref = check_against_restatement(r, src, tgt, q, m, 0.02, 300, 1, out)
    assert ref["has_model"]


FAR_SHIFT = np.array([1e4, -2e4, 3e3])
FAR_THRESHOLD = 2.0 ** -7
FAR_SEED = 3


def test_far_from_the_origin(gpu):
    """both clouds moved by (1e4, -2e4, 3e3): the coordinates are multiples of 2^-10, 2^-9 and 2^-12 there, so d2 takes few
    values and some pair sits ON threshold^2 = 2^-14 (asserted) -- the `threshold` margin cannot hold and is off; what it
    stood for holds by contract.  The sample threshold is shifted by the list's first point and keeps its value."""
    near_src, near_tgt, q, m = scene(2500, FAR_SEED, noise=0.004)
    src = (near_src.astype(np.float64) + FAR_SHIFT).astype(F)
    tgt = (near_tgt.astype(np.float64) + FAR_SHIFT).astype(F)
    thr = FAR_THRESHOLD
    want_thresh = rr.sample_dist_thresh(near_src[q])
    assert abs(rr.sample_dist_thresh(src[q]) - want_thresh) <= 1e-5 * want_thresh
    own = rr.reject(src, tgt, q, m, thr, 1000, seed=4)
    edge = word(thr * thr)
    on_the_bound = 0
    for rec in own["trace"]:
        d2 = rr.pair_d2(rec["T"], src[q], tgt[m])
        d2 = d2[np.isfinite(d2) & (d2 > 0)]
        on_the_bound += int((np.abs(bits(d2).astype(np.int64) - edge) <= 1).sum())
    print("far scene: %d trials, %d scored pairs within 1 ulp of threshold^2" % (own["trials"], on_the_bound))
    assert on_the_bound >= 1
    r = make(gpu, src, tgt, thr, 1000, 4)
    out = run_twice(r, q, m)
    assert abs(out[4]["sample_dist_thresh"] - want_thresh) <= 1e-5 * want_thresh
    ref = check_against_restatement(r, src, tgt, q, m, thr, 1000, 4, out, margins=("k", "edge"))
    assert ref["has_model"] and 0.3 * len(q) < ref["best_count"] < 0.7 * len(q)  # 70 % matched, noise at half the threshold


def test_a_nan_first_source_point_shifts_by_nothing(gpu):
    src, tgt, q, m = scene(400, 33, mismatched=0.1)
    src[q[0]] = np.nan  # K = 0: the sums are taken about the origin
    r = make(gpu, src, tgt, 0.02, 200, 6)
    out = run_twice(r, q, m)
    ref = check_against_restatement(r, src, tgt, q, m, 0.02, 200, 6, out)
    assert ref["has_model"] and 0 not in out[2].tolist()


def test_a_list_in_random_order(gpu):
    src, tgt, q, m = scene(800, 35)
    perm = np.random.default_rng(36).permutation(len(q))
    q, m = np.ascontiguousarray(q[perm]), np.ascontiguousarray(m[perm])
    r = make(gpu, src, tgt, 0.02, 1000, 3)
    out = run_twice(r, q, m)
    ref = check_against_restatement(r, src, tgt, q, m, 0.02, 1000, 3, out)
    assert ref["has_model"] and (np.diff(out[2]) > 0).all() and np.array_equal(out[0], q[out[2]])


def test_a_perfect_scene_stops_after_its_first_trial(gpu):
    """every pair an inlier: w = 1, p_outliers clamped to DBL_EPSILON, k = log(0.01) / log(DBL_EPSILON) < 1"""
    src, tgt, q, m = scene(500, 37, mismatched=0.0, noise=0.0)
    r = make(gpu, src, tgt, 0.05, 1000, 0)
    out = run_twice(r, q, m)
    ref = check_against_restatement(r, src, tgt, q, m, 0.05, 1000, 0, out)
    st = out[4]
    assert st["trials"] == st["iterations"] == 1 and st["best_count"] == len(q) == st["remaining"] and ref["has_model"]
    assert np.array_equal(out[2], np.arange(len(q)))


# ---- g. the chain ------------------------------------------------------------------------------------------------------------------
def estimation(gpu, bun, indices=None):
    import pcl_amd
    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputTarget(bun["tgt"])
    ce.setInputSource(bun["src"])
    ce.setIndicesSource(indices)
    return ce


def distance_rejector(max_distance):
    import pcl_amd
    h = pcl_amd.CorrespondenceRejectorDistance()
    h.setMaximumDistance(max_distance)
    return h


def sac_rejector(gpu, seed, threshold=0.01, max_iterations=1000):
    import pcl_amd
    sac = pcl_amd.CorrespondenceRejectorSampleConsensus(gpu)
    sac.setInlierThreshold(threshold)
    sac.setMaximumIterations(max_iterations)
    sac.setSeed(seed)
    return sac


def chain_equals_standalone(gpu, bun, ce, head, seeds=(0, 3)):
    """[head..., sac] in the chain against the standalone call on what [head...] leaves -> the standalone results"""
    q0, m0, _ = ce.determineCorrespondences(rejectors=head())
    assert len(q0) > 3 and (np.diff(q0) > 0).all()  # by original query index
    results = []
    for seed in seeds:
        rq, rm, pos, T, st, _ = run_twice(make(gpu, bun["src"], bun["tgt"], 0.01, 1000, seed), q0, m0)
        assert st["has_model"] and 3 <= len(rq) < len(q0)
        for _ in range(2):
            sac = sac_rejector(gpu, seed)
            cq, cm, _ = ce.determineCorrespondences(rejectors=head() + [sac])
            assert np.array_equal(cq, rq) and np.array_equal(cm, rm)
            assert np.array_equal(bits(sac.getBestTransformation()), bits(T))
            cs = sac.lastStats()
            assert {k: cs[k] for k in st} == st
        results.append((rq, rm, T, st))
    return q0, m0, results


@pytest.fixture(scope="module")
def subset():
    """a strict, unsorted subset of the bunny's 397 source points"""
    ind = np.random.default_rng(41).permutation(397)[:200].astype(np.int32)
    assert (np.diff(ind) < 0).any() and len(set(ind.tolist())) == 200
    return ind


@pytest.mark.parametrize("first", ["distance", "none"])
def test_chain_on_a_source_subset(gpu, bun, subset, first):
    """n != n_orig: the keep bits are scattered over a cleared array and the list is numbered by original index"""
    head = (lambda: [distance_rejector(bun["golden"]["rej_dist_max_dist"])]) if first == "distance" else (lambda: [])
    q0, _, _ = chain_equals_standalone(gpu, bun, estimation(gpu, bun, subset), head)
    assert set(q0.tolist()) <= set(subset.tolist()) and (first == "distance" or len(q0) == 200)


def test_chain_on_a_permutation_of_the_whole_source(gpu, bun):
    """as many indices as records, in another order: nothing is cleared, every original index has its slot"""
    ind = np.random.default_rng(42).permutation(397).astype(np.int32)
    q0, _, _ = chain_equals_standalone(gpu, bun, estimation(gpu, bun, ind), lambda: [], seeds=(1,))
    assert np.array_equal(q0, np.arange(397))


def test_a_rejector_after_the_sample_consensus(gpu, bun):
    import pcl_amd

    def median():
        h = pcl_amd.CorrespondenceRejectorMedianDistance()
        h.setMedianFactor(1.0)
        return h

    ce = estimation(gpu, bun)
    q0, m0, results = chain_equals_standalone(gpu, bun, ce, lambda: [], seeds=(2,))
    rq, rm, T, st = results[0]
    # the median rejector over exactly the pairs the standalone call keeps: a chain of its own on those source points
    eq, em, _ = estimation(gpu, bun, rq).determineCorrespondences(rejectors=[median()])
    assert 0 < len(eq) < len(rq) and set(zip(eq.tolist(), em.tolist())) <= set(zip(rq.tolist(), rm.tolist()))
    sac = sac_rejector(gpu, 2)
    cq, cm, _ = ce.determineCorrespondences(rejectors=[sac, median()])
    assert np.array_equal(cq, eq) and np.array_equal(cm, em)
    assert np.array_equal(bits(sac.getBestTransformation()), bits(T))
    cs = sac.lastStats()
    assert {k: cs[k] for k in st} == st


class Registration:
    """CorrespondenceEstimation.determineCorrespondences on ONE registration object for several chains"""

    def __init__(self, gpu, src, tgt):
        import pcl_amd
        from pcl_amd import api
        self.api, self.gpu, self.lib = api, gpu, gpu.lib
        self.tree = pcl_amd.KdTree(gpu)
        self.tree.setInputCloud(tgt)
        self.src = np.ascontiguousarray(src, F)
        self.h = C.c_void_p()
        api.check(self.lib.pclhip_icp_create(self.tree.h, C.byref(self.h)), gpu.h)
        api.check(self.lib.pclhip_icp_set_source(self.h, C.c_void_p(self.src.ctypes.data), 12, len(self.src)), gpu.h)

    def apply(self, rejectors):
        api, lib, n = self.api, self.lib, len(self.src)
        api._set_filters(lib, self.gpu, self.h, list(rejectors), False)
        sums = np.zeros(api._lib.NSUMS, np.float64)
        api.check(lib.pclhip_icp_iterate(self.h, api._fp(I4.reshape(16).copy()), float(api._SQRT_DBL_MAX), api.POINT_TO_POINT,
                                         sums.ctypes.data_as(C.POINTER(C.c_double))), self.gpu.h)
        q, m, d = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, F)
        cnt = C.c_uint64(0)
        api.check(lib.pclhip_icp_fetch_correspondences(self.h, C.c_void_p(q.ctypes.data), C.c_void_p(m.ctypes.data),
                                                       C.c_void_p(d.ctypes.data), C.byref(cnt)), self.gpu.h)
        c = int(cnt.value)
        assert c == int(sums[28])
        api._read_filters(lib, self.gpu, self.h, rejectors)
        return q[:c].copy(), m[:c].copy()

    def close(self):
        self.lib.pclhip_icp_destroy(self.h)


def test_chain_on_lists_of_none_and_of_two_pairs(gpu, bun):
    """a distance rejector so tight that 0, then exactly 2 pairs reach the sample consensus: the list passes through, there
    is no model, and the registration goes on working"""
    src, tgt = bun["src"], bun["tgt"]
    reg = Registration(gpu, src, tgt)
    try:
        q0, m0 = reg.apply([])
        assert len(q0) == 397
        d2 = np.sort(((src[q0].astype(np.float64) - tgt[m0].astype(np.float64)) ** 2).sum(axis=1))
        assert d2[0] > 0 and d2[2] > 1.01 * d2[1]
        for max_distance, count in ((0.0, 0), (float(np.sqrt(0.5 * (d2[1] + d2[2]))), 2)):
            before = reg.apply([distance_rejector(max_distance)])
            assert len(before[0]) == count
            sac = sac_rejector(gpu, 0)
            after = reg.apply([distance_rejector(max_distance), sac])
            assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
            st = sac.lastStats()
            assert not st["has_model"] and st["n"] == count == st["remaining"] and st["trials"] == 0 and st["best_trial"] == -1
            assert np.array_equal(bits(sac.getBestTransformation()), bits(I4))
        # the next call on the same registration: the whole list again
        dist = bun["golden"]["rej_dist_max_dist"]
        qd, md = reg.apply([distance_rejector(dist)])
        rq, rm, pos, T, st, _ = run_twice(make(gpu, src, tgt, 0.01, 1000, 0), qd, md)
        sac = sac_rejector(gpu, 0)
        cq, cm = reg.apply([distance_rejector(dist), sac])
        assert st["has_model"] and np.array_equal(cq, rq) and np.array_equal(cm, rm)
        assert np.array_equal(bits(sac.getBestTransformation()), bits(T))
    finally:
        reg.close()


@pytest.mark.parametrize("whole", [False, True])
def test_chain_refuses_a_source_index_listed_twice(gpu, bun, subset, whole):
    """the standalone call refuses duplicate query indices, and so does the chain kind (include/pclhip.h): two slots of one
    original index would be one pair to the scan and two to the scoring pass, and with as many indices as records
    (whole) an original index without a slot would leave the scanned array unwritten."""
    from pcl_amd import PclHipError
    ind = np.arange(397, dtype=np.int32) if whole else subset.copy()
    ind[7] = ind[3]
    ce = estimation(gpu, bun, ind)
    for rejectors in ([sac_rejector(gpu, 0)], [distance_rejector(1.0), sac_rejector(gpu, 0)]):
        with pytest.raises(PclHipError) as e:
            ce.determineCorrespondences(rejectors=rejectors)
        assert e.value.status == -1 and "twice" in str(e.value)
    # the context still works, and so does the same estimation on a source without the repeat
    ind[7] = next(i for i in range(397) if i not in set(ind.tolist())) if not whole else 7
    ce.setIndicesSource(ind)
    cq, _, _ = ce.determineCorrespondences(rejectors=[sac_rejector(gpu, 0)])
    assert 3 <= len(cq) < len(ind)


# ---- h. device buffers -----------------------------------------------------------------------------------------------------------------
def raw_run(gpu, src, n_src, src_stride, tgt, n_tgt, tgt_stride, q, m, n, threshold, max_iterations, seed):
    """pclhip_correspondence_rejector_sample_consensus on raw pointers -> (positions, T bits, stats)"""
    from pcl_amd import _lib
    lib = gpu.lib
    p = _lib.RejectorSacParams()
    lib.pclhip_rejector_sac_params_default(C.byref(p))
    p.inlier_threshold, p.max_iterations, p.seed = threshold, max_iterations, seed
    pos = np.full(n, -7, np.int32)
    T = np.zeros(16, F)
    n_out = C.c_uint64(0)
    st = _lib.RejectorSacStats()
    rc = lib.pclhip_correspondence_rejector_sample_consensus(
        gpu.h, C.c_void_p(src), n_src, src_stride, C.c_void_p(tgt), n_tgt, tgt_stride, C.c_void_p(q), C.c_void_p(m), n,
        C.byref(p), C.c_void_p(pos.ctypes.data), n, C.byref(n_out), T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
    assert rc == 0, lib.pclhip_last_error(gpu.h)
    k = int(n_out.value)
    assert (pos[k:] == -7).all()
    return pos[:k].copy(), bits(T).copy(), (st.trials, st.iterations, st.best_trial, st.best_count, st.remaining, st.has_model,
                                            st.no_sample, st.n, st.sample_dist_thresh)


@pytest.mark.parametrize("width", [4, 8])
def test_torch_device_buffers(gpu, width):
    """clouds as device tensors with records of 4 and of 8 floats (stride 16 and 32), lists as device int32: the positions,
    the bytes of T and the statistics of the host call"""
    import torch
    src, tgt, q, m = scene(1200, 51)
    host = raw_run(gpu, src.ctypes.data, len(src), 12, tgt.ctypes.data, len(tgt), 12, q.ctypes.data, m.ctypes.data, len(q),
                   0.02, 1000, 5)
    rq, rm, pos, T, st, _ = run_twice(make(gpu, src, tgt, 0.02, 1000, 5), q, m)
    assert st["has_model"] and np.array_equal(host[0], pos) and np.array_equal(host[1], bits(T).reshape(-1))
    assert host[2][:4] == (st["trials"], st["iterations"], st["best_trial"], st["best_count"])
    rng = np.random.default_rng(52)
    wide = [np.ascontiguousarray(np.column_stack([c, rng.normal(size=(len(c), width - 3))]), F) for c in (src, tgt)]
    # host arrays with wide records first, then the same records and the lists in device memory
    got = raw_run(gpu, wide[0].ctypes.data, len(src), 4 * width, wide[1].ctypes.data, len(tgt), 4 * width, q.ctypes.data,
                  m.ctypes.data, len(q), 0.02, 1000, 5)
    assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]) and got[2] == host[2]
    ds, dt = (torch.from_numpy(w).cuda() for w in wide)
    dq, dm = torch.from_numpy(q).cuda(), torch.from_numpy(m).cuda()
    assert ds.is_cuda and ds.stride(0) == width and dq.dtype == torch.int32
    torch.cuda.synchronize()
    for _ in range(2):
        got = raw_run(gpu, ds.data_ptr(), len(src), 4 * width, dt.data_ptr(), len(tgt), 4 * width, dq.data_ptr(), dm.data_ptr(),
                      len(q), 0.02, 1000, 5)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]) and got[2] == host[2]
    # through the class: device clouds, host lists
    r = make(gpu, ds, dt, 0.02, 1000, 5)
    out = run_twice(r, q, m)
    assert np.array_equal(out[2], pos) and np.array_equal(bits(out[3]), bits(T)) and out[4] == st
