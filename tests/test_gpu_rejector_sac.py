"""pcl_amd.CorrespondenceRejectorSampleConsensus / pclhip_correspondence_rejector_sample_consensus / chain kind 4 on the
device against the numpy restatement (tests/rejector_sac_restatement.py, the same draw function) and the reference's golden
(tests/golden/rejector_sac_bun.json).  Every device call is made twice and its bytes are compared.

Quality against the reference's own 97 inliers on the 397 bunny pairs (threshold 0.01, 1,000 iterations): the bar is what the
restatement gets with the same seeds, and the device must equal it.  Restatement, seeds 0..3: winner counts 94, 97, 101, 97 after
345, 314, 278, 332 iterations (the reference's rand() sequence found 97; a numpy RANSAC with other draws gave 95-105).

Trace parity: samples, attempts and flags equal the restatement's; T within 1e-5 of the float64 umeyama for thick triangles
(the bar of tests/test_gpu_scp.py); counts exact for the device's own T; winner, iterations, remaining list and best T equal
to the restatement run on the device's transforms.  The scenes are chosen so that no float order can matter: asserted first."""
import json
import os

import numpy as np
import pytest

import rejector_sac_restatement as rr
from test_gpu_scp import triangle_is_thick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TILE = 2048  # pairs a block of the scoring kernel takes per step (rejector_sac.hpp: RSAC_TILE)
RESTATEMENT_BUNNY_COUNTS = {0: 94, 1: 97, 2: 101, 3: 97}


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def bun():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    f = json.load(open(os.path.join(ROOT, "tests", "golden", "rejector_sac_bun.json")))
    z = np.load(os.path.join(ROOT, "tests", "golden", "bunny.npz"))
    return dict(src=np.ascontiguousarray(z["bun0"][:, :3], F), tgt=np.ascontiguousarray(z["bun4"][:, :3], F),
                co=np.array(g["correspondences_original"], np.int32), fix=f, golden=g)


def rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def scene(n, seed, mismatched=0.3, noise=0.002):
    """a cloud, its rigid copy plus noise in another order, and the list: 30 % of the pairs name a wrong match"""
    rng = np.random.default_rng(seed)
    src = (rng.random((n, 3)) * (2.0, 1.5, 1.0) + (3.0, -1.0, 0.5)).astype(F)
    T = rigid(0.3, -0.2, 0.5, (0.4, -0.3, 0.2))
    order = rng.permutation(n)
    tgt = np.empty((n, 3), F)
    tgt[order] = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (n, 3))).astype(F)
    q = np.arange(n, dtype=np.int32)
    m = order.astype(np.int32)
    bad = rng.random(n) < mismatched
    if n > 0:
        m[bad] = rng.integers(0, n, int(bad.sum()))
    return src, tgt, q, m


def make(gpu, src, tgt, threshold, max_iterations=1000, seed=0, batch=0):
    import pcl_amd
    r = pcl_amd.CorrespondenceRejectorSampleConsensus(gpu)
    r.setInputSource(src)
    r.setInputTarget(tgt)
    r.setInlierThreshold(threshold)
    r.setMaximumIterations(max_iterations)
    r.setSeed(seed)
    r.setSaveInliers(True)
    if batch:
        r.setBatchSize(batch)
    return r


def run_twice(r, q, m):
    """getRemainingCorrespondences twice: the same bytes -> (index_query, index_match, positions, T, stats, trace)"""
    outs = []
    for _ in range(2):
        rq, rm = r.getRemainingCorrespondences(q, m)
        outs.append((rq, rm, r.getInliersIndices(), r.getBestTransformation(), r.lastStats(), r.trace()))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[3]), bits(b[3])) and a[4] == b[4] and len(a[5]) == len(b[5])
    for x, y in zip(a[5], b[5]):
        assert x["samples"] == y["samples"] and x["attempts"] == y["attempts"] and x["count"] == y["count"]
        assert np.array_equal(bits(x["transformation"]), bits(y["transformation"]))
    return a


def edge_margin(trace, s, seed, thresh):
    """the smallest |edge^2 - thresh| / thresh over every sample the restatement drew (good or bad)"""
    worst = np.inf
    for trial, rec in enumerate(trace):
        for a in range(rec["attempts"]):
            smp = rr.draw_samples(seed, trial, a, len(s))
            for i, j in ((0, 1), (0, 2), (1, 2)):
                e = float(rr.sr.edge_sq(s[smp[i]], s[smp[j]]))
                if np.isfinite(e) and thresh > 0:
                    worst = min(worst, abs(e - thresh) / thresh)
    return worst


def check_against_restatement(r, src, tgt, q, m, threshold, max_iterations, seed, out, margins=("k", "threshold", "edge")):
    """the device's run against the restatement on the device's own transforms, after the restatement alone has shown that
    no float order and no libm can matter on this scene.  margins: which of those three assertions are made (all, unless a
    case of tests/test_gpu_rejector_sac_regimes.py states why one cannot hold on its scene)"""
    rq, rm, pos, T, st, trace = out
    s, t = src[q], tgt[m]
    own = rr.reject(src, tgt, q, m, threshold, max_iterations, seed=seed)
    if "k" in margins:
        assert own["k_margin"] > 64 * 2.0 ** -52, "a trial's iteration count within 64 ulps of k: choose another scene"
    if "threshold" in margins:
        assert rr.threshold_margin(own["trace"], s, t, threshold) > 1e-6, "a pair within 1e-6 of threshold^2"
    if own["sample_dist_thresh"] > 0:
        if "edge" in margins:
            assert edge_margin(own["trace"], s, seed, own["sample_dist_thresh"]) > 1e-4, "an edge within 1e-4 of the sample threshold"
        assert abs(st["sample_dist_thresh"] - own["sample_dist_thresh"]) <= 1e-5 * own["sample_dist_thresh"]
    assert len(trace) == own["trials"] == st["trials"]
    for d, w in zip(trace, own["trace"]):
        assert d["samples"] == w["samples"] and d["attempts"] == w["attempts"] and d["no_sample"] == w["no_sample"]
    ref = rr.reject(src, tgt, q, m, threshold, max_iterations, seed=seed,
                    transforms={i: d["transformation"] for i, d in enumerate(trace)})
    if "threshold" in margins:
        assert rr.threshold_margin(ref["trace"], s, t, threshold) > 1e-6
    worst_R = worst_t = 0.0
    for d, w in zip(trace, ref["trace"]):
        if d["no_sample"]:
            assert d["count"] == 0 and not d["transformation"].any()
            continue
        assert d["count"] == w["count"]  # exact, for the device's own T
        smp = d["samples"]
        if triangle_is_thick(s[smp].astype(np.float64)) and triangle_is_thick(t[smp].astype(np.float64)):
            T64 = w["T64"]
            worst_R = max(worst_R, np.abs(d["transformation"][:3, :3] - T64[:3, :3]).max())
            worst_t = max(worst_t, np.abs(d["transformation"][:3, 3] - T64[:3, 3]).max() / (1 + np.abs(T64[:3, 3]).max()))
    assert worst_R <= 1e-5 and worst_t <= 1e-5, (worst_R, worst_t)
    assert st["best_trial"] == ref["best_trial"] and st["iterations"] == ref["iterations"]
    assert st["best_count"] == ref["best_count"] and st["has_model"] == ref["has_model"]
    assert st["no_sample"] == ref["no_sample"] and st["n"] == len(q)
    assert np.array_equal(pos, ref["remaining"] if ref["has_model"] else np.zeros(0, np.int32))
    assert np.array_equal(rq, ref["index_query"]) and np.array_equal(rm, ref["index_match"])
    assert np.array_equal(bits(T), bits(ref["T"]))
    return ref


# ---- a. golden ---------------------------------------------------------------------------------------------------------------
def test_golden_transform_scores_the_reference_97(gpu, bun):
    r = make(gpu, bun["src"], bun["tgt"], bun["fix"]["rej_sac_max_dist"])
    co = bun["co"]
    T = np.array(bun["fix"]["transform_from_SAC"], F)
    for _ in range(2):
        cnt = r.evaluate(T[None], co[:, 0], co[:, 1])
        assert cnt.tolist() == [97]
    # several transforms in one call: the golden one, the identity, a far one
    far = np.eye(4, dtype=F)
    far[:3, 3] = 5
    cnt = r.evaluate(np.stack([T, np.eye(4, dtype=F), far, T]))
    s, t = bun["src"][co[:, 0]], bun["tgt"][co[:, 1]]
    assert cnt.tolist() == [97, rr.count_within(np.eye(4, dtype=F), s, t, 0.01), 0, 97]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_golden_run_equals_the_restatement(gpu, bun, seed):
    fix, co = bun["fix"], bun["co"]
    thr, iters = fix["rej_sac_max_dist"], fix["rej_sac_max_iter"]
    own = rr.reject(bun["src"], bun["tgt"], co[:, 0], co[:, 1], thr, iters, seed=seed)
    print("seed %d: restatement winner %d inliers (reference: 97)" % (seed, own["best_count"]))
    assert own["best_count"] == RESTATEMENT_BUNNY_COUNTS[seed]  # the bar: asserted first, on the CPU
    r = make(gpu, bun["src"], bun["tgt"], thr, iters, seed)
    out = run_twice(r, co[:, 0], co[:, 1])
    rq, rm, pos, T, st, trace = out
    assert len(rq) >= 3 and (np.diff(pos) > 0).all()
    assert np.array_equal(rq, co[pos, 0]) and np.array_equal(rm, co[pos, 1])          # a subset of the input, in order
    keep = rr.within(T, bun["src"][co[:, 0]], bun["tgt"][co[:, 1]], thr)
    assert np.array_equal(np.nonzero(keep)[0], pos)                                     # the score of the returned T
    assert r.evaluate(T[None]).tolist() == [len(pos)]
    check_against_restatement(r, bun["src"], bun["tgt"], co[:, 0], co[:, 1], thr, iters, seed, out)
    assert st["best_count"] == own["best_count"]                                        # the device equals the bar


# ---- b. trace parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(1500, 1), (700, 7)])
def test_trace_parity_on_a_synthetic_scene(gpu, n, seed):
    src, tgt, q, m = scene(n, 100 + seed)
    r = make(gpu, src, tgt, 0.02, 1000, seed)
    out = run_twice(r, q, m)
    ref = check_against_restatement(r, src, tgt, q, m, 0.02, 1000, seed, out)
    assert ref["has_model"] and 0.6 * n < ref["best_count"] < 0.8 * n  # the 70 % that were not mismatched


# ---- c. sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_sizes(gpu, n):
    src, tgt, q, m = scene(n, 40 + n) if n else (np.zeros((1, 3), F), np.zeros((1, 3), F), np.zeros(0, np.int32),
                                                  np.zeros(0, np.int32))
    r = make(gpu, src, tgt, 0.02, 40, 3)
    out = run_twice(r, q, m)
    check_against_restatement(r, src, tgt, q, m, 0.02, 40, 3, out)
    if n < 3:
        assert np.array_equal(out[0], q) and np.array_equal(bits(out[3]), bits(np.eye(4, dtype=F)))


def test_sizes_largest(gpu):
    n = 10000
    src, tgt, q, m = scene(n, 77)
    r = make(gpu, src, tgt, 0.02, 40, 5)
    out = run_twice(r, q, m)
    check_against_restatement(r, src, tgt, q, m, 0.02, 40, 5, out)


@pytest.mark.parametrize("max_iterations", [0, 1, 63, 64, 65])
def test_hypothesis_counts_across_a_batch_edge(gpu, max_iterations):
    # all pairs mismatched: no hypothesis gathers a consensus, so the loop runs to max_iterations + 1 trials
    src, tgt, q, m = scene(300, 5, mismatched=1.0)
    results = []
    for batch in (64, 1, 7, 0):
        r = make(gpu, src, tgt, 0.02, max_iterations, 2, batch)
        out = run_twice(r, q, m)
        assert out[4]["trials"] == max_iterations + 1 == out[4]["iterations"]
        results.append(out)
    check_against_restatement(r, src, tgt, q, m, 0.02, max_iterations, 2, results[0])
    a = results[0]
    for b in results[1:]:  # the batch schedule never changes a result
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3]))
        assert a[4] == b[4] and [t["count"] for t in a[5]] == [t["count"] for t in b[5]]
        assert all(np.array_equal(bits(x["transformation"]), bits(y["transformation"])) for x, y in zip(a[5], b[5]))


def test_batch_size_never_changes_a_converging_run(gpu):
    src, tgt, q, m = scene(900, 21)
    outs = [run_twice(make(gpu, src, tgt, 0.02, 1000, 4, batch), q, m) for batch in (1, 7, 0)]
    for b in outs[1:]:
        assert np.array_equal(outs[0][2], b[2]) and np.array_equal(bits(outs[0][3]), bits(b[3])) and outs[0][4] == b[4]


# ---- d. result rules ----------------------------------------------------------------------------------------------------------
def test_fewer_than_three_inliers_leave_the_list(gpu):
    src, tgt, q, m = scene(200, 9)
    r = make(gpu, src, tgt, 1e-7, 30, 1)  # only the sampled pairs themselves can fall inside
    out = run_twice(r, q, m)
    ref = check_against_restatement(r, src, tgt, q, m, 1e-7, 30, 1, out)
    assert not ref["has_model"] and ref["best_count"] < 3
    assert np.array_equal(out[0], q) and np.array_equal(out[1], m) and np.array_equal(bits(out[3]), bits(np.eye(4, dtype=F)))
    assert out[4]["remaining"] == 200


def test_coincident_source_points_find_no_sample(gpu):
    n = 50
    src = np.tile(np.array([[1.0, 2.0, 3.0]], F), (n, 1))
    tgt = np.random.default_rng(0).random((n, 3)).astype(F)
    q = m = np.arange(n, dtype=np.int32)
    r = make(gpu, src, tgt, 0.05, 1000, 0)
    rq, rm, pos, T, st, trace = run_twice(r, q, m)
    assert st["sample_dist_thresh"] == 0.0 and st["no_sample"] and st["trials"] == 1 and not st["has_model"]
    assert len(trace) == 1 and trace[0]["attempts"] == 1000 and trace[0]["no_sample"]
    assert np.array_equal(rq, q) and np.array_equal(rm, m) and np.array_equal(bits(T), bits(np.eye(4, dtype=F)))
    own = rr.reject(src, tgt, q, m, 0.05, 1000, seed=0)
    assert own["no_sample"] and own["trials"] == 1 and own["trace"][0]["samples"] == trace[0]["samples"]


def test_nan_points_are_never_inliers(gpu):
    src, tgt, q, m = scene(400, 31, mismatched=0.1)
    src[5] = np.nan
    src[17, 1] = np.inf
    tgt[m[40], 2] = np.nan
    r = make(gpu, src, tgt, 0.02, 200, 6)
    out = run_twice(r, q, m)
    ref = check_against_restatement(r, src, tgt, q, m, 0.02, 200, 6, out)
    assert ref["has_model"] and not ({5, 17, 40} & set(out[2].tolist()))
    assert np.isfinite(out[4]["sample_dist_thresh"]) and out[4]["sample_dist_thresh"] > 0  # the moments skip them


# ---- e. chain equals standalone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["distance", "median"])
def test_chain_equals_standalone(gpu, bun, first):
    import pcl_amd
    src, tgt = bun["src"], bun["tgt"]

    def head():
        if first == "distance":
            h = pcl_amd.CorrespondenceRejectorDistance()
            h.setMaximumDistance(bun["golden"]["rej_dist_max_dist"])
        else:
            h = pcl_amd.CorrespondenceRejectorMedianDistance()
            h.setMedianFactor(bun["golden"]["rej_median_factor"])
        return h

    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputTarget(tgt)
    ce.setInputSource(src)
    q0, m0, _ = ce.determineCorrespondences(rejectors=[head()])
    assert 3 < len(q0) < 397
    for seed in (0, 3):
        alone = make(gpu, src, tgt, 0.01, 1000, seed)
        rq, rm, pos, T, st, _ = run_twice(alone, q0, m0)
        assert st["has_model"] and 3 <= len(rq) < len(q0)
        for _ in range(2):
            sac = pcl_amd.CorrespondenceRejectorSampleConsensus(gpu)
            sac.setInlierThreshold(0.01)
            sac.setMaximumIterations(1000)
            sac.setSeed(seed)
            cq, cm, _ = ce.determineCorrespondences(rejectors=[head(), sac])
            assert np.array_equal(cq, rq) and np.array_equal(cm, rm)
            assert np.array_equal(bits(sac.getBestTransformation()), bits(T))
            cs = sac.lastStats()
            assert {k: cs[k] for k in st} == st


# ---- f. ICP ------------------------------------------------------------------------------------------------------------------
def mat4_mul_f32(A, B):
    """the library's float product (host_math.cpp: mat4_mul_f32): each entry summed over k = 0..3 in order, in float32
    (numpy's @ is free to order and fuse the sum otherwise)"""
    out = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            a = F(0)
            for k in range(4):
                a = F(a + F(A[i, k] * B[k, j]))
            out[i, j] = a
    return out


def host_loop_align(icp, conv):
    """impl/icp.hpp:113-268 driven from the host (tests/test_gpu_loop.py: _host_loop_align, with the library's own float
    product for final_transformation_, since this test compares bits)"""
    import ctypes as C
    from pcl_amd import _lib
    lib = _lib.load()
    icp.reset()
    final = np.eye(4, dtype=F)
    T_apply = np.eye(4, dtype=F)
    it = 0
    while True:
        sums = icp.iterate(T_apply)
        ncorr = sums[28]
        if ncorr < icp.p.min_number_correspondences:
            break
        Tk = icp.solve(sums)
        T_apply = Tk
        final = mat4_mul_f32(np.asarray(Tk, F), final)
        it += 1
        t = np.ascontiguousarray(Tk, F).reshape(16)
        if lib.pclhip_convergence_has_converged(C.byref(icp.p), C.byref(conv), it, t.ctypes.data_as(C.POINTER(C.c_float)),
                                                float(sums[27] / ncorr)) or conv.convergence_state != 0:
            break
    return final, it


ICP_CASES = [  # (delta translation, net rotation angles, net translation): test_registration.cpp:350-365 samples such pairs
    ((0.030, 0.020, 0.030), (0.8, -1.9, 2.6), (7.98, 9.12, 1.98)),
    ((0.010, 0.035, 0.005), (2.9, 0.4, -1.2), (3.35, 7.68, 2.78)),
    ((0.028, 0.028, 0.028), (-0.6, 1.1, 0.2), (5.54, 4.77, 6.29)),
]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_icp_with_median_and_sample_consensus_rejectors(gpu, bun, case):
    """the reference's IterativeClosestPointWithRejectors (test/registration/test_registration.cpp:337-381)"""
    import ctypes as C
    import pcl_amd
    from pcl_amd import _lib
    dt, ang, nt = ICP_CASES[case]
    assert np.linalg.norm(dt) <= 0.05
    delta = rigid(0, 0, 0, dt)
    net = rigid(*ang, nt)
    p = np.concatenate([bun["src"].astype(np.float64), np.ones((397, 1))], axis=1)
    source = np.ascontiguousarray((p @ (np.linalg.inv(delta) @ net).T)[:, :3], F)
    target = np.ascontiguousarray((p @ net.T)[:, :3], F)

    def reg():
        icp = pcl_amd.IterativeClosestPoint(gpu)
        icp.setInputTarget(target)
        icp.setInputSource(source)
        icp.setMaximumIterations(50)
        icp.setTransformationEpsilon(1e-8)
        icp.setMaxCorrespondenceDistance(0.15)
        med = pcl_amd.CorrespondenceRejectorMedianDistance()
        med.setMedianFactor(4.0)
        icp.addCorrespondenceRejector(med)
        sac = pcl_amd.CorrespondenceRejectorSampleConsensus(gpu)  # defaults: 0.05, 1,000 iterations
        icp.addCorrespondenceRejector(sac)
        return icp, sac

    finals = []
    for _ in range(2):
        dev, sac = reg()
        dev.align()
        T = dev.getFinalTransformation()
        finals.append(T)
        print("case %d: %d iterations, |t - delta| = %.3g" % (case, dev.nr_iterations_, np.abs(T[:3, 3] - delta[:3, 3]).max()))
        assert np.abs(T[:, 3] - delta[:, 3]).max() < 1e-2          # the reference's own bars (:373-379)
        assert np.abs(T[:, :3] - delta[:, :3]).max() < 1e-1
        assert sac.lastStats()["has_model"] and np.abs(sac.getBestTransformation() - np.eye(4)).max() < 0.1
    assert np.array_equal(bits(finals[0]), bits(finals[1]))
    host, _ = reg()
    host._ensure()
    conv = _lib.ConvergenceState()
    _lib.load().pclhip_convergence_init(C.byref(conv))
    Th, it = host_loop_align(host, conv)
    assert it == dev.nr_iterations_
    assert np.array_equal(bits(Th), bits(finals[0]))  # host-driven and device-driven: the same bits


# ---- g. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu, bun):
    import ctypes as C
    import pcl_amd
    from pcl_amd import PclHipError, _lib
    co = bun["co"]
    r = make(gpu, bun["src"], bun["tgt"], 0.01, 100, 0)
    with pytest.raises(NotImplementedError):
        r.setRefineModel(True)
    r.setRefineModel(False)
    lib = gpu.lib
    p = _lib.RejectorSacParams()
    lib.pclhip_rejector_sac_params_default(C.byref(p))
    assert (p.inlier_threshold, p.max_iterations, p.probability, p.refine) == (0.05, 1000, 0.99, 0)
    p.refine = 1
    n_out = C.c_uint64(7)
    q, m = np.ascontiguousarray(co[:, 0]), np.ascontiguousarray(co[:, 1])
    rc = lib.pclhip_correspondence_rejector_sample_consensus(
        gpu.h, C.c_void_p(bun["src"].ctypes.data), 397, 12, C.c_void_p(bun["tgt"].ctypes.data), 361, 12,
        C.c_void_p(q.ctypes.data), C.c_void_p(m.ctypes.data), 397, C.byref(p), None, 0, C.byref(n_out), None, None)
    assert rc == -1 and b"setRefineModel" in lib.pclhip_last_error(gpu.h)
    dup_q = q.copy()
    dup_q[10] = dup_q[3]
    with pytest.raises(PclHipError) as e:
        r.getRemainingCorrespondences(dup_q, m)
    assert e.value.status == -1 and "twice" in str(e.value)
    for bad_q, bad_m in ((397, 0), (-1, 0), (0, 361), (0, -1)):
        qq, mm = q.copy(), m.copy()
        qq[5], mm[5] = bad_q, bad_m
        with pytest.raises(PclHipError) as e:
            r.getRemainingCorrespondences(qq, mm)
        assert e.value.status == -1 and "outside" in str(e.value)
    # a capacity that is too small: the count first, then the overflow
    p.refine = 0
    p.inlier_threshold = 0.01
    pos = np.zeros(2, np.int32)
    rc = lib.pclhip_correspondence_rejector_sample_consensus(
        gpu.h, C.c_void_p(bun["src"].ctypes.data), 397, 12, C.c_void_p(bun["tgt"].ctypes.data), 361, 12,
        C.c_void_p(q.ctypes.data), C.c_void_p(m.ctypes.data), 397, C.byref(p), C.c_void_p(pos.ctypes.data), 2, C.byref(n_out),
        None, None)
    assert rc == -5 and n_out.value == RESTATEMENT_BUNNY_COUNTS[0]
    # kind 5 in the chain is still unknown; kind 4 is not
    ce = pcl_amd.CorrespondenceEstimation(gpu)
    ce.setInputTarget(bun["tgt"])
    ce.setInputSource(bun["src"])
    h = C.c_void_p()
    assert lib.pclhip_icp_create(ce.tree.h, C.byref(h)) == 0
    try:
        arr = (_lib.Rejector * 1)()
        arr[0].kind, arr[0].param, arr[0].min_correspondences = 5, 0.05, 1000
        assert lib.pclhip_icp_set_rejectors(h, arr, 1) == -1 and b"unknown rejector kind" in lib.pclhip_last_error(gpu.h)
        arr[0].kind = 4
        assert lib.pclhip_icp_set_rejectors(h, arr, 1) == 0
        T = np.zeros(16, F)
        assert lib.pclhip_icp_last_sac_transformation(h, T.ctypes.data_as(C.POINTER(C.c_float))) == -4  # none has run yet
    finally:
        lib.pclhip_icp_destroy(h)
    # the context still works
    rq, rm = r.getRemainingCorrespondences(q, m)
    assert len(rq) >= 3
