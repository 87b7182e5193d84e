"""SACSegmentation (planes, RANSAC) on the device against the numpy restatement (tests/sac_restatement.py, pinned on the
reference's own criterion by tests/test_sac_restatement.py).  Per trial of the trace the samples, the coefficient bits, the
skip flag and the count are equal; so are the winner, the iterations and both lists.  Every case runs twice and the two runs'
outputs must be the same bytes.

Instability cap: 0.  The restatement is the same float32 arithmetic in the same order, so no trial is excluded from the
bitwise comparison (sac_restatement.unstable exists to say why, should one ever differ)."""
import ctypes as C
import os

import numpy as np
import pytest

import sac_restatement as sac

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 3072  # points a block of the scoring kernel takes per step (sac.hpp: SAC_BLOCK * SAC_P)
BATCH = 1024  # hypotheses of one scoring pass (SAC_MAX_BATCH)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def gold():
    return np.ascontiguousarray(np.load(os.path.join(GOLD, "sac_plane_radius.npz"))["cloud"][:, :3], np.float32)


@pytest.fixture(scope="module")
def gold_refs(gold):
    """the restatement on the golden cloud, once per seed"""
    return {seed: sac.segment(gold, 0.03, seed=seed) for seed in (1, 2, 3)}


def scene(n, seed=0, clutter=0.3):
    """a tilted plane with noise and uniform clutter, n points"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n, 2))
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.5 + rng.normal(0, 0.004, n)
    off = rng.random(n) < clutter
    z[off] = rng.uniform(-1, 2, int(off.sum()))
    return np.ascontiguousarray(np.column_stack([xy, z]), np.float32)


def segmenter(gpu, cloud, thr, seed=0, max_iterations=50, probability=0.99, optimize=True, indices=None, batch=0):
    import pcl_amd
    s = pcl_amd.SACSegmentation(gpu)
    s.setModelType(pcl_amd.SACMODEL_PLANE)
    s.setMethodType(pcl_amd.SAC_RANSAC)
    s.setDistanceThreshold(thr)
    s.setMaxIterations(max_iterations)
    s.setProbability(probability)
    s.setOptimizeCoefficients(optimize)
    s.setSeed(seed)
    s.setBatchSize(batch)
    s.setInputCloud(cloud)
    s.setIndices(indices)
    return s


def trace_bytes(tr):
    return b"".join(np.array(t["samples"] + [int(t["skipped"]), t["count"]], np.int64).tobytes() + t["coefficients"].tobytes()
                    for t in tr)


def run(gpu, cloud, thr, **kw):
    """segment twice: the same bytes -> dict(inliers, coefficients, outliers, stats, trace, seg)"""
    s = segmenter(gpu, cloud, thr, **kw)
    inl, coeff = s.segment()
    out = dict(inliers=np.asarray(inl).copy(), coefficients=np.asarray(coeff).copy(), outliers=np.asarray(s.getOutliers()).copy(),
               stats=s.lastStats(), trace=s.trace(), seg=s)
    inl2, coeff2 = s.segment()
    assert out["inliers"].tobytes() == np.asarray(inl2).tobytes() and out["coefficients"].tobytes() == np.asarray(coeff2).tobytes()
    assert out["outliers"].tobytes() == np.asarray(s.getOutliers()).tobytes()
    assert trace_bytes(out["trace"]) == trace_bytes(s.trace())
    st2 = s.lastStats()
    assert all(out["stats"][k] == st2[k] for k in ("trials", "iterations", "skipped", "best_trial", "best_count", "refined"))
    assert out["inliers"].dtype == np.int32 and out["outliers"].dtype == np.int32
    return out


def same_trace(got, ref):
    assert len(got) == len(ref)
    for t, (a, b) in enumerate(zip(got, ref)):
        assert a["samples"] == b["samples"] and a["skipped"] == b["skipped"] and a["count"] == b["count"], (t, a, b)
        ca, cb = a["coefficients"], b["coefficients"]
        nan = np.isnan(cb)  # (the sign of a NaN is not pinned)
        assert np.array_equal(np.isnan(ca), nan) and ca[~nan].tobytes() == cb[~nan].tobytes(), (t, ca, cb)


def check(gpu, cloud, thr, ref=None, **kw):
    """the device against the restatement: trace, winner, iterations, lists.  With the refit the refined selection is
    the restatement's select on the DEVICE's refined coefficients (the refit's sums differ from the reference's float
    sums by design; test_refit_against_float64 measures them)."""
    got = run(gpu, cloud, thr, **kw)
    if ref is None:
        ref = sac.segment(cloud, thr, max_iterations=kw.get("max_iterations", 50), probability=kw.get("probability", 0.99),
                          optimize=False, seed=kw.get("seed", 0), indices=kw.get("indices"))
    same_trace(got["trace"], ref["trace"])
    st = got["stats"]
    assert (st["trials"], st["iterations"], st["skipped"], st["best_trial"], st["best_count"]) == \
        (ref["trials"], ref["iterations"], ref["skipped"], ref["best_trial"], ref["best_count"])
    pts, ids = sac.point_set(cloud, kw.get("indices"))
    if not ref["found"]:
        assert len(got["inliers"]) == 0 and len(got["coefficients"]) == 0 and np.array_equal(got["outliers"], ids)
        return got, ref
    if st["refined"]:
        assert kw.get("optimize", True) and ref["best_count"] > 3
        mask = sac.within(pts, got["coefficients"], thr)
    else:
        assert got["coefficients"].tobytes() == ref["coefficients"].tobytes()
        mask = sac.within(pts, ref["coefficients"], thr)
        assert int(mask.sum()) == ref["best_count"]
    assert np.array_equal(got["inliers"], ids[mask]) and np.array_equal(got["outliers"], ids[~mask])
    assert st["n_inliers"] == int(mask.sum()) and st["n_outliers"] == int((~mask).sum())
    return got, ref


# ---- the golden cloud ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_golden_cloud(gpu, gold, gold_refs, seed):
    ref = gold_refs[seed]
    got, _ = check(gpu, gold, 0.03, ref=ref, seed=seed, optimize=False)
    assert got["stats"]["batches"] == 1 and len(got["inliers"]) == ref["best_count"] > 2000
    assert np.array_equal(got["inliers"], ref["first_inliers"])
    # countWithinDistance of the traced models gives their counts
    models = np.stack([t["coefficients"] for t in got["trace"]])
    cnt = got["seg"].countWithinDistance(models)
    assert cnt.tolist() == [t["count"] for t in got["trace"]]
    assert got["seg"].countWithinDistance(models).tobytes() == cnt.tobytes()
    got, _ = check(gpu, gold, 0.03, ref=ref, seed=seed, optimize=True)
    assert got["stats"]["refined"]


def float64_fit(points):
    p = np.asarray(points, np.float64)
    c = p.mean(0)
    w, v = np.linalg.eigh(np.cov((p - c).T, bias=True))
    n = v[:, 0]
    return np.array([n[0], n[1], n[2], -float(n @ c)])


def fit_distance(coeff, fit):
    """largest component difference after aligning the sign, d's relative to max(1, |d|)"""
    c = np.asarray(coeff, np.float64)
    if np.dot(c[:3], fit[:3]) < 0:
        c = -c
    e = np.abs(c - fit)
    e[3] /= max(1.0, abs(fit[3]))
    return float(e.max())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_refit_against_float64(gpu, gold, gold_refs, seed):
    """The refined plane against a float64 fit (numpy eigh) of the same inliers.  Bar: the device is no further from it
    than 2 x the distance of the reference's float path (sac_restatement.refit: the oracle's computeMeanAndCovarianceMatrix
    and eigen33) from it, plus 8 * 2^-24 (the float representation of a unit vector's components)."""
    ref = gold_refs[seed]
    got = run(gpu, gold, 0.03, seed=seed, optimize=True)
    assert got["stats"]["refined"]
    fit = float64_fit(gold[ref["first_inliers"]])
    d_dev = fit_distance(got["coefficients"], fit)
    d_ref = fit_distance(ref["refined"], fit)
    print("seed %d: device %.3g, reference float path %.3g from the float64 fit" % (seed, d_dev, d_ref))
    assert d_dev <= 2.0 * d_ref + 8.0 * 2.0 ** -24
    mask = sac.within(gold, got["coefficients"], 0.03)
    assert np.array_equal(got["inliers"], np.nonzero(mask)[0]) and np.array_equal(got["outliers"], np.nonzero(~mask)[0])
    off = run(gpu, gold, 0.03, seed=seed, optimize=False)
    assert off["coefficients"].tobytes() == ref["coefficients"].tobytes() and not off["stats"]["refined"]


# ---- edges of the count kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, TILE - 1, TILE, TILE + 1, 100007])
def test_point_counts(gpu, n):
    cloud = scene(n, seed=n)
    thr = 0.01 if n > 4 else 10.0
    got, ref = check(gpu, cloud, thr, seed=n)
    assert ref["found"]
    models = np.stack([t["coefficients"] for t in ref["trace"]])
    assert got["seg"].countWithinDistance(models).tolist() == [sac.count_within(cloud, m, thr) for m in models]


def test_fewer_than_three_points(gpu):
    for n in (0, 1, 2):
        got = run(gpu, scene(3)[:n].reshape(n, 3), 1.0)
        assert len(got["inliers"]) == 0 and len(got["coefficients"]) == 0 and got["outliers"].tolist() == list(range(n))
        assert got["stats"]["best_trial"] == -1 and got["stats"]["trials"] == 0


@pytest.mark.parametrize("h", [1, 2, 65, BATCH + 1])
def test_model_counts(gpu, h):
    cloud = scene(5000, seed=7)
    rng = np.random.default_rng(h)
    nrm = rng.normal(0, 1, (h, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    models = np.column_stack([nrm, rng.uniform(-1, 1, h)]).astype(np.float32)
    models[0] = (0.3, -0.2, -1.0, 0.5)
    models[0] /= np.linalg.norm(models[0, :3])
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):  # a coefficient that is not finite counts 0
        if 1 + i < h:
            models[-1 - i, (i + 3) % 4] = bad
    s = segmenter(gpu, cloud, 0.02)
    cnt = s.countWithinDistance(models)
    assert cnt.dtype == np.uint32 and cnt.tobytes() == s.countWithinDistance(models).tobytes()
    assert cnt.tolist() == [sac.count_within(cloud, m, 0.02) for m in models]
    assert cnt[0] > 1000 and (h < 2 or cnt[-1] == 0)
    for thr in (0.0, -1.0, float("nan")):  # nothing is below a threshold of 0
        s.setDistanceThreshold(thr)
        assert not s.countWithinDistance(models).any()


def test_batch_size_changes_nothing(gpu, gold, gold_refs):
    ref = gold_refs[2]
    runs = [check(gpu, gold, 0.03, ref=ref, seed=2, batch=b)[0] for b in (0, 1, 7)]
    assert [r["stats"]["batches"] for r in runs] == [1, 8, 2]
    for r in runs[1:]:
        assert r["inliers"].tobytes() == runs[0]["inliers"].tobytes() and r["outliers"].tobytes() == runs[0]["outliers"].tobytes()
        assert r["coefficients"].tobytes() == runs[0]["coefficients"].tobytes()
        assert trace_bytes(r["trace"]) == trace_bytes(runs[0]["trace"])
    # ... nor does it when skips stretch the call over several automatic batches
    cloud = scene(300, seed=11)
    cloud[: 200] = cloud[0]  # two thirds coincide: most samples are degenerate
    runs = [check(gpu, cloud, 0.01, seed=4, max_iterations=200, probability=0.999999, batch=b)[0] for b in (0, 1, 7, 1024)]
    assert runs[0]["stats"]["skipped"] > 50 and runs[0]["stats"]["batches"] > 1
    for r in runs[1:]:
        assert trace_bytes(r["trace"]) == trace_bytes(runs[0]["trace"]) and r["inliers"].tobytes() == runs[0]["inliers"].tobytes()


def test_strict_bound(gpu):
    thr = 0.03
    at = np.float32(thr)
    below = np.nextafter(at, np.float32(0))
    g = np.arange(40, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    z = np.where((X + Y) % 2 == 0, at, below).astype(np.float32)
    z[::3] *= -1
    cloud = np.column_stack([X.ravel(), Y.ravel(), z.ravel()]).astype(np.float32)
    s = segmenter(gpu, cloud, thr)
    cnt = s.countWithinDistance([[0, 0, 1, 0], [0, 0, -1, 0]])
    expect = int((np.abs(cloud[:, 2]) == below).sum())
    assert 0 < expect < len(cloud) and cnt.tolist() == [expect, expect]
    assert sac.count_within(cloud, [0, 0, 1, 0], thr) == expect


# ---- indices --------------------------------------------------------------------------------------------------------------
def test_indices(gpu, gold):
    rng = np.random.default_rng(3)
    n = len(gold)
    subset = np.arange(0, n, 3, dtype=np.int32)
    for ind in (subset, rng.permutation(subset).astype(np.int32), np.repeat(np.arange(100, 1500, dtype=np.int32), 2)):
        for optimize in (False, True):
            got, ref = check(gpu, gold, 0.03, seed=5, indices=ind, optimize=optimize)
            assert ref["found"] and np.isin(got["inliers"], ind).all()
            # inliers + outliers = the index list, each in the list's order
            both = np.concatenate([got["inliers"], got["outliers"]])
            assert sorted(both.tolist()) == sorted(ind.tolist())
            pos = {}
            for p, v in enumerate(ind.tolist()):
                pos.setdefault(v, p)
            for lst in (got["inliers"], got["outliers"]):
                first = [pos[v] for v in lst.tolist()]
                assert all(a <= b for a, b in zip(first, first[1:]))
    import pcl_amd
    for bad in ([0, 1, n], [-1, 2, 3]):
        with pytest.raises(pcl_amd._lib.PclHipError) as ei:
            segmenter(gpu, gold, 0.03, indices=np.array(bad, np.int32)).segment()
        assert ei.value.status == -1  # PCLHIP_ERR_INVALID


# ---- records that are not finite -------------------------------------------------------------------------------------------
def test_non_finite_records(gpu, gold):
    cloud = gold.copy()
    rng = np.random.default_rng(9)
    bad = np.sort(rng.choice(len(cloud), len(cloud) // 4, replace=False))
    cloud[bad, rng.integers(0, 3, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    for optimize in (False, True):
        got, ref = check(gpu, cloud, 0.03, seed=6, optimize=optimize)
        assert ref["found"] and not np.isin(bad, got["inliers"]).any() and np.isin(bad, got["outliers"]).all()
        hit = [t for t in got["trace"] if np.isin(t["samples"], bad).any()]
        assert hit and all(t["count"] == 0 and not t["skipped"] for t in hit)  # sampled: no skip, counts 0


# ---- clouds without a plane ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["collinear", "coincident", "tiny"])
def test_degenerate_clouds(gpu, kind):
    n = 500
    t = np.linspace(0, 1, n, dtype=np.float32)
    if kind == "collinear":
        cloud = np.column_stack([t, 2 * t, -t]).astype(np.float32)
    elif kind == "coincident":
        cloud = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (n, 1))
    else:
        cloud = (scene(n, seed=1) * np.float32(1e-4)).astype(np.float32)  # every cross product is below 1e-5
    got, ref = check(gpu, cloud, 0.01, seed=2, max_iterations=5)
    assert not ref["found"] and got["stats"]["skipped"] == 50 and got["stats"]["trials"] == 50
    assert got["stats"]["iterations"] == 0 and got["stats"]["best_trial"] == -1
    assert len(got["inliers"]) == 0 and len(got["coefficients"]) == 0 and len(got["outliers"]) == n


# ---- capacities ---------------------------------------------------------------------------------------------------------------
def test_capacity_too_small(gpu, gold, gold_refs):
    import pcl_amd
    ref = gold_refs[1]
    n_in, n_out = ref["best_count"], len(gold) - ref["best_count"]
    for cap_in, cap_out in ((n_in - 1, n_out), (n_in, n_out - 1), (0, 0)):
        s = segmenter(gpu, gold, 0.03, seed=1, optimize=False)
        with pytest.raises(pcl_amd._lib.PclHipError) as ei:
            s.segment(inliers_capacity=cap_in, outliers_capacity=cap_out)
        assert ei.value.status == -5  # PCLHIP_ERR_OVERFLOW, after the counts
        assert (s.lastStats()["n_inliers"], s.lastStats()["n_outliers"]) == (n_in, n_out)
    s = segmenter(gpu, gold, 0.03, seed=1, optimize=False)
    inl, coeff = s.segment(inliers_capacity=n_in, outliers_capacity=n_out)  # exactly enough
    assert np.array_equal(inl, ref["first_inliers"]) and len(s.getOutliers()) == n_out
    # every list is optional: the counts and the coefficients alone
    p = pcl_amd._lib.SacPlaneParams()
    gpu.lib.pclhip_sac_plane_params_default(C.byref(p))
    assert (p.distance_threshold, p.max_iterations, p.probability, p.optimize_coefficients) == (0.0, 50, 0.99, 1)
    p.distance_threshold, p.seed, p.optimize_coefficients = 0.03, 1, 0
    coeff = np.zeros(4, np.float32)
    a, b = C.c_uint64(0), C.c_uint64(0)
    cloud = np.ascontiguousarray(gold)
    rc = gpu.lib.pclhip_sac_segment_plane(gpu.h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, None, 0, C.byref(p),
                                          coeff.ctypes.data_as(C.POINTER(C.c_float)), None, 0, C.byref(a), None, 0,
                                          C.byref(b), None)
    assert rc == 0 and (a.value, b.value) == (n_in, n_out) and coeff.tobytes() == ref["coefficients"].tobytes()


def test_other_models_and_methods_raise(gpu):
    import pcl_amd
    s = pcl_amd.SACSegmentation(gpu)
    with pytest.raises(NotImplementedError):
        s.setModelType(1)   # SACMODEL_LINE
    with pytest.raises(NotImplementedError):
        s.setMethodType(1)  # SAC_LMEDS
    s.setInputCloud(scene(10))
    with pytest.raises(ValueError):
        s.segment()         # no model type was set


# ---- torch ----------------------------------------------------------------------------------------------------------------------
def test_torch_device_buffers(gpu, gold, gold_refs):
    import torch
    ref = gold_refs[3]
    cloud = torch.from_numpy(gold).cuda()
    ind = torch.arange(0, len(gold), 2, dtype=torch.int32).cuda()
    s = segmenter(gpu, cloud, 0.03, seed=3, optimize=False)
    inl, coeff = s.segment()
    assert inl.is_cuda and inl.dtype == torch.int32 and s.getOutliers().is_cuda
    assert np.array_equal(inl.cpu().numpy(), ref["first_inliers"]) and coeff.tobytes() == ref["coefficients"].tobytes()
    inl2, _ = s.segment()
    assert torch.equal(inl, inl2)
    s.setIndices(ind)
    inl, coeff = s.segment()
    r2 = sac.segment(gold, 0.03, seed=3, optimize=False, indices=ind.cpu().numpy())
    assert np.array_equal(inl.cpu().numpy(), r2["inliers"]) and np.array_equal(s.getOutliers().cpu().numpy(), r2["outliers"])


# ---- the tutorial loop ------------------------------------------------------------------------------------------------------------
def test_tutorial_loop(gpu):
    """cluster_extraction.cpp: take the largest plane away until little is left, then cluster the rest"""
    import pcl_amd
    rng = np.random.default_rng(21)
    n1, n2, blobs = 6000, 3000, (400, 250, 120)
    p1 = np.column_stack([rng.uniform(-2, 2, (n1, 2)), rng.normal(0, 0.002, n1)])                     # z = 0
    p2 = np.column_stack([rng.normal(0, 0.002, n2) + 2.5, rng.uniform(-2, 2, n2), rng.uniform(0.2, 2, n2)])  # x = 2.5
    centres = ((-1.0, -1.0, 0.6), (0.0, 1.0, 0.8), (1.2, -0.5, 1.1))
    parts = [p1, p2] + [rng.normal(0, 0.03, (m, 3)) + np.array(c) for m, c in zip(blobs, centres)]
    cloud = np.ascontiguousarray(np.concatenate(parts), np.float32)
    owner = np.repeat(np.arange(5), [n1, n2] + list(blobs))
    perm = rng.permutation(len(cloud))
    cloud, owner = cloud[perm], owner[perm]
    rest = None
    normals = []
    for step in range(2):
        s = segmenter(gpu, cloud, 0.02, seed=step, indices=rest, max_iterations=100)
        inl, coeff = s.segment()
        assert (owner[inl] == step).mean() > 0.98 and (owner[inl] == step).sum() == (n1, n2)[step]
        normals.append(coeff)
        rest = np.asarray(s.getOutliers())
    assert abs(abs(normals[0][2]) - 1) < 1e-3 and abs(normals[0][3]) < 5e-3           # z = 0
    assert abs(abs(normals[1][0]) - 1) < 1e-3 and abs(abs(normals[1][3]) - 2.5) < 5e-3  # x = 2.5
    assert len(rest) <= sum(blobs) and len(rest) > sum(blobs) - 60
    e = pcl_amd.EuclideanClusterExtraction(gpu)
    e.setInputCloud(cloud)
    e.setIndices(rest)
    e.setClusterTolerance(0.08)
    e.setMinClusterSize(50)
    clusters = e.extract()
    assert len(clusters) == 3
    for c, m, k in zip(clusters, blobs, (2, 3, 4)):
        assert (owner[c] == k).all() and m - 30 <= len(c) <= m
