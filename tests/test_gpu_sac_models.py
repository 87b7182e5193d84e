"""The constrained planes of SACSegmentation and the planes of SACSegmentationFromNormals on the device against the numpy
restatement (tests/sac_models_restatement.py, pinned on the reference's own criteria by
tests/test_sac_models_restatement.py).  Per trial of the trace the samples, the coefficient bits, the skip flag, the gate's
bit and the count are equal; so are the winner, the iterations and both lists.  Every case runs twice and the two runs'
outputs must be the same bytes.

The float parts of the distance are the restatement's bits; its double parts (acos, the blend) are numpy's, so a flag is
pinned only where |distance - threshold| > 64 * 2^-53 * max(threshold, distance), and a gate likewise.  Every case asserts
FIRST, with the restatement alone, that no pair and no hypothesis of its inputs lies inside that band: the comparison is
then exact and complete."""
import ctypes as C
import os

import numpy as np
import pytest

import sac_models_restatement as sm
import sac_restatement as sac

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NTILE = 2048  # points a block of the normal-plane scoring kernel takes per step (sac_models.hpp: SAC_BLOCK * SACN_P)
FLOOR = (-0.8964, -0.5868, -1.208)  # the golden cloud's plane, up to scale (the reference's expectation)
ALONG = (0.5477, -0.8367, 0.0)      # a direction inside it, of unit length (models 15 and 16 take the axis as given)
SETTINGS = [(ndw, thr) for ndw in (0.01, 0.1, 0.3) for thr in (0.03, 0.01)]
MODELS = {  # parameters that leave the golden cloud's plane valid
    0: dict(model_type=0),
    9: dict(model_type=9, axis=FLOOR, eps_angle=0.1),
    15: dict(model_type=15, axis=ALONG, eps_angle=0.1),
    11: dict(model_type=11, ndw=0.1),
    16: dict(model_type=16, axis=FLOOR, eps_angle=0.1, ndw=0.1),
}


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def gold():
    cloud = np.ascontiguousarray(np.load(os.path.join(GOLD, "sac_plane_radius.npz"))["cloud"][:, :3], np.float32)
    return cloud, np.load(os.path.join(GOLD, "sac_plane_normals.npz"))["normals"]


@pytest.fixture(scope="module")
def gold_models(gold):
    """70 hypotheses of the golden cloud: one full group of 64 and a tail"""
    return sm.hypotheses(gold[0], 70, seed=1)


def scene(n, seed=0, clutter=0.3):
    """a tilted plane with noise and uniform clutter and normals around the plane's with curvatures in [0, 0.1)"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n, 2))
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.5 + rng.normal(0, 0.004, n)
    off = rng.random(n) < clutter
    z[off] = rng.uniform(-1, 2, int(off.sum()))
    nrm = np.array([0.3, -0.2, -1.0]) + rng.normal(0, 0.05, (n, 3))
    nrm[off] = rng.normal(0, 1, (int(off.sum()), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    normals = np.column_stack([nrm, rng.uniform(0, 0.1, n)])
    return np.ascontiguousarray(np.column_stack([xy, z]), np.float32), np.ascontiguousarray(normals, np.float32)


def segmenter(gpu, cloud, normals, thr, mk, seed=0, max_iterations=50, probability=0.99, optimize=True, indices=None, batch=0,
              plain=False):
    """mk: the keywords of sm.Model.  plain: pcl_amd.SACSegmentation (models 0, 9, 15), else SACSegmentationFromNormals"""
    import pcl_amd
    s = pcl_amd.SACSegmentation(gpu) if plain else pcl_amd.SACSegmentationFromNormals(gpu)
    s.setModelType(mk.get("model_type", 0))
    s.setMethodType(pcl_amd.SAC_RANSAC)
    s.setDistanceThreshold(thr)
    s.setMaxIterations(max_iterations)
    s.setProbability(probability)
    s.setOptimizeCoefficients(optimize)
    s.setSeed(seed)
    s.setBatchSize(batch)
    s.setInputCloud(cloud)
    s.setIndices(indices)
    if "axis" in mk:
        s.setAxis(mk["axis"])
    s.setEpsAngle(mk.get("eps_angle", 0.0))
    if not plain:
        s.setInputNormals(normals)
        s.setNormalDistanceWeight(mk.get("ndw", 0.1))
        s.setDistanceFromOrigin(mk.get("distance_from_origin", 0.0))
    s.m.eps_dist = mk.get("eps_dist", 0.0)  # (the classes have no setter for it: the C interface's field)
    return s


def trace_bytes(tr):
    return b"".join(np.array(t["samples"] + [int(t["skipped"]), int(t["valid"]), t["count"]], np.int64).tobytes() +
                    t["coefficients"].tobytes() for t in tr)


def run(gpu, cloud, normals, thr, mk, **kw):
    """segment twice: the same bytes -> dict(inliers, coefficients, outliers, stats, trace, seg)"""
    s = segmenter(gpu, cloud, normals, thr, mk, **kw)
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
        assert a["samples"] == b["samples"] and a["skipped"] == b["skipped"] and a["valid"] == b["valid"], (t, a, b)
        assert a["count"] == b["count"], (t, a, b)
        ca, cb = a["coefficients"], b["coefficients"]
        nan = np.isnan(cb)  # (the sign of a NaN is not pinned)
        assert np.array_equal(np.isnan(ca), nan) and ca[~nan].tobytes() == cb[~nan].tobytes(), (t, ca, cb)


def check(gpu, cloud, normals, thr, mk, **kw):
    """the device against the restatement: the band empty first, then trace, winner, iterations, lists.  With the refit the
    refined selection is the restatement's on the DEVICE's refined coefficients (the refit is the plane's: its sums differ
    from the reference's float sums by design, tests/test_gpu_sac.py measures them), its band empty as well."""
    model = sm.Model(**mk)
    ref = sm.segment(model, cloud, normals, thr, max_iterations=kw.get("max_iterations", 50),
                     probability=kw.get("probability", 0.99), seed=kw.get("seed", 0), indices=kw.get("indices"))
    assert ref["in_band"] == 0 and ref["gate_band"] == 0
    got = run(gpu, cloud, normals, thr, mk, **kw)
    same_trace(got["trace"], ref["trace"])
    st = got["stats"]
    assert (st["trials"], st["iterations"], st["skipped"], st["best_trial"], st["best_count"]) == \
        (ref["trials"], ref["iterations"], ref["skipped"], ref["best_trial"], ref["best_count"])
    _, ids = sac.point_set(cloud, kw.get("indices"))
    if not ref["found"]:
        assert len(got["inliers"]) == 0 and len(got["coefficients"]) == 0 and np.array_equal(got["outliers"], ids)
        return got, ref
    if st["refined"]:
        assert kw.get("optimize", True) and ref["best_count"] > 3
        inl, outl, band = sm.select(model, cloud, normals, got["coefficients"], thr, kw.get("indices"))
        assert band == 0
    else:
        assert got["coefficients"].tobytes() == ref["coefficients"].tobytes()
        inl, outl = ref["first_inliers"], ref["first_outliers"]
        assert len(inl) == ref["best_count"]  # the first selection counts exactly the winner's score
    assert np.array_equal(got["inliers"], inl) and np.array_equal(got["outliers"], outl)
    assert st["n_inliers"] == len(inl) and st["n_outliers"] == len(outl)
    return got, ref


def evaluated(gpu, cloud, normals, thr, mk, coeffs, indices=None):
    """countWithinDistance on the device, twice, against the restatement with its band empty -> the counts"""
    ev = sm.evaluate(sm.Model(**mk), cloud, normals, coeffs, thr, indices)
    assert ev["in_band"] == 0 and ev["gate_band"] == 0
    s = segmenter(gpu, cloud, normals, thr, mk, indices=indices)
    cnt, valid = s.evaluate(coeffs)
    cnt2, valid2 = s.evaluate(coeffs)
    assert cnt.dtype == np.uint32 and cnt.tobytes() == cnt2.tobytes() and valid.tobytes() == valid2.tobytes()
    assert valid.tolist() == ev["valid"]
    assert cnt.tolist() == ev["counts"]
    return cnt


# ---- the scoring pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndw,thr", SETTINGS)
def test_normal_plane_counts(gpu, gold, gold_models, ndw, thr):
    cloud, normals = gold
    cnt = evaluated(gpu, cloud, normals, thr, dict(model_type=11, ndw=ndw), gold_models)
    assert cnt.max() > 50
    one = evaluated(gpu, cloud, normals, thr, dict(model_type=11, ndw=ndw), gold_models[int(cnt.argmax())][None, :])
    assert one.tolist() == [int(cnt.max())]


@pytest.mark.parametrize("model", [9, 15, 16])
def test_gated_counts(gpu, gold, gold_models, model):
    cloud, normals = gold
    cnt = evaluated(gpu, cloud, normals, 0.03, MODELS[model], gold_models)
    valid = sm.Model(**MODELS[model]).gate(gold_models)[0]
    assert 0 < valid.sum() < len(valid) and not cnt[~valid].any() and cnt[valid].max() > 2000


# ---- segment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("model", [0, 9, 15, 11, 16])
def test_segment(gpu, gold, model, subset, optimize):
    cloud, normals = gold
    ind = np.random.default_rng(model).permutation(np.arange(0, len(cloud), 2, dtype=np.int32)).astype(np.int32) if subset else None
    got, ref = check(gpu, cloud, normals, 0.03, MODELS[model], seed=3, indices=ind, optimize=optimize)
    assert ref["found"] and len(got["inliers"]) > (900 if subset else 1800) and got["stats"]["refined"] == optimize
    bad = np.nonzero(np.isnan(normals).any(axis=1))[0]
    if model in (11, 16):  # a NaN normal or curvature: never an inlier
        assert not np.isin(bad, got["inliers"]).any()
    if model in (0, 9, 15):  # ... and the plain class gives the same bytes
        p = run(gpu, cloud, None, 0.03, MODELS[model], seed=3, indices=ind, optimize=optimize, plain=True)
        assert p["inliers"].tobytes() == got["inliers"].tobytes() and p["coefficients"].tobytes() == got["coefficients"].tobytes()
        assert trace_bytes(p["trace"]) == trace_bytes(got["trace"])


def test_reference_criterion(gpu, gold):
    """SampleConsensusModelNormalPlane, RANSAC (test_sample_consensus_plane_models.cpp:319-332): ndw 0.01, threshold 0.03"""
    cloud, normals = gold
    for optimize in (False, True):
        got, ref = check(gpu, cloud, normals, 0.03, dict(model_type=11, ndw=0.01), seed=1, max_iterations=1000, optimize=optimize)
        c = got["coefficients"].astype(np.float64)
        assert len(got["inliers"]) > 2000 and np.abs(c[:3] / c[3] - np.array(FLOOR)).max() < 0.1


def test_plane_through_the_new_entry_point(gpu, gold):
    """model 0 through pclhip_sac_segment_model gives the bytes of pclhip_sac_segment_plane"""
    import pcl_amd
    cloud, normals = gold
    for optimize in (False, True):
        new = run(gpu, cloud, normals, 0.03, MODELS[0], seed=2, optimize=optimize)
        old = run(gpu, cloud, None, 0.03, MODELS[0], seed=2, optimize=optimize, plain=True)
        assert not old["seg"]._through_model() and new["seg"]._through_model()
        for k in ("inliers", "outliers", "coefficients"):
            assert new[k].tobytes() == old[k].tobytes()
        assert trace_bytes(new["trace"]) == trace_bytes(old["trace"]) and all(t["valid"] != t["skipped"] for t in new["trace"])
        ref = sac.segment(cloud, 0.03, seed=2, optimize=False)
        assert [t["count"] for t in new["trace"]] == [t["count"] for t in ref["trace"]]
    # ... and without normals, through the C interface
    p = pcl_amd._lib.SacPlaneParams()
    gpu.lib.pclhip_sac_plane_params_default(C.byref(p))
    p.distance_threshold, p.seed, p.optimize_coefficients = 0.03, 2, 1
    m = pcl_amd._lib.SacModelParams()
    gpu.lib.pclhip_sac_model_params_default(C.byref(m))
    assert (m.model_type, list(m.axis), m.eps_angle, m.normal_distance_weight, m.distance_from_origin, m.eps_dist) == \
        (0, [0.0, 0.0, 0.0], 0.0, 0.1, 0.0, 0.0)
    coeff = np.zeros(4, np.float32)
    a, b = C.c_uint64(0), C.c_uint64(0)
    inl = np.zeros(len(cloud), np.int32)
    rc = gpu.lib.pclhip_sac_segment_model(gpu.h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, None, 0, None, 0, C.byref(p),
                                          C.byref(m), coeff.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(inl.ctypes.data),
                                          len(inl), C.byref(a), None, 0, C.byref(b), None)
    assert rc == 0 and coeff.tobytes() == old["coefficients"].tobytes() and inl[:a.value].tobytes() == old["inliers"].tobytes()


# ---- gates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [9, 15, 16])
def test_axis_outside_the_cone(gpu, gold, model):
    """the axis turned by a right angle: every trial fails the gate -> no model, every point left over, every trial an
    iteration and none skipped; with eps_angle 0 the gate is off"""
    cloud, normals = gold
    mk = dict(MODELS[model], axis=ALONG if model != 15 else FLOOR, eps_angle=0.02)
    got, ref = check(gpu, cloud, normals, 0.03, mk, seed=4, max_iterations=40)
    assert not ref["found"] and got["stats"]["iterations"] == 41 and got["stats"]["skipped"] == 0
    assert got["stats"]["best_trial"] == -1 and len(got["outliers"]) == len(cloud) and len(got["trace"]) == 41
    assert all(not t["valid"] and not t["skipped"] and t["count"] == 0 for t in got["trace"])
    off, _ = check(gpu, cloud, normals, 0.03, dict(mk, eps_angle=0.0), seed=4)
    free, _ = check(gpu, cloud, normals, 0.03, dict(model_type=11 if model == 16 else 0), seed=4)
    assert trace_bytes(off["trace"]) == trace_bytes(free["trace"]) and off["inliers"].tobytes() == free["inliers"].tobytes()


def test_ten_coplanar_points(gpu):
    """test_sample_consensus_plane_models.cpp:335-397: 10 / 10 / 0 inliers, whatever the draws"""
    import math
    rng = np.random.default_rng(0)
    cloud = np.column_stack([rng.integers(-100, 100, (10, 2)), np.zeros(10)]).astype(np.float32)
    normals = np.tile(np.array([[0, 0, 1, 0]], np.float32), (10, 1))
    eps, tilt = 0.01, 0.001
    axes = [(0, 0, 1), (0, math.sin(eps * (1 - tilt)), math.cos(eps * (1 - tilt))),
            (0, math.sin(eps * (1 + tilt)), math.cos(eps * (1 + tilt)))]
    got = [len(check(gpu, cloud, normals, 0.03, dict(model_type=16, axis=a, eps_angle=eps), seed=1, optimize=False)[0]["inliers"])
           for a in axes]
    assert got == [10, 10, 0]


def test_eps_dist(gpu, gold, gold_models):
    """the distance gate of SACMODEL_NORMAL_PARALLEL_PLANE: the classes never set it, the C interface does"""
    cloud, normals = gold
    d = float(-gold_models[0][3])
    mk = dict(model_type=16, distance_from_origin=d, eps_dist=0.2)
    cnt = evaluated(gpu, cloud, normals, 0.03, mk, gold_models)
    valid = sm.Model(**mk).gate(gold_models)[0]
    assert valid[0] and 0 < valid.sum() < len(valid) and not cnt[~valid].any()
    got, ref = check(gpu, cloud, normals, 0.03, dict(mk, axis=FLOOR, eps_angle=0.1), seed=3)
    assert any(not t["valid"] for t in got["trace"])
    # the class's setter alone constrains nothing
    a = run(gpu, cloud, normals, 0.03, dict(model_type=16, distance_from_origin=d), seed=3)
    b = run(gpu, cloud, normals, 0.03, dict(model_type=16), seed=3)
    assert trace_bytes(a["trace"]) == trace_bytes(b["trace"])


def test_refit_leaves_the_cone(gpu, gold):
    """the winner passes the gate, the refined plane does not: no inliers, the refined coefficients all the same"""
    cloud, _ = gold
    found = None
    for seed in (1, 2, 3, 4):
        found = sm.tilting_axis(cloud, 0.03, 0.05, seed=seed)
        if found is not None:
            break
    assert found is not None
    model, ref = found
    mk = dict(model_type=9, axis=model.axis, eps_angle=model.eps_angle)
    got = run(gpu, cloud, None, 0.03, mk, seed=seed, optimize=True, plain=True)
    same_trace(got["trace"], ref["trace"])
    assert got["stats"]["refined"] and got["stats"]["best_count"] == ref["best_count"] > 2000
    assert len(got["inliers"]) == 0 and len(got["outliers"]) == len(cloud)
    assert not model.valid(got["coefficients"]) and model.valid(ref["coefficients"])
    assert np.abs(got["coefficients"] - ref["refined"]).max() < 1e-4 and got["coefficients"].tobytes() != ref["coefficients"].tobytes()
    keep, _ = check(gpu, cloud, None, 0.03, mk, seed=seed, optimize=False, plain=True)
    assert len(keep["inliers"]) == ref["best_count"]


# ---- normals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["zero", "flat", "ndw0", "ndw1", "antiparallel", "weights", "inf"])
def test_normals(gpu, gold, gold_models, case):
    cloud, normals = gold
    nrm = normals.copy()
    ndw, models = 0.1, gold_models[:16]
    ok = ~np.isnan(normals).any(axis=1)
    if case == "zero":            # a normal of length 0 stays 0 (Eigen's normalized()): its angle is pi / 2
        nrm[::3, :3] = 0.0
    elif case == "flat":          # curvature 1: weight 0, the distance is the Euclidean one
        nrm[:, 3] = 1.0
    elif case == "ndw0":
        ndw = 0.0
    elif case == "ndw1":          # the angle alone
        ndw = 1.0
    elif case == "antiparallel":  # the fold: min(a, pi - a)
        nrm[::2, :3] *= -1.0
    elif case == "weights":       # curvatures that put the weight outside [0, 1]: no screen, the exact path
        nrm[::4, 3], nrm[1::4, 3] = -20.0, 2.0
    elif case == "inf":
        nrm[::5, 0], nrm[1::5, 3], nrm[2::5, 3] = np.inf, np.inf, -np.inf
    thr = 0.2 if case == "ndw1" else 0.03
    mk = dict(model_type=11, ndw=ndw)
    cnt = evaluated(gpu, cloud, nrm, thr, mk, models)
    assert cnt.max() > 100
    if case in ("flat", "ndw0"):  # ... which the plane model's flags equal on the records that have a normal
        plane = [sac.count_within(cloud[ok], m, thr) for m in models]
        assert cnt.tolist() == plane
    got, _ = check(gpu, cloud, nrm, thr, mk, seed=5)
    assert not np.isin(np.nonzero(~ok)[0], got["inliers"]).any()


# ---- sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, NTILE - 1, NTILE, NTILE + 1, 10000])
def test_point_counts(gpu, n):
    cloud, normals = scene(n, seed=n)
    thr = 0.03 if n > 4 else 10.0
    got, ref = check(gpu, cloud, normals, thr, dict(model_type=11, ndw=0.1), seed=n)
    assert ref["found"]
    models = np.stack([t["coefficients"] for t in ref["trace"] if not t["skipped"]])
    cnt = evaluated(gpu, cloud, normals, thr, dict(model_type=11, ndw=0.1), models)
    assert cnt.tolist() == [t["count"] for t in ref["trace"] if not t["skipped"]]


def test_fewer_than_three_points(gpu):
    cloud, normals = scene(3)
    for n in (0, 1, 2):
        got = run(gpu, cloud[:n].reshape(n, 3), normals[:n].reshape(n, 4), 1.0, dict(model_type=11))
        assert len(got["inliers"]) == 0 and len(got["coefficients"]) == 0 and got["outliers"].tolist() == list(range(n))
        assert got["stats"]["best_trial"] == -1 and got["stats"]["trials"] == 0 and got["trace"] == []


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(gpu, gold):
    import pcl_amd
    cloud, normals = gold
    plain = pcl_amd.SACSegmentation(gpu)
    for t in (11, 16):  # the reference's SACSegmentation builds no model with normals
        with pytest.raises(ValueError):
            plain.setModelType(t)
    for s in (plain, pcl_amd.SACSegmentationFromNormals(gpu)):
        with pytest.raises(NotImplementedError):
            s.setModelType(1)   # SACMODEL_LINE
        with pytest.raises(NotImplementedError):
            s.setModelType(5)   # SACMODEL_CYLINDER
    s = segmenter(gpu, cloud, None, 0.03, dict(model_type=11))
    with pytest.raises(ValueError):
        s.segment()             # no normals
    s.setInputNormals(normals[:-1])
    with pytest.raises(ValueError):
        s.segment()             # not one per record
    for t in (9, 15, 16):       # an angle without an axis
        with pytest.raises(pcl_amd._lib.PclHipError) as ei:
            segmenter(gpu, cloud, normals, 0.03, dict(model_type=t, eps_angle=0.1)).segment()
        assert ei.value.status == -1 and "axis" in str(ei.value)
        segmenter(gpu, cloud, normals, 0.03, dict(model_type=t)).segment()  # eps_angle 0 needs none
    # the C interface: a model type it does not know, a normal model without normals
    p = pcl_amd._lib.SacPlaneParams()
    gpu.lib.pclhip_sac_plane_params_default(C.byref(p))
    m = pcl_amd._lib.SacModelParams()
    gpu.lib.pclhip_sac_model_params_default(C.byref(m))
    coeff = np.zeros(4, np.float32)
    a = C.c_uint64(0)
    for t, nptr in ((1, C.c_void_p(normals.ctypes.data)), (17, C.c_void_p(normals.ctypes.data)), (11, None), (16, None)):
        m.model_type = t
        rc = gpu.lib.pclhip_sac_segment_model(gpu.h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, nptr, 16, None, 0, C.byref(p),
                                              C.byref(m), coeff.ctypes.data_as(C.POINTER(C.c_float)), None, 0, C.byref(a), None,
                                              0, None, None)
        assert rc == -1 and a.value == 0  # PCLHIP_ERR_INVALID
        cnt = np.zeros(1, np.uint32)
        rc = gpu.lib.pclhip_sac_model_evaluate(gpu.h, C.c_void_p(cloud.ctypes.data), len(cloud), 12, nptr, 16, None, 0, 0.03,
                                               C.byref(m), coeff.ctypes.data_as(C.POINTER(C.c_float)), 1,
                                               C.c_void_p(cnt.ctypes.data), None)
        assert rc == -1


# ---- torch --------------------------------------------------------------------------------------------------------------
def test_torch_device_buffers(gpu, gold):
    import torch
    cloud, normals = gold
    mk = dict(model_type=16, axis=FLOOR, eps_angle=0.1, ndw=0.1)
    ref = sm.segment(sm.Model(**mk), cloud, normals, 0.03, seed=3)
    assert ref["in_band"] == 0 and ref["gate_band"] == 0
    ind = torch.arange(0, len(cloud), 2, dtype=torch.int32).cuda()
    s = segmenter(gpu, torch.from_numpy(cloud).cuda(), torch.from_numpy(normals).cuda(), 0.03, mk, seed=3, optimize=False)
    inl, coeff = s.segment()
    assert inl.is_cuda and inl.dtype == torch.int32 and s.getOutliers().is_cuda
    assert np.array_equal(inl.cpu().numpy(), ref["first_inliers"]) and coeff.tobytes() == ref["coefficients"].tobytes()
    inl2, _ = s.segment()
    assert torch.equal(inl, inl2)
    s.setIndices(ind)
    inl, coeff = s.segment()
    r2 = sm.segment(sm.Model(**mk), cloud, normals, 0.03, seed=3, indices=ind.cpu().numpy())
    assert r2["in_band"] == 0
    assert np.array_equal(inl.cpu().numpy(), r2["first_inliers"]) and np.array_equal(s.getOutliers().cpu().numpy(), r2["first_outliers"])
