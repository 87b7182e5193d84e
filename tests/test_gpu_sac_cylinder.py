"""SampleConsensusModelCylinder and RandomSampleConsensus on the device against the numpy restatement
(tests/sac_cylinder_restatement.py, pinned on the reference's own criteria by tests/test_sac_cylinder_restatement.py).  Per
trial of the trace the samples, the coefficient bits, the skip flag, the gate's bit and the count are equal; so are the
winner, the iterations and both lists.  Every case runs twice and the two runs' outputs must be the same bytes.

The float parts of the distance are the restatement's bits; its double parts (acos, sqrt, the blend) are numpy's, so a flag
is pinned only where |distance - threshold| > 64 * 2^-53 * max(threshold, distance), wed against the threshold and a gate
likewise.  Every case asserts FIRST, with the restatement alone, that nothing of its inputs lies inside that band: the
comparison is then exact and complete.

The refit is not compared as bytes: the restatement evaluates, in double at the device's returned float coefficients, the
Gauss-Newton step of the refit's objective, and |step|_inf <= 4 * 2^-23 * max(1, |line_pt|_inf, r) says the device stopped
at the minimum to within the resolution of its float output (rounding alone moves a coordinate by 2^-24 of its magnitude;
the factor covers three coordinates combining).  The inputs are checked on the CPU first: noise <= 1 % of the radius and
the restatement's own optimum, rounded to float, within half the bar.  The selection after the refit is compared exactly,
with the device's refined coefficients fed to the restatement."""
import os

import numpy as np
import pytest

import sac_cylinder_restatement as cy

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NTILE = 2048  # points a block of the cylinder scoring kernel takes per step (sac_cylinder.hpp: SAC_BLOCK * SACC_P)
F = np.float32


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLD, "sac_cylinder_20.npz"))
    return np.ascontiguousarray(g["cloud"], F), np.ascontiguousarray(np.column_stack([g["normals"], np.zeros(20)]), F)


AXIS = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
BASE = np.array([0.1, 0.2, -0.1])
RADIUS = 0.05


def scene(n, seed=0, noise=4e-4, nan_every=97):
    """a cylinder of radius 0.05 on a tilted axis with analytic normals plus small noise (half the points), a plane and
    uniform clutter with random normals, and some NaN records"""
    rng = np.random.default_rng(seed)
    a = AXIS
    e1 = np.cross(a, [1.0, 0, 0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    kind = rng.integers(0, 4, n)  # 0, 1: cylinder; 2: plane; 3: clutter
    phi, h = rng.uniform(0, 2 * np.pi, n), rng.uniform(-0.2, 0.2, n)
    radial = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    pts = BASE + h[:, None] * a + (RADIUS + rng.uniform(-noise, noise, n))[:, None] * radial
    nrm = radial + rng.normal(0, 0.003, (n, 3))
    pl = kind == 2
    pts[pl] = np.column_stack([rng.uniform(-0.3, 0.3, (int(pl.sum()), 2)), np.full(int(pl.sum()), -0.3)])
    nrm[pl] = (0, 0, 1)
    cl = kind == 3
    pts[cl] = rng.uniform(-0.3, 0.3, (int(cl.sum()), 3))
    nrm[cl] = rng.normal(0, 1, (int(cl.sum()), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cloud = np.ascontiguousarray(pts, F)
    normals = np.ascontiguousarray(np.column_stack([nrm, rng.uniform(0, 0.1, n)]), F)
    if nan_every and n > 4:
        cloud[3::nan_every, 1] = np.nan
        normals[5::nan_every, 0] = np.nan
    return cloud, normals


TRUE = np.concatenate([BASE, AXIS, [RADIUS]]).astype(F)


def model_of(gpu, cloud, normals, mk, indices=None):
    import pcl_amd
    m = pcl_amd.SampleConsensusModelCylinder(cloud, indices, gpu)
    m.setInputNormals(normals)
    m.setNormalDistanceWeight(mk.get("ndw", 0.1))
    if "radius_min" in mk or "radius_max" in mk:
        m.setRadiusLimits(mk.get("radius_min", -cy.DBL_MAX), mk.get("radius_max", cy.DBL_MAX))
    if "axis" in mk:
        m.setAxis(mk["axis"])
    m.setEpsAngle(mk.get("eps_angle", 0.0))
    return m


def ransac_of(gpu, cloud, normals, thr, mk, seed=0, max_iterations=10000, probability=0.99, indices=None, batch=0):
    import pcl_amd
    r = pcl_amd.RandomSampleConsensus(model_of(gpu, cloud, normals, mk, indices), thr)
    r.setMaxIterations(max_iterations)
    r.setProbability(probability)
    r.setSeed(seed)
    r.setBatchSize(batch)
    return r


def trace_bytes(tr):
    return b"".join(np.array(t["samples"] + [int(t["skipped"]), int(t["valid"]), t["count"]], np.int64).tobytes() +
                    t["coefficients"].tobytes() for t in tr)


def same_trace(got, ref):
    assert len(got) == len(ref)
    for t, (a, b) in enumerate(zip(got, ref)):
        assert a["samples"] == b["samples"] and a["skipped"] == b["skipped"] and a["valid"] == b["valid"], (t, a, b)
        assert a["count"] == b["count"], (t, a, b)
        ca, cb = a["coefficients"], b["coefficients"]
        nan = np.isnan(cb)  # (the sign of a NaN is not pinned)
        assert np.array_equal(np.isnan(ca), nan) and ca[~nan].tobytes() == cb[~nan].tobytes(), (t, ca, cb)


STAT_KEYS = ("trials", "iterations", "skipped", "best_trial", "best_count", "refined")


def check(gpu, cloud, normals, thr, mk, **kw):
    """computeModel against the restatement, twice: the band empty first, then trace, winner, iterations, lists"""
    model = cy.Model(**mk)
    ref = cy.compute_model(model, cloud, normals, thr, max_iterations=kw.get("max_iterations", 10000),
                           probability=kw.get("probability", 0.99), seed=kw.get("seed", 0), indices=kw.get("indices"))
    assert ref["in_band"] == 0 and ref["gate_band"] == 0
    r = ransac_of(gpu, cloud, normals, thr, mk, **kw)
    found = r.computeModel()
    got = dict(found=found, inliers=np.asarray(r.getInliers()).copy(), coefficients=np.asarray(r.getModelCoefficients()).copy(),
               sample=r.getModel(), stats=r.stats(), trace=r.trace(), ransac=r)
    assert r.computeModel() == found
    assert got["inliers"].tobytes() == np.asarray(r.getInliers()).tobytes() and got["inliers"].dtype == np.int32
    assert got["coefficients"].tobytes() == np.asarray(r.getModelCoefficients()).tobytes() and got["sample"] == r.getModel()
    assert trace_bytes(got["trace"]) == trace_bytes(r.trace())
    assert all(got["stats"][k] == r.stats()[k] for k in STAT_KEYS)
    same_trace(got["trace"], ref["trace"])
    st = got["stats"]
    assert (st["trials"], st["iterations"], st["skipped"], st["best_trial"], st["best_count"]) == \
        (ref["trials"], ref["iterations"], ref["skipped"], ref["best_trial"], ref["best_count"])
    assert found == ref["found"]
    if not found:
        assert len(got["inliers"]) == 0 and len(got["coefficients"]) == 0
        return got, ref
    _, ids = cy.sac.point_set(cloud, kw.get("indices"))
    assert got["coefficients"].tobytes() == ref["coefficients"].tobytes()
    assert got["sample"] == [int(ids[p]) for p in ref["sample"]]
    assert np.array_equal(got["inliers"], ref["inliers"]) and len(got["inliers"]) == ref["best_count"]
    return got, ref


def gn_bar(coeff):
    c = np.asarray(coeff, np.float64)
    return 4.0 * 2.0 ** -23 * max(1.0, float(np.abs(c[:3]).max()), float(c[6]))


def check_refit(cloud, inlier_ids, start, refined, noisy=True):
    """the condition on the inputs on the CPU, then the device's refined coefficients at the minimum.  noisy: the inliers
    lie within 1 % of the radius of the restatement's own optimum (the reference's 20 points do not: their first is 4 % off)"""
    P = np.asarray(cloud, F)[inlier_ids]
    own, _ = cy.refit(P, start)
    assert own is not None and np.abs(cy.gn_step(P, cy.rounded(own))).max() <= 0.5 * gn_bar(own)
    if noisy:
        f, _ = cy.residuals(np.array([0, 0, 0, 0, own[6]]), cy.frame(own, P), P, jac=False)
        assert np.abs(f).max() <= 0.01 * own[6]
    step = np.abs(cy.gn_step(P, refined)).max()
    assert step <= gn_bar(refined), (step, gn_bar(refined))
    assert abs(float(np.linalg.norm(np.asarray(refined, np.float64)[3:6])) - 1.0) < 1e-6


def evaluated(gpu, cloud, normals, thr, mk, coeffs, indices=None):
    """evaluate on the device, twice, against the restatement with the band empty -> counts"""
    ref_cnt, ref_val, in_band, gate_band = cy.evaluate(cy.Model(**mk), cloud, normals, coeffs, thr, indices)
    assert in_band == 0 and gate_band == 0
    m = model_of(gpu, cloud, normals, mk, indices)
    cnt, val = m.evaluate(coeffs, thr)
    cnt2, val2 = m.evaluate(coeffs, thr)
    assert cnt.tobytes() == cnt2.tobytes() and val.tobytes() == val2.tobytes()
    assert np.array_equal(val, ref_val), np.flatnonzero(val != ref_val)
    assert np.array_equal(cnt, ref_cnt), (np.flatnonzero(cnt != ref_cnt)[:8], cnt[:8], ref_cnt[:8])
    return cnt


# ---- the reference's own test, on its 20 points -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fixture_through_ransac(gpu, gold, seed):
    """test_sample_consensus_quadric_models.cpp:452-499 through the two classes"""
    cloud, normals = gold
    got, ref = check(gpu, cloud, normals, 0.03, dict(ndw=0.1), seed=seed)
    assert got["found"] and len(got["sample"]) == 2 and len(got["inliers"]) == 20
    c = got["coefficients"]
    assert len(c) == 7 and abs(c[0] + 0.5) < 1e-3 and abs(c[1] - 1.7) < 1e-3 and abs(c[6] - 0.5) < 1e-3
    m = got["ransac"].model
    assert m.getSampleSize() == 2 and m.getModelSize() == 7
    fine = m.optimizeModelCoefficients(got["inliers"], c)
    assert m.lastOptimize()["refined"] and 0 < m.lastOptimize()["iterations"] <= 100
    assert fine.tobytes() == m.optimizeModelCoefficients(got["inliers"], c).tobytes()
    assert len(fine) == 7 and abs(fine[6] - 0.5) < 1e-3
    check_refit(cloud, got["inliers"], c, fine, noisy=False)
    d = m.getDistancesToModel(fine)
    assert d.dtype == np.float64 and len(d) == 20 and abs(d[0] - 0.020) < 1e-3 and np.abs(d[1:]).max() < 1e-3
    pts, raw, un, ids = cy.point_set(cloud, normals)
    dref = cy.Model(0.1).distances(pts, un, fine)
    assert np.abs(d - dref).max() <= cy.BAND * dref.max()
    assert m.countWithinDistance(fine, 0.021) == 20 and m.countWithinDistance(fine, 0.019) == 19
    assert len(m.selectWithinDistance(fine, 0.021)) == 20
    assert np.array_equal(m.selectWithinDistance(fine, 0.019), np.arange(1, 20))


@pytest.mark.parametrize("optimize", [False, True])
def test_fixture_in_one_call(gpu, gold, optimize):
    """pclhip_sac_cylinder_segment equals computeModel -> optimizeModelCoefficients -> selectWithinDistance as bytes"""
    cloud, normals = gold
    r = ransac_of(gpu, cloud, normals, 0.03, dict(ndw=0.1), seed=1)
    inl, coeff, outl = r.segment(optimize)
    inl2, coeff2, outl2 = r.segment(optimize)
    assert inl.tobytes() == inl2.tobytes() and coeff.tobytes() == coeff2.tobytes() and outl.tobytes() == outl2.tobytes()
    assert r.stats()["refined"] == optimize
    assert r.computeModel()
    c, ids = r.getModelCoefficients(), r.getInliers()
    if optimize:
        c = r.model.optimizeModelCoefficients(ids, c)
        ids = r.model.selectWithinDistance(c, 0.03)
    assert coeff.tobytes() == c.tobytes() and inl.tobytes() == np.asarray(ids).tobytes()
    assert np.array_equal(np.sort(np.concatenate([inl, outl])), np.arange(20))
    want, rest, in_band, gate_band = cy.select(cy.Model(0.1), cloud, normals, coeff, 0.03)
    assert in_band == 0 and np.array_equal(inl, want) and np.array_equal(outl, rest)


# ---- the synthetic scene ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 65, 70, 1025])
def test_evaluate_hypothesis_counts(gpu, H):
    cloud, normals = scene(700, seed=2)
    coeffs = cy.hypotheses(cloud, normals, H, seed=4)
    coeffs[0] = TRUE
    cnt = evaluated(gpu, cloud, normals, 0.002, dict(ndw=0.1), coeffs)
    assert cnt[0] > 250


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, NTILE - 1, NTILE, NTILE + 1, 10000])
def test_point_counts(gpu, n):
    cloud, normals = scene(n, seed=n, nan_every=0 if n < 64 else 97)
    got, ref = check(gpu, cloud, normals, 0.002, dict(ndw=0.1), seed=3, max_iterations=40)
    assert got["found"] or n < 64
    if n < 2:
        assert not got["found"] and got["stats"]["trials"] == 0
    if n >= 63:
        coeffs = np.vstack([TRUE, cy.hypotheses(cloud, normals, 5, seed=1)])
        assert evaluated(gpu, cloud, normals, 0.002, dict(ndw=0.1), coeffs)[0] > n // 3


def test_scene_in_one_call_with_the_refit(gpu):
    n = 3000
    cloud, normals = scene(n, seed=11)
    mk = dict(ndw=0.1)
    got, ref = check(gpu, cloud, normals, 0.002, mk, seed=5, max_iterations=60)
    assert ref["best_count"] > n // 3
    r = got["ransac"]
    inl, coeff, outl = r.segment(True)
    inl2, coeff2, outl2 = r.segment(True)
    assert inl.tobytes() == inl2.tobytes() and coeff.tobytes() == coeff2.tobytes() and outl.tobytes() == outl2.tobytes()
    assert r.stats()["refined"] and all(r.stats()[k] == got["stats"][k] for k in STAT_KEYS[:5])
    check_refit(cloud, got["inliers"], got["coefficients"], coeff)
    assert abs(coeff[6] - RADIUS) < 1e-4 and abs(abs(float(coeff[3:6] @ AXIS)) - 1.0) < 1e-5
    want, rest, in_band, gate_band = cy.select(cy.Model(**mk), cloud, normals, coeff, 0.002)
    assert in_band == 0 and np.array_equal(inl, want) and np.array_equal(outl, rest)
    fine = r.model.optimizeModelCoefficients(got["inliers"], got["coefficients"])
    assert fine.tobytes() == coeff.tobytes()


def test_indices_and_repeats(gpu):
    cloud, normals = scene(1500, seed=6)
    rng = np.random.default_rng(0)
    for ind in (np.arange(0, 1500, 2, dtype=np.int32), rng.permutation(1500).astype(np.int32)[:900],
                rng.integers(0, 1500, 1200).astype(np.int32)):
        got, ref = check(gpu, cloud, normals, 0.002, dict(ndw=0.1), seed=2, max_iterations=40, indices=ind)
        assert got["found"]
        inl, coeff, outl = got["ransac"].segment(False)
        assert np.array_equal(inl, ref["inliers"]) and np.array_equal(outl, ref["outliers"])
        coeffs = np.vstack([TRUE, cy.hypotheses(cloud, normals, 3, seed=1, indices=ind)])
        evaluated(gpu, cloud, normals, 0.002, dict(ndw=0.1), coeffs, indices=ind)
    empty = model_of(gpu, cloud, normals, dict(ndw=0.1), np.zeros(0, np.int32))
    assert empty.countWithinDistance(TRUE, 0.002) == 0 and len(empty.selectWithinDistance(TRUE, 0.002)) == 0


@pytest.mark.parametrize("batch", [0, 1, 7, 1024])
def test_batch_sizes_never_change_a_result(gpu, batch):
    cloud, normals = scene(800, seed=8)
    got, ref = check(gpu, cloud, normals, 0.002, dict(ndw=0.1), seed=9, max_iterations=30, probability=0.999999, batch=batch)
    assert got["stats"]["iterations"] > 7


def test_model_from_a_sample(gpu, gold):
    cloud, normals = gold
    m = model_of(gpu, cloud, normals, dict(ndw=0.1))
    for s in ((1, 2), (2, 1), (0, 19), (7, 7)):
        want, skipped = cy.model_from_samples(cloud[s[0]], cloud[s[1]], normals[s[0]], normals[s[1]])
        got = m.computeModelCoefficients(s)
        assert (got is None) == skipped
        if got is not None:
            assert got.tobytes() == want.tobytes()
    m.setRadiusLimits(0.6, 0.7)
    assert m.computeModelCoefficients((1, 2)) is None and m.getRadiusLimits() == (0.6, 0.7)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(gpu, gold):
    import pcl_amd
    cloud, normals = gold
    m = pcl_amd.SampleConsensusModelCylinder(cloud, None, gpu)
    with pytest.raises(ValueError):
        m.countWithinDistance(TRUE, 0.03)            # no normals
    m.setInputNormals(normals[:19])
    with pytest.raises(ValueError):
        m.countWithinDistance(TRUE, 0.03)            # not one per record
    m.setInputNormals(normals[:, :3])
    with pytest.raises(ValueError):
        m.countWithinDistance(TRUE, 0.03)            # records without the fourth column
    m.setInputNormals(normals)
    m.setEpsAngle(0.1)
    with pytest.raises(pcl_amd.PclHipError, match="axis"):
        m.countWithinDistance(TRUE, 0.03)            # the zero axis with eps_angle > 0
    m.setEpsAngle(0.0)
    m.setRadiusLimits(2.0, 1.0)
    with pytest.raises(pcl_amd.PclHipError, match="radius_min"):
        m.countWithinDistance(TRUE, 0.03)
    m.setRadiusLimits(-cy.DBL_MAX, cy.DBL_MAX)
    with pytest.raises(ValueError):
        m.countWithinDistance(TRUE[:4], 0.03)
    with pytest.raises(ValueError):
        m.computeModelCoefficients((1, 2, 3))
    m.setIndices(np.array([0, 20], np.int32))
    with pytest.raises(pcl_amd.PclHipError, match="outside"):
        m.countWithinDistance(TRUE, 0.03)
    m.setIndices(None)
    r = pcl_amd.RandomSampleConsensus(m, 0.03)
    for bad in (lambda: r.setMaxIterations(-1), lambda: r.setProbability(1.5), lambda: r.setBatchSize(1025)):
        bad()
        with pytest.raises(pcl_amd.PclHipError):
            r.computeModel()
        r.setMaxIterations(50), r.setProbability(0.99), r.setBatchSize(0)
    with pytest.raises(NotImplementedError):
        r.refineModel()
    with pytest.raises(NotImplementedError):
        r.setNumberOfThreads(4)
    with pytest.raises(NotImplementedError):
        pcl_amd.RandomSampleConsensus(object(), 0.03)
    with pytest.raises(NotImplementedError):          # the segmentation classes keep refusing the cylinder
        pcl_amd.SACSegmentationFromNormals(gpu).setModelType(5)
    assert r.computeModel() and len(r.getInliers()) == 20


# ---- torch --------------------------------------------------------------------------------------------------------------
def test_torch_device_buffers(gpu):
    import torch
    cloud, normals = scene(2500, seed=12)
    ref = cy.compute_model(cy.Model(0.1), cloud, normals, 0.002, max_iterations=40, seed=3)
    assert ref["in_band"] == 0 and ref["found"]
    r = ransac_of(gpu, torch.from_numpy(cloud).cuda(), torch.from_numpy(normals).cuda(), 0.002, dict(ndw=0.1), seed=3,
                  max_iterations=40)
    assert r.computeModel()
    inl = r.getInliers()
    assert inl.is_cuda and inl.dtype == torch.int32 and np.array_equal(inl.cpu().numpy(), ref["inliers"])
    assert r.getModelCoefficients().tobytes() == ref["coefficients"].tobytes()
    ind = torch.arange(0, len(cloud), 2, dtype=torch.int32).cuda()
    r.model.setIndices(ind)
    r2 = cy.compute_model(cy.Model(0.1), cloud, normals, 0.002, max_iterations=40, seed=3, indices=ind.cpu().numpy())
    assert r2["in_band"] == 0
    inl, coeff, outl = r.segment(False)
    assert inl.is_cuda and outl.is_cuda
    assert np.array_equal(inl.cpu().numpy(), r2["inliers"]) and np.array_equal(outl.cpu().numpy(), r2["outliers"])
    sel = r.model.selectWithinDistance(coeff, 0.002)
    assert sel.is_cuda and torch.equal(sel, inl)
    fine = r.model.optimizeModelCoefficients(inl, coeff)
    assert r.model.lastOptimize()["refined"]
    assert fine.tobytes() == r.model.optimizeModelCoefficients(inl.cpu().numpy(), coeff).tobytes()
