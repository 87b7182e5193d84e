"""The point-to-point solve where it runs on or behind the device, on planes and lines (tests/solver_reference.py: the regimes,
the fp64 reference and what is asserted of every solve; tests/test_solver_regimes.py holds the host solver to the same over
every regime):
  * pclhip_estimate_rigid_transformation: device sums feed the host solve
  * the device loop's own instantiation of cf::rotation_from_sigma (icp_solve_step), one iteration over known pairs, against
    the reference and against its host twin (tests/test_gpu_loop.py: icp.iterate + icp.solve)
  * align() end to end: the final transformation, a float product of one solve per iteration, is still a rotation, and the
    source lands on its partners.  hasConverged() alone is asserted nowhere: it was True with det R = 0.4."""
import ctypes as C

import numpy as np
import pytest

import solver_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


RIGID_CASES = (["ball"] + ["slab %s seed %d" % (th, s) for th in ("1e-07", "0") for s in (0, 1, 2)]
               + ["rod 0 seed 0", "mirror z -> -z", "three pairs", "coincident points", "plane x 1e+10", "plane + 10000"])


@pytest.fixture(scope="module")
def by_name():
    return {c.name: c for c in sr.cases()}


@pytest.mark.parametrize("name", RIGID_CASES, ids=[n.replace(" ", "_") for n in RIGID_CASES])
def test_estimate_rigid_transformation(gpu, by_name, name):
    import pcl_amd
    case = by_name[name]
    sr.in_regime(case)
    T, sums = pcl_amd.estimateRigidTransformation(gpu, pcl_amd.POINT_TO_POINT, case.src, case.tgt)
    assert sums[28] == len(case.src)
    j = sr.check(T, case)
    print("%s: orth %.3g B, excess %.3g B M, max|T - K| %.3g, max|R - R_K| %.3g (determined: %s)"
          % (name, j["orth"] / sr.B, j["excess"] / sr.B, j["diff"], j["diff_R"], j["determined"]))


# ---- the device loop over known pairs -------------------------------------------------------------------------------------------
PLANE_H, LINE_H = 0.05, 0.005


def flat_scan(shape, seed):
    """-> (target, source, partners, h): the target is a 40 x 40 in-plane lattice of spacing h (a 400-point line of spacing h),
    jittered in the plane (along the line) by at most h/8 and tilted; the source is every second target point under an
    in-plane rigid motion (a rigid motion about the centroid, for the line) that displaces no point by more than h/4."""
    rng = np.random.default_rng([91, seed, shape == "line"])
    if shape == "plane":
        h = PLANE_H
        i, j = np.meshgrid(np.arange(40) - 19.5, np.arange(40) - 19.5, indexing="ij")
        p = np.stack([i.ravel() * h, j.ravel() * h, np.zeros(1600)], axis=1)
        p[:, :2] += rng.uniform(-h / 8, h / 8, (1600, 2))
        axis, reach = np.array([0.0, 0.0, 1.0]), 20 * h * np.sqrt(2) + h
        shift = np.array([0.6, -0.8, 0.0]) * h / 10
    else:
        h = LINE_H
        p = np.zeros((400, 3))
        p[:, 0] = (np.arange(400) - 199.5) * h + rng.uniform(-h / 8, h / 8, 400)
        axis, reach = rng.normal(size=3), 200 * h + h
        shift = np.array([1.0, 0.0, 0.0]) * h / 10
    tilt = sr.random_rotation(rng)
    tgt = np.ascontiguousarray(p @ tilt.T, np.float32)
    partners = np.arange(0, len(tgt), 2)
    G = tilt @ sr.rotation(axis, (h / 8) / reach) @ tilt.T  # a turn of at most h/8 at the rim, then a slide of h/10
    t64 = tgt[partners].astype(np.float64)
    c = t64.mean(0)
    src = np.ascontiguousarray((t64 - c) @ G.T + c + tilt @ shift, np.float32)
    assert np.linalg.norm(src.astype(np.float64) - t64, axis=1).max() <= h / 4
    # brute force: every nearest neighbour is the true partner
    d2 = ((src.astype(np.float64)[:, None, :] - tgt.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    assert np.array_equal(d2.argmin(1), partners)
    return tgt, src, partners, h


def make_icp(gpu, tgt, src, h, iterations):
    import pcl_amd
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setMaximumIterations(iterations)
    icp.setMaxCorrespondenceDistance(h)
    return icp


@pytest.mark.parametrize("shape", ["plane", "line"])
def test_one_iteration_of_the_device_loop(gpu, shape):
    tgt, src, partners, h = flat_scan(shape, 0)
    case = sr.Case(shape, "slab" if shape == "plane" else "rod", src, tgt[partners], "unit", 0.0)
    sr.in_regime(case)
    icp = make_icp(gpu, tgt, src, h, 1)
    icp.align()
    assert icp.nr_iterations_ == 1
    T = icp.getLastIncrementalTransformation()
    j = sr.check(T, case)
    print("%s: orth %.3g B, excess %.3g B M, max|T - K| %.3g" % (shape, j["orth"] / sr.B, j["excess"] / sr.B, j["diff"]))
    assert np.array_equal(icp.getFinalTransformation(), T)
    # the host twin: the same kernels' sums, the solve on the host
    host = make_icp(gpu, tgt, src, h, 1)
    host.reset()
    sums = host.iterate(np.eye(4, dtype=np.float32))
    assert sums[28] == len(src)
    Th = host.solve(sums)
    sr.check(Th, case)
    assert np.abs(T - Th).max() <= 2e-6


@pytest.mark.parametrize("symmetric", [False, True])
def test_exactly_singular_normal_system_ends_the_loop_as_its_host_twin(gpu, symmetric):
    """Point-to-plane and symmetric ICP against the plane z = 0 with every normal (0, 0, 1): the 6 x 6 is exactly singular, the
    first solve returns NaN (tests/test_solver_regimes.py pins that for the host call), every point of the next search is
    non-finite and the alignment ends without correspondences -- on the device as in the host-driven loop."""
    import pcl_amd
    from pcl_amd import _lib
    from test_gpu_loop import _host_loop_align
    rng = np.random.default_rng(17)
    tgt = np.zeros((1600, 4), np.float32)
    tgt[:, :2] = (np.stack(np.meshgrid(np.arange(40) - 19.5, np.arange(40) - 19.5, indexing="ij"), -1).reshape(-1, 2) * PLANE_H
                  + rng.uniform(-PLANE_H / 8, PLANE_H / 8, (1600, 2)))
    tgt[:, 3] = 1
    nrm = np.zeros((1600, 3), np.float32)
    nrm[:, 2] = 1
    src = tgt[::2].copy()
    src[:, :3] += np.float32([0.004, -0.003, 0.01])

    def make():
        icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
        icp.setInputTarget(tgt)
        icp.setTargetNormals(nrm)
        icp.setInputSource(src)
        if symmetric:
            icp.setSourceNormals(nrm[::2].copy())
            icp.setUseSymmetricObjective(True)
        icp.setMaximumIterations(5)
        icp.setMaxCorrespondenceDistance(PLANE_H)
        return icp
    dev, host = make(), make()
    host._ensure()
    conv = _lib.ConvergenceState()
    _lib.load().pclhip_convergence_init(C.byref(conv))
    dev.align()
    b = _host_loop_align(host, conv)
    assert np.isnan(b["last"][:3]).all() and np.array_equal(b["last"][3], [0, 0, 0, 1])
    assert (b["it"], _lib.CONVERGENCE_STATES[b["state"]], b["conv"]) == (1, "NO_CORRESPONDENCES", False)
    assert (dev.nr_iterations_, dev.getConvergenceState(), dev.hasConverged()) == (1, "NO_CORRESPONDENCES", False)
    assert np.isnan(dev.getLastIncrementalTransformation()[:3]).all() and np.isnan(dev.getFinalTransformation()[:3]).all()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", ["plane", "line"])
def test_align_end_to_end(gpu, shape, seed):
    tgt, src, partners, h = flat_scan(shape, seed)
    icp = make_icp(gpu, tgt, src, h, 30)
    icp.align()
    k = icp.nr_iterations_
    assert 1 <= k <= 30
    T = icp.getFinalTransformation().astype(np.float64)
    assert np.isfinite(T).all() and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    orth = np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max()
    rms = sr.rms_residual(T, src, tgt[partners])
    print("%s seed %d: %d iterations, max|R^T R - I| = %.3g B (bound %d B), rms to the partners %.3g h"
          % (shape, seed, k, orth / sr.B, k + 1, rms / h))
    assert orth <= (k + 1) * sr.B
    assert rms < h / 100
