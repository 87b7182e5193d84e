"""SACSegmentation (planes, RANSAC) off the easy path, with the machinery of tests/test_gpu_sac.py (check / run /
same_trace: trace, winner, iterations and both lists bit for bit against tests/sac_restatement.py, every case twice, the
two runs the same bytes): a cloud large enough that every block of the scoring kernel takes a second tile, the lists cross
the scan's carry and the refit's grid strides; the refit's accuracy at a size, an offset and a scale where its bar means
something; samples around the 1e-5 skip test; coordinates where the order of the four-term sum decides counts;
overflowing coordinates; the stopping rule's edges through the device path; the trace's cap; records wider than 12 bytes.

Instability cap: 0, as in tests/test_gpu_sac.py.  sac_restatement.unstable flags every scored trial of the shifted and of
the full-grid cloud (some point always lies within a few ulps of the threshold there) -- which is why they are here: no
trial is excluded from the bitwise comparison."""
import numpy as np
import pytest

import sac_restatement as sac
from test_gpu_sac import TILE, check, fit_distance, float64_fit, run, same_trace, scene, trace_bytes

pytestmark = pytest.mark.gpu
SCAN_CARRY = 1024 * 4096   # elements beyond which the scan's top kernel carries (device_scan.hpp)
MOMENT_GRID = 1024 * 256   # inliers beyond which the refit's moments kernel strides (sac.hpp: SAC_MOMENT_BLOCKS * SAC_BLOCK)
TRACE_MAX = 65536          # records the trace keeps (sac.hpp: SAC_TRACE_MAX)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def models_of(trace):
    return np.stack([t["coefficients"] for t in trace])


# ---- 1. every block takes a second tile ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    """A block of the scoring kernel takes 3,072 points per tile and a CU holds at most 8 blocks of 256 threads, so
    whatever occupancy the runtime reports, (8 * CUs + 3) tiles give some blocks a second tile; 17 more points leave the
    last tile ragged.  Not larger than that."""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = (8 * cus + 3) * TILE + 17
    cloud = scene(n, seed=1)
    ref = sac.segment(cloud, 0.01, seed=1, optimize=False)
    print("fullgrid scene: %d CUs -> %d points, %d trials" % (cus, n, ref["trials"]))
    return cloud, ref


def test_fullgrid_trace_and_lists(gpu, full):
    cloud, ref = full
    n = len(cloud)
    assert n > SCAN_CARRY and ref["found"] and MOMENT_GRID < ref["best_count"] < n - MOMENT_GRID
    got, _ = check(gpu, cloud, 0.01, ref=ref, seed=1, optimize=False)
    assert np.array_equal(got["inliers"], ref["first_inliers"])
    # the traced models' counts are sac.count_within's (the restatement's trace); two more models by hand
    hand = np.array([[0.0, 0.0, 1.0, -0.5], [0.6, 0.0, -0.8, 0.25]], np.float32)
    assert not any(t["skipped"] for t in ref["trace"])
    models = np.concatenate([models_of(ref["trace"]), hand])
    cnt = got["seg"].countWithinDistance(models)
    expect = [t["count"] for t in ref["trace"]] + [sac.count_within(cloud, m, 0.01) for m in hand]
    assert cnt.tolist() == expect and expect[-1] > 0 and expect[-2] > 0
    assert got["seg"].countWithinDistance(models).tobytes() == cnt.tobytes()


def test_fullgrid_refit(gpu, full):
    """the moments kernel over far more inliers than its grid has threads; the lists are the restatement's selection on the
    device's coefficients (check)"""
    cloud, ref = full
    got, _ = check(gpu, cloud, 0.01, ref=ref, seed=1, optimize=True)
    assert got["stats"]["refined"] and ref["best_count"] > MOMENT_GRID  # (the refit's accuracy: test_refit_strided)


# ---- 2. the refit with a strided grid ------------------------------------------------------------------------------------------
def tilted_plane(n=300000, seed=5):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n, 2))
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.5 + rng.normal(0, 0.004, n)
    return np.column_stack([xy, z])  # float64


def refit_case(kind):
    p = tilted_plane()
    if kind == "shifted":
        p = p + np.array([1000.0, -2000.0, 500.0])
    elif kind == "scaled":
        p = p * 1e-2
    return np.ascontiguousarray(p, np.float32)


@pytest.mark.parametrize("kind", ["plain", "shifted", "scaled"])
def test_refit_strided(gpu, kind):
    """Bar of test_refit_against_float64: the device is no further from the float64 fit (numpy eigh) of the inliers than
    2 x the reference's float path (sac_restatement.refit) plus 8 * 2^-24.  Every point is an inlier (the threshold is
    larger than the cloud), so the moments kernel strides over 300,000 entries.
    Measured on an MI355X, device / reference float path: see DESIGN.md row f-11.  The reference adds its 300,000 terms
    one after the other in float and sits 3e-5 (4.6e-4 at the offset, where the normal's error reaches d through a
    centroid 2,300 from the origin and the measure divides by |d| of about 200) from the float64 fit, so that bar is wide
    here.  A second one, from the device's own arithmetic: double sums, ONE rounding of the covariance to float and a float
    eigen33 on eigenvalues with a gap of order 1 leave the normal within a few 2^-24; d = -(n . centroid) carries that
    times |centroid| / max(1, |d|).  16 * 2^-24 times that lever; sums kept in float would be 30 times and more beyond it."""
    cloud = refit_case(kind)
    n = len(cloud)
    got = run(gpu, cloud, 10.0, seed=3, optimize=True)
    st = got["stats"]
    assert st["refined"] and st["best_count"] == n > MOMENT_GRID and len(got["inliers"]) == n and len(got["outliers"]) == 0
    fit = float64_fit(cloud)
    d_dev = fit_distance(got["coefficients"], fit)
    d_ref = fit_distance(sac.refit(cloud, np.arange(n, dtype=np.int32)), fit)
    print("refit %s: device %.3g, reference float path %.3g from the float64 fit" % (kind, d_dev, d_ref))
    assert d_dev <= 2.0 * d_ref + 8.0 * 2.0 ** -24
    lever = max(1.0, float(np.linalg.norm(cloud.astype(np.float64).mean(0))) / max(1.0, abs(fit[3])))
    assert d_dev <= 16.0 * 2.0 ** -24 * lever, (d_dev, lever)


def test_refit_exactly_coplanar(gpu):
    """an integer lattice on z = 0: the smallest eigenvalue is exactly 0.  (0, 0, +-1, 0) up to the same bar, from the
    refit or -- should its solve not be finite -- from the winner, which is kept then"""
    gx, gy = np.meshgrid(np.arange(600, dtype=np.float32), np.arange(500, dtype=np.float32), indexing="ij")
    cloud = np.ascontiguousarray(np.column_stack([gx.ravel(), gy.ravel(), np.zeros(gx.size, np.float32)]))
    n = len(cloud)
    got, ref = check(gpu, cloud, 0.5, seed=1, optimize=True)
    assert ref["found"] and ref["best_count"] == n > MOMENT_GRID
    fit = np.array([0.0, 0.0, 1.0, 0.0])
    d_dev = fit_distance(got["coefficients"], fit)
    host = sac.refit(cloud, np.arange(n, dtype=np.int32))
    d_ref = fit_distance(host, fit) if host is not None else 0.0
    print("refit coplanar: device %.3g (refined %s), reference float path %.3g" % (d_dev, got["stats"]["refined"], d_ref))
    if not got["stats"]["refined"]:
        assert got["coefficients"].tobytes() == ref["coefficients"].tobytes()
    assert d_dev <= 2.0 * d_ref + 8.0 * 2.0 ** -24
    assert len(got["inliers"]) == n


def test_refit_smallest_sets(gpu):
    cloud = scene(4, seed=4)
    got, ref = check(gpu, cloud, 10.0, seed=4, optimize=True)  # 4 inliers: the refit runs
    assert ref["best_count"] == 4 and got["stats"]["refined"]
    fit = float64_fit(cloud)
    d_dev = fit_distance(got["coefficients"], fit)
    d_ref = fit_distance(sac.refit(cloud, np.arange(4, dtype=np.int32)), fit)
    print("refit 4 points: device %.3g, reference float path %.3g from the float64 fit" % (d_dev, d_ref))
    assert d_dev <= 2.0 * d_ref + 8.0 * 2.0 ** -24
    got, ref = check(gpu, cloud[:3], 10.0, seed=4, optimize=True)  # 3 inliers: it does not
    assert ref["best_count"] == 3 and not got["stats"]["refined"]
    assert got["coefficients"].tobytes() == ref["coefficients"].tobytes()


# ---- 3. samples around the skip test ---------------------------------------------------------------------------------------------
def test_skip_boundary(gpu):
    """cross products of a few 1e-5: norms on both sides of Eigen's dummy_precision"""
    cloud = (scene(2000, seed=3) * np.float32(3e-3)).astype(np.float32)
    kw = dict(seed=1, max_iterations=200, probability=0.999999)
    ref = sac.segment(cloud, 0.012 * 3e-3, optimize=False, **kw)
    assert (ref["trials"], ref["skipped"], ref["iterations"], ref["best_count"]) == (74, 40, 34, 1391)
    flags = [t["skipped"] for t in ref["trace"]]
    assert 4 * sum(flags) >= len(flags) and 4 * (len(flags) - sum(flags)) >= len(flags)
    check(gpu, cloud, 0.012 * 3e-3, ref=ref, optimize=False, **kw)


# ---- 4. cancellation ----------------------------------------------------------------------------------------------------------------
def test_far_from_the_origin(gpu):
    """|a x|, |b y|, |c z| and |d| of hundreds to thousands against a threshold of 0.012: any contraction or reordering of
    (a x + b y) + (c z + d) moves counts"""
    cloud = (scene(5000, seed=4).astype(np.float64) + np.array([1000.0, -2000.0, 500.0])).astype(np.float32)
    got, ref = check(gpu, cloud, 0.012, seed=2, optimize=False)
    assert ref["found"] and ref["best_count"] > 1000
    models = models_of(ref["trace"])
    assert got["seg"].countWithinDistance(models).tolist() == [sac.count_within(cloud, m, 0.012) for m in models]
    check(gpu, cloud, 0.012, ref=ref, seed=2, optimize=True)


# ---- 5. overflow ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1e19, 1e30])
def test_overflowing_coordinates(gpu, factor):
    """at 1e19 the squares of the cross product overflow, at 1e30 the cross product itself: infinities and NaNs in the
    coefficients, compared NaN-aware (same_trace)"""
    cloud = (scene(2000, seed=3) * np.float32(factor)).astype(np.float32)
    assert np.isfinite(cloud).all()
    got, ref = check(gpu, cloud, 0.012 * factor, seed=3, optimize=False)
    if factor == 1e30:
        assert np.isnan(models_of(ref["trace"])).any()
        assert not ref["found"] and ref["trials"] == 51 and all(t["count"] == 0 for t in got["trace"])
        assert got["stats"]["trials"] == 51 and len(got["inliers"]) == 0 and len(got["outliers"]) == len(cloud)
    check(gpu, cloud, 0.012 * factor, ref=ref, seed=3, optimize=True)


# ---- 6. the stopping rule ------------------------------------------------------------------------------------------------------------
def test_stopping_rule_edges(gpu):
    cloud = scene(2000, seed=3)
    got, ref = check(gpu, cloud, 0.012, seed=1, optimize=False, probability=0.0)
    assert ref["trials"] == 1 and got["stats"]["trials"] == 1 and ref["found"]
    got, ref = check(gpu, cloud, 0.012, seed=1, optimize=False, probability=1.0, max_iterations=30)
    assert ref["iterations"] == 31 and got["stats"]["iterations"] == 31 and got["stats"]["skipped"] == 0
    got, ref = check(gpu, cloud, 0.012, seed=1, optimize=False, max_iterations=0)
    assert ref["trials"] == 1 and got["stats"]["trials"] == 1 and ref["found"] and len(got["inliers"]) == ref["best_count"] > 0


def test_more_trials_than_a_batch(gpu):
    """64 + 128 + 256 + 512 + 1,024 trials, then the last automatic batch clipped to max_iterations + 1 - iterations"""
    cloud = scene(2000, seed=3)
    got, ref = check(gpu, cloud, 1e-7, seed=1, optimize=False, max_iterations=3000, probability=0.999999999)
    assert ref["trials"] == 3001 and ref["skipped"] == 0 and ref["found"]
    assert got["stats"]["trials"] == 3001 and got["stats"]["batches"] == 6


# ---- 7. the trace's cap --------------------------------------------------------------------------------------------------------------
def test_trace_cap(gpu):
    cloud = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (500, 1))
    ref = sac.segment(cloud, 0.01, seed=2, optimize=False, max_iterations=7000)
    assert ref["trials"] == ref["skipped"] == 70000 and not ref["found"]
    got = run(gpu, cloud, 0.01, seed=2, optimize=False, max_iterations=7000)
    st = got["stats"]
    assert (st["trials"], st["skipped"], st["iterations"], st["best_trial"]) == (70000, 70000, 0, -1)
    assert len(got["trace"]) == TRACE_MAX
    same_trace(got["trace"], ref["trace"][:TRACE_MAX])
    assert len(got["inliers"]) == 0 and len(got["coefficients"]) == 0 and np.array_equal(got["outliers"], np.arange(500))


# ---- 8. records wider than 12 bytes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,fill", [(4, np.inf), (8, np.nan)])
def test_wide_records(gpu, width, fill):
    cloud = scene(5000, seed=7)
    wide = np.full((len(cloud), width), fill, np.float32)
    wide[:, :3] = cloud
    models = np.array([[0.3, -0.2, -1.0, 0.5], [0.0, 0.0, 1.0, -0.5], [1.0, 0.0, 0.0, 0.0]], np.float32)
    for optimize in (False, True):
        a = run(gpu, cloud, 0.012, seed=8, optimize=optimize)
        b = run(gpu, wide, 0.012, seed=8, optimize=optimize)
        assert len(a["inliers"]) > 1000 and a["stats"]["refined"] == optimize
        assert trace_bytes(a["trace"]) == trace_bytes(b["trace"])
        assert a["coefficients"].tobytes() == b["coefficients"].tobytes()
        assert a["inliers"].tobytes() == b["inliers"].tobytes() and a["outliers"].tobytes() == b["outliers"].tobytes()
    both = np.concatenate([models, models_of(a["trace"])])
    assert a["seg"].countWithinDistance(both).tobytes() == b["seg"].countWithinDistance(both).tobytes()
    check(gpu, wide, 0.012, seed=8, optimize=False)
