"""The normal-plane scoring pass off its easy path: inputs that put every pair inside the interval its screen cannot
decide (the double acos on every lane, on both sides of the threshold), lanes that mix the screen's three outcomes, more
hypotheses than one pass holds, batches of every size, the device's whole grid.  Same contract and the same band as
tests/test_gpu_sac_models.py, asserted empty first."""
import numpy as np
import pytest

import sac_models_restatement as sm
from test_gpu_sac_models import NTILE, check, evaluated, gold, gpu, scene, segmenter, trace_bytes  # noqa: F401

pytestmark = pytest.mark.gpu


def tilted_sheet(n, angle, seed=0):
    """points ON the plane z = 0 whose normals all make `angle` with z, in directions all around"""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0, 2 * np.pi, n)
    cloud = np.column_stack([rng.uniform(-1, 1, (n, 2)), np.zeros(n)]).astype(np.float32)
    nrm = np.column_stack([np.sin(angle) * np.cos(phi), np.sin(angle) * np.sin(phi), np.full(n, np.cos(angle)), np.zeros(n)])
    return cloud, np.ascontiguousarray(nrm, np.float32)


@pytest.mark.parametrize("angle", [0.0, 1e-3, 0.3, 1.2, np.pi / 2])
def test_every_pair_inside_the_screens_interval(gpu, angle):
    """distance = ndw * angle for every point; thresholds a few 1e-7 either side of it lie inside ndw * 7.5e-5 of every
    pair, so the polynomial decides none and the double acos decides all -- in both directions, with the float rounding of
    the normals spreading the pairs over both sides"""
    n, ndw = 1000, 0.5
    cloud, normals = tilted_sheet(n, angle, seed=7)
    model = sm.Model(11, ndw=ndw)
    pts, nrm, _ = sm.point_set(cloud, normals)
    plane = np.array([[0, 0, 1, 0], [0, 0, -1, 0]], np.float32)
    d = model.distances(pts, model.prepare(nrm), plane[0])
    mid = float(np.median(d))  # (a float dot near 1 quantises a small angle: 9.8e-4 for 1e-3)
    assert np.abs(d - mid).max() < 1e-6 and abs(mid - ndw * angle) < 2e-5
    seen = set()
    for thr in (mid, float(d.min()), float(np.nextafter(d.max(), 1.0)), mid + 3e-7, mid - 3e-7):
        if thr <= 0.0:
            continue
        ev = sm.evaluate(model, cloud, normals, plane, thr)
        if ev["in_band"] != 0:  # a threshold ON a distance: 1e-11 up is off it by far more than the band (7e-15)
            thr = thr * (1.0 + 1e-11)
        cnt = evaluated(gpu, cloud, normals, thr, dict(model_type=11, ndw=ndw), plane)
        seen.add(int(cnt[0]))
    assert len(seen) >= (2 if angle > 0 else 1) and max(seen) == n


def test_lanes_mix_the_outcomes(gpu):
    """neighbouring points alternate between far outside, deep inside, inside the interval and a weight outside [0, 1]"""
    n = 3 * NTILE + 77
    cloud, normals = tilted_sheet(n, 0.2, seed=3)
    k = np.arange(n) % 4
    cloud[k == 0, 2] = 0.5                      # out by the Euclidean part alone
    normals[k == 1, :3] = (0, 0, -1)            # in: the angle folds to 0
    normals[k == 3, 3] = np.where(np.arange((k == 3).sum()) % 2 == 0, -3.0, 1.5)  # weights 0.4 and -0.05: the exact path
    plane = np.array([[0, 0, 1, 0], [0, 0, 1, -0.5], [0.6, 0, 0.8, 0]], np.float32)
    for thr in (0.1 * 0.2 + 2e-7, 0.05):
        cnt = evaluated(gpu, cloud, normals, thr, dict(model_type=11, ndw=0.1), plane)
        assert 0 < cnt[0] < n


def test_more_hypotheses_than_a_pass(gpu):
    cloud, normals = scene(700, seed=5)
    models = sm.hypotheses(cloud, 1025, seed=9)
    cnt = evaluated(gpu, cloud, normals, 0.03, dict(model_type=11, ndw=0.1), models)
    assert cnt.max() > 300
    cnt = evaluated(gpu, cloud, normals, 0.03, dict(model_type=9, axis=(0.3, -0.2, -1.0), eps_angle=0.2), models)
    assert cnt.max() > 300 and (cnt == 0).sum() > 500


@pytest.mark.parametrize("model", [9, 11])
def test_batch_size_changes_nothing(gpu, gold, model):
    cloud, normals = gold
    mk = dict(model_type=11, ndw=0.1) if model == 11 else dict(model_type=9, axis=(-0.8964, -0.5868, -1.208), eps_angle=0.1)
    runs = [check(gpu, cloud, normals, 0.03, mk, seed=2, batch=b)[0] for b in (0, 1, 7, 1024)]
    assert runs[1]["stats"]["batches"] > runs[2]["stats"]["batches"] > runs[0]["stats"]["batches"] == 1
    for r in runs[1:]:
        assert r["inliers"].tobytes() == runs[0]["inliers"].tobytes() and r["outliers"].tobytes() == runs[0]["outliers"].tobytes()
        assert r["coefficients"].tobytes() == runs[0]["coefficients"].tobytes()
        assert trace_bytes(r["trace"]) == trace_bytes(runs[0]["trace"])


def test_skips_and_invalid_trials_together(gpu):
    """two thirds of the points coincide (degenerate samples: skips) under a gate most planes fail (iterations that
    count 0): both kinds in one trace, over several automatic batches"""
    cloud, normals = scene(300, seed=11)
    cloud[:200] = cloud[0]
    mk = dict(model_type=16, axis=(0.3, -0.2, -1.0), eps_angle=0.3, ndw=0.1)
    got, ref = check(gpu, cloud, normals, 0.02, mk, seed=4, max_iterations=200, probability=0.999999)
    kinds = {(t["skipped"], t["valid"]) for t in got["trace"]}
    assert kinds == {(True, False), (False, False), (False, True)} and got["stats"]["batches"] > 1
    assert got["stats"]["skipped"] > 50


def test_fullgrid(gpu):
    """A block of the normal-plane scoring kernel takes 2,048 points per tile and a CU holds at most 8 blocks of 256
    threads, so whatever occupancy the runtime reports, (8 * CUs + 3) tiles give some blocks a second tile; 17 more points
    leave the last tile ragged.  Two hypotheses keep the restatement quick.  (On the emulation, with its 32 blocks, the
    cases above reach a block's second tile already: tests/test_sac_models_wavesim.py leaves this one to the GPU.)"""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n = (8 * cus + 3) * NTILE + 17
    cloud, normals = scene(n, seed=1)
    models = np.array([[0.3, -0.2, -1.0, 0.5], [0.0, 0.0, 1.0, -0.5]], np.float32)
    models[0] /= np.linalg.norm(models[0, :3])
    cnt = evaluated(gpu, cloud, normals, 0.03, dict(model_type=11, ndw=0.1), models)
    print("fullgrid scene: %d CUs -> %d points, counts %s" % (cus, n, cnt.tolist()))
    assert cnt[0] > n // 2 > cnt[1] > 0
