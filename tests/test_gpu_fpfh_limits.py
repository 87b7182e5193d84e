"""The 16-bit limit of pclhip_fpfh's bin counters (FPFH_MAX_COUNT in pcl_amd/csrc/fpfh.hpp), the only guard against a
histogram that wrapped without a word: a neighbourhood of 65,535 other points fills a counter to 0xFFFF and succeeds, one
of 65,536 is PCLHIP_ERR_OVERFLOW.  No smaller shape reaches the limit, so this module runs on the hardware only (it is
not part of tests/test_fpfh_wavesim.py: 4.3e9 pair evaluations per SPFH pass are out of the emulation's reach).

The cloud is the coplanar grid of tests/test_gpu_fpfh_regimes.py, whose rows are known in closed form: every pair has
f1 = f2 = f3 = 0, every count falls into bins 5 / 16 / 27.  FPFH rows are asked for 256 spread points only, so that only
the SPFH pass is quadratic.

Measured on an MI355X: the whole module 0.8 s of wall time (three fully dense calls, 4.3e9 pairs each); one call 0.12 s,
of which the SPFH kernel 57 ms (75e9 pairs per second: every pair takes the same branch) and the weighting kernel of the
256 queries 46 ms (four waves, each lane walking 65,536 neighbours)."""
import time

import numpy as np
import pytest

import fpfh_restatement as fr
from test_gpu_fpfh import bits
from test_gpu_fpfh_regimes import HOT, check_plane_fpfh, plane_grid, plane_rows

pytestmark = pytest.mark.gpu

SIDE = 256
N = SIDE * SIDE
RADIUS = 2.0


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def plane():
    pts, nrm = plane_grid(SIDE)
    assert len(pts) == N == 65536
    sel = np.ascontiguousarray(np.arange(256, dtype=np.int32) * 257 % N)  # 256 spread points, every row and column once
    return pts, nrm, sel


@pytest.fixture(scope="module")
def at_the_limit(gpu, plane):
    """one object over the 65,536-point grid: (object, FPFH rows of the 256 queries, SPFH rows, seconds)"""
    import pcl_amd
    pts, nrm, sel = plane
    f = pcl_amd.FPFHEstimation(gpu)
    f.setInputCloud(pts)
    f.setInputNormals(nrm)
    f.setRadiusSearch(RADIUS)
    f.setIndices(sel)
    t0 = time.perf_counter()
    out, spfh = f.computeBoth()
    dt = time.perf_counter() - t0
    print("n = %d, every point a neighbour of every point: %.3f s (SPFH kernel %.1f ms, weighting kernel %.1f ms)" %
          ((N, dt) + tuple(f.lastPassMs())))
    return f, out, spfh, dt


def test_65535_neighbours_fill_a_counter(at_the_limit, plane):
    f, out, spfh, _ = at_the_limit
    pts, nrm, sel = plane
    assert f.nan_count == 0 and out.shape == (256, 33) and spfh.shape == (N, 33)
    want = plane_rows(N)  # hist_incr = 100 / 65535 added 65,535 times
    cold = np.ones(33, bool)
    cold[HOT] = False
    assert (want[cold] == 0).all() and (want[HOT] > 0).all()
    sample = np.sort(np.random.default_rng(1).permutation(N)[:64])
    assert (bits(spfh[sample]) == bits(want)[None, :]).all()
    counts = fr.counts_from_rows(spfh[sample[:2]], np.full(2, N))
    assert (counts[:, HOT] == 0xFFFF).all() and (counts[:, cold] == 0).all()  # a counter sits at its last value
    check_plane_fpfh(out)


def test_65536_neighbours_overflow_and_the_object_recovers(at_the_limit, plane):
    import pcl_amd
    f, out, spfh, _ = at_the_limit
    pts, nrm, sel = plane
    more = np.ascontiguousarray(np.concatenate([pts, np.float32([[1.0, 1.0, 0.0]])]))
    more_nrm = np.ascontiguousarray(np.concatenate([nrm, np.float32([[0.0, 0.0, 1.0]])]))
    f.setInputCloud(more)
    f.setInputNormals(more_nrm)
    with pytest.raises(pcl_amd.PclHipError) as e:
        f.computeBoth()
    assert e.value.status == -5  # PCLHIP_ERR_OVERFLOW
    # the point dropped again, the same tree and context: the first run's bits
    f.setInputCloud(pts)
    f.setInputNormals(nrm)
    out2, spfh2 = f.computeBoth()
    assert f.nan_count == 0
    assert np.array_equal(bits(out2), bits(out)) and np.array_equal(bits(spfh2), bits(spfh))
