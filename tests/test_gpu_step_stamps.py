"""The marker-free step of the device-driven ICP loop: the chain-free loop (no rejectors, no reciprocal test, no served-group
lists, no per-lane search) queues its three kernels and nothing else -- they stamp their own times with the device's
constant-rate counter, and the host learns of a finished step from the sequence word of the step record instead of an event.
Option "step_events" = 1 sends the same loop down the event path every other loop still takes.

Nothing of this may change a result.  Checked here, the two paths side by side on two contexts:

  * runSteps and align() on 100,000-point clouds, point-to-point and point-to-plane: every record field equal (==), the
    transformations bit for bit;
  * 200 steps through the 64-slot record ring (more than three wraps), in sequence, the alignments restarting alike;
  * the step times: 0 < search_ms <= kernels_ms <= step_ms for every step, and the steps of a call (disjoint intervals of
    one device clock: a step starts at its predecessor's exit stamp) add up to no more than the host's wall time;
  * the two ways a queued launch leaves no record -- an alignment that ends at once for lack of correspondences, and
    launches queued behind the last iteration that fall through -- return instead of waiting for one;
  * forty registration objects, each made, aligned once and dropped.

Reference behaviour: IterativeClosestPoint::computeTransformation (registration/include/pcl/registration/impl/icp.hpp:113-268),
DefaultConvergenceCriteria (default_convergence_criteria.h).
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("iteration", "state", "converged", "alignment_ended", "num_correspondences", "mse")


@pytest.fixture(scope="module")
def contexts():
    """(stamped, events): two contexts that differ in option "step_events" only"""
    from conftest import make_context
    stamped, events = make_context(0), make_context(0)
    stamped.setOption("step_events", 0)
    events.setOption("step_events", 1)
    return stamped, events


_scenes = {}


def scene(ctx, n, mode):
    """the n-point pair of pcl_amd.synth.icp_pair indexed on `ctx` (normals for point-to-plane): built once per context"""
    import pcl_amd
    key = (id(ctx), n, mode)
    if key not in _scenes:
        tgt, src, _ = pcl_amd.synth.icp_pair(n)
        tree = pcl_amd.KdTree(ctx)
        tree.setInputCloud(tgt)
        ne = None
        if mode == 1:
            ne = pcl_amd.NormalEstimation(ctx)
            ne.setInputCloud(tgt)
            ne.setSearchMethod(tree)
            ne.setKSearch(8)
            ne.setViewPoint(0, 0, 10)
            ne.compute(want_output=False)
        _scenes[key] = {"tgt": tgt, "src": src, "tree": tree, "ne": ne}
    return _scenes[key]


def make_icp(ctx, n, mode, max_iterations=20, max_distance=0.1):
    import pcl_amd
    sc = scene(ctx, n, mode)
    cls = pcl_amd.IterativeClosestPointWithNormals if mode == 1 else pcl_amd.IterativeClosestPoint
    icp = cls(ctx)
    icp.setSearchMethodTarget(sc["tree"], True)
    icp.setInputSource(sc["src"])
    icp.setMaximumIterations(max_iterations)
    icp.setMaxCorrespondenceDistance(max_distance)
    icp.setTransformationEpsilon(1e-10)
    return icp


def assert_same_records(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for f in FIELDS:
            assert x[f] == y[f], (k, f, x[f], y[f])
        assert np.array_equal(x["final_transformation"], y["final_transformation"]), k


def aligned(icp):
    icp.align()
    return icp.nr_iterations_, icp.getConvergenceState(), icp.hasConverged(), icp.getFinalTransformation().copy()


def assert_same_alignment(a, b):
    assert a[:3] == b[:3], (a[:3], b[:3])
    assert np.array_equal(a[3], b[3])


@pytest.mark.parametrize("mode", [0, 1])
def test_the_two_paths_agree(contexts, mode):
    stamped, events = contexts
    a, b = make_icp(stamped, 100_000, mode), make_icp(events, 100_000, mode)
    ra, rb = a.runSteps(12), b.runSteps(12)
    assert len(ra) == 12
    assert_same_records(ra, rb)
    assert any(s["alignment_ended"] for s in ra) or ra[-1]["iteration"] == 12
    assert_same_alignment(aligned(a), aligned(b))


def test_ring_wrap(contexts):
    stamped, events = contexts
    a, b = make_icp(stamped, 4096, 1), make_icp(events, 4096, 1)
    ra, rb = a.runSteps(200), b.runSteps(200)      # the ring holds 64 records: more than three wraps
    assert len(ra) == 200 and len(rb) == 200
    prev_ended, prev_it = True, 0
    for k, s in enumerate(ra):
        if s["state"] != "NO_CORRESPONDENCES":
            assert s["iteration"] == (1 if prev_ended else prev_it + 1), (k, s["iteration"], prev_it, prev_ended)
        prev_ended, prev_it = s["alignment_ended"], s["iteration"]
    assert sum(1 for s in ra if s["alignment_ended"]) >= 3      # the alignment restarted inside the queue
    assert [(s["iteration"], s["state"]) for s in ra] == [(s["iteration"], s["state"]) for s in rb]
    assert_same_records(ra, rb)


@pytest.mark.parametrize("which", ["stamped", "events"])
@pytest.mark.parametrize("n,steps", [(4096, 40), (100_000, 12)])
def test_times_are_sane(contexts, which, n, steps):
    ctx = contexts[0] if which == "stamped" else contexts[1]
    icp = make_icp(ctx, n, 1)
    icp.runSteps(3)       # the first call of a registration allocates the loop's state
    for _ in range(2):
        ctx.synchronize()
        t0 = time.perf_counter()
        rec = icp.runSteps(steps)
        ctx.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        for k, s in enumerate(rec):
            assert 0.0 < s["search_ms"] <= s["kernels_ms"] <= s["step_ms"], (k, s["search_ms"], s["kernels_ms"], s["step_ms"])
        total = sum(s["step_ms"] for s in rec)
        print("%s n=%d: %d steps, sum(step_ms) %.4f ms, wall %.4f ms" % (which, n, steps, total, wall_ms))
        assert total <= wall_ms, (total, wall_ms)


def test_no_correspondences_ends_without_a_hang(contexts):
    stamped, events = contexts
    # no target point lies within 1e-9 of a source point: the first iteration finds no pair
    ra = aligned(make_icp(stamped, 4096, 1, max_distance=1e-9))
    rb = aligned(make_icp(events, 4096, 1, max_distance=1e-9))
    assert ra[1] == "NO_CORRESPONDENCES" and not ra[2], ra[:3]
    assert_same_alignment(ra, rb)
    assert np.array_equal(ra[3], np.eye(4, dtype=np.float32))
    # ... and as a queue of steps every step is such an alignment, each with its record
    sa = make_icp(stamped, 4096, 1, max_distance=1e-9).runSteps(5)
    sb = make_icp(events, 4096, 1, max_distance=1e-9).runSteps(5)
    assert all(s["state"] == "NO_CORRESPONDENCES" and s["alignment_ended"] for s in sa)
    assert_same_records(sa, sb)


@pytest.mark.parametrize("mode", [0, 1])
def test_launches_behind_the_last_iteration_leave_no_record(contexts, mode):
    stamped, events = contexts
    for ctx in contexts:
        ctx.setOption("icp_lookahead", 3)      # three launches queued behind the one that ends the alignment: they fall through
    try:
        a, b = make_icp(stamped, 4096, mode, max_iterations=1), make_icp(events, 4096, mode, max_iterations=1)
        ra, rb = aligned(a), aligned(b)
        assert ra[0] == 1 and ra[1] == "ITERATIONS", ra[:3]
        assert_same_alignment(ra, rb)
        assert_same_alignment(aligned(a), aligned(b))      # the loop is armed again behind the launches that fell through
        assert_same_records(a.runSteps(70), b.runSteps(70))
    finally:
        for ctx in contexts:
            ctx.setOption("icp_lookahead", 1)


def test_object_per_alignment(contexts):
    stamped, events = contexts
    first = aligned(make_icp(stamped, 20_000, 1))
    assert first[0] > 1
    for k in range(39):
        icp = make_icp(stamped, 20_000, 1)
        assert_same_alignment(aligned(icp), first)
        del icp
    assert_same_alignment(aligned(make_icp(events, 20_000, 1)), first)
