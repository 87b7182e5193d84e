"""The lean ICP step: the group counters re-armed by the kernel that closes an iteration instead of a memset in front of every
search launch, and the matches kept as sorted positions only (the original index is read where somebody wants it).

Nothing of this may change a result.  Checked here, against the oracle and the host-driven loop:

  * the device-driven loop at source sizes around the 64-point group (1, 63, 64, 65, 127, 129) and past the target's size,
    across restarts of the alignment inside one queue (the counters are re-armed step after step, never by the host);
  * launches of other kinds interleaved on the same context (k-NN, a second registration, speculative launches that fall
    through behind a finished alignment) -- every one of them must find the counters zero.  The counters only hand out
    groups once a wave has two or more of its own: FEED_POINTS is the smallest source for which that is the case on 256
    compute units (2 groups x 64 points for each of 256 x 4 x 4 resident waves), so the interleaving runs at that size;
  * a lattice target full of exact ties: the (distance, lowest index) policy of the reference;
  * every reader of the matches' original indices: the correspondence fetch (twice in a row, and before any step), the
    OneToOne rejector, reciprocal correspondences, GICP's pair packing, the served-group lists under a region;
  * an empty source and a source without a finite point.

Reference behaviour: CorrespondenceEstimation::determineCorrespondences
(registration/include/pcl/registration/impl/correspondence_estimation.hpp:145-218), IterativeClosestPoint::
computeTransformation (impl/icp.hpp:113-268), CorrespondenceRejectorOneToOne (correspondence_rejection_one_to_one.cpp:49-65).

The CPU tier runs this module on the emulation with smaller clouds (tests/test_step_lean_wavesim.py sets the two sizes).
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TGT = int(os.environ.get("PCLHIP_STEP_LEAN_TARGET", "4096"))
FEED_POINTS = int(os.environ.get("PCLHIP_STEP_LEAN_FEED", str(2 * 64 * 256 * 4 * 4 + 4097)))
SIZES = [1, 63, 64, 65, 127, 129, N_TGT + 1]
STATES = ["NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES", "FAILURE_AFTER_MAX_ITERATIONS"]


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


@pytest.fixture(scope="module")
def scene(orc):
    """the 4k-point sheet, its oracle tree and normals, and a source stream longer than any case needs: computed once"""
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(FEED_POINTS, n_target=N_TGT)
    otree = orc.KdTree(tgt)
    nrm = otree.normals(tgt, 8, viewpoint=(0, 0, 10))[0]
    for a in (tgt, src, nrm):
        a.setflags(write=False)
    return {"tgt": tgt, "src": src, "otree": otree, "nrm": nrm}


def make_icp(gpu, scene, src, mode, max_iterations=20):
    import pcl_amd
    cls = pcl_amd.IterativeClosestPointWithNormals if mode == 1 else pcl_amd.IterativeClosestPoint
    icp = cls(gpu)
    icp.setInputTarget(scene["tgt"])
    if mode == 1:
        icp.setTargetNormals(scene["nrm"])
    icp.setInputSource(src)
    icp.setMaximumIterations(max_iterations)
    icp.setMaxCorrespondenceDistance(0.1)
    icp.setTransformationEpsilon(1e-10)
    return icp


def same_pairs(got, want):
    (q, m, d), (oq, om, od) = got, want
    return np.array_equal(q, oq) and np.array_equal(m, om) and np.array_equal(d.view(np.uint32), od.view(np.uint32))


def summary(steps):
    return [(s["iteration"], s["state"], s["alignment_ended"], s["num_correspondences"], s["mse"],
             s["final_transformation"].tobytes()) for s in steps]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_src", SIZES)
def test_device_loop_equals_oracle_and_host_loop(gpu, orc, scene, n_src, mode):
    from pcl_amd import _lib
    from test_gpu_loop import _host_loop_align
    src = np.ascontiguousarray(scene["src"][:n_src])
    # every iteration's correspondences against the oracle, the oracle's cloud moved by the device's own increments
    gpu.setOption("icp_lookahead", 0)
    try:
        cur = src.copy()
        for K in range(1, 21):
            icp = make_icp(gpu, scene, src, mode, K)
            icp.align()
            if icp.nr_iterations_ < K and K > 1:
                break
            assert same_pairs(icp.fetchCorrespondences(), scene["otree"].correspondences(cur, 0.1)), K
            if icp.nr_iterations_ < K:
                break   # (too few pairs to estimate from: the one search there was is compared above)
            cur = orc.transform_cloud(icp.getLastIncrementalTransformation(), cur, order=1 if mode == 1 else 0)
    finally:
        gpu.setOption("icp_lookahead", 1)
    # the device-driven loop against its host-driven twin, twice (the criteria keep their memory)
    dev, host = make_icp(gpu, scene, src, mode, 25), make_icp(gpu, scene, src, mode, 25)
    host._ensure()
    conv = _lib.ConvergenceState()
    _lib.load().pclhip_convergence_init(C.byref(conv))
    ends = []
    for rep in range(2):
        dev.align()
        b = _host_loop_align(host, conv)
        assert dev.nr_iterations_ == b["it"] and dev.getConvergenceState() == STATES[b["state"]], (rep, b)
        assert dev.hasConverged() == b["conv"], rep
        assert np.abs(dev.getFinalTransformation() - b["T"]).max() < 2e-6
        ends.append((dev.nr_iterations_, dev.getConvergenceState(), dev.getFinalTransformation().copy()))
    # one queue of steps long enough to restart the alignment at least twice: its alignments are those two, bit for bit
    (k, state, T), (k2, state2, T2) = ends
    steps = dev.runSteps(max(k, 1) + max(k2, 1) + 2)
    last = [i for i, s in enumerate(steps) if s["alignment_ended"]]
    assert len(last) >= 2 and last[0] == max(k, 1) - 1 and last[1] == last[0] + max(k2, 1)
    for i, (kk, st, TT) in zip(last, ends):
        assert steps[i]["iteration"] == kk and steps[i]["state"] == st
        assert np.array_equal(steps[i]["final_transformation"], TT)
    assert steps[last[1] + 1]["iteration"] in (0, 1)    # a third alignment started behind the second restart


def big_source(scene):
    return np.ascontiguousarray(scene["src"][:FEED_POINTS])


def test_knn_between_two_queues_of_steps(gpu, orc, scene):
    import pcl_amd
    src = big_source(scene)
    # the launch that starts an alignment and the first seeded one at this size, against the oracle
    cur = src
    for K in (1, 2):
        one = make_icp(gpu, scene, src, 1, K)
        one.align()
        assert one.nr_iterations_ == K
        assert same_pairs(one.fetchCorrespondences(), scene["otree"].correspondences(cur, 0.1)), K
        cur = orc.transform_cloud(one.getLastIncrementalTransformation(), cur, order=1)
    icp = make_icp(gpu, scene, src, 1)
    icp.align()
    n = 2 * icp.nr_iterations_ + 1                                 # two alignments and the start of a third
    first = icp.runSteps(n)
    assert sum(s["alignment_ended"] for s in first) == 2
    pairs = icp.fetchCorrespondences()
    assert len(pairs[0]) == first[-1]["num_correspondences"] and same_pairs(icp.fetchCorrespondences(), pairs)
    gi, gd = icp.tree.nearestKSearch(src, 1)                       # as many queries: its waves take groups from the counters too
    oi, od = scene["otree"].knn(src, 1)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)
    again = icp.runSteps(n)
    assert summary(first) == summary(again)
    assert same_pairs(icp.fetchCorrespondences(), pairs)
    fresh = make_icp(pcl_amd.Context(0), scene, src, 1)            # single use, on a context of its own
    assert summary(fresh.runSteps(n)) == summary(first)
    assert same_pairs(fresh.fetchCorrespondences(), pairs)


def test_two_registrations_stepped_alternately(gpu, orc, scene):
    a_src, b_src = big_source(scene), np.ascontiguousarray(scene["src"][5: 5 + 129])
    a, b = make_icp(gpu, scene, a_src, 1), make_icp(gpu, scene, b_src, 0)
    solo = [summary(make_icp(gpu, scene, a_src, 1).runSteps(2)), summary(make_icp(gpu, scene, b_src, 0).runSteps(2))]
    want = [None, None]
    for _ in range(3):
        for i, (icp, src, order) in enumerate(((a, a_src, 1), (b, b_src, 0))):
            steps = icp.runSteps(2)          # the launch that starts an alignment, then a seeded one
            assert summary(steps) == solo[i]
            if want[i] is None:              # from the identity the first step's final transformation is its increment
                want[i] = scene["otree"].correspondences(orc.transform_cloud(steps[0]["final_transformation"], src, order=order), 0.1)
            assert same_pairs(icp.fetchCorrespondences(), want[i]), i


def test_align_with_speculative_launches_then_a_fresh_align(gpu, orc, scene):
    src = big_source(scene)
    ref = make_icp(gpu, scene, src, 1)
    gpu.setOption("icp_lookahead", 0)
    try:
        ref.align()
    finally:
        gpu.setOption("icp_lookahead", 1)
    want = (ref.nr_iterations_, ref.getConvergenceState(), ref.getFinalTransformation().tobytes())
    pairs = ref.fetchCorrespondences()
    gpu.setOption("icp_lookahead", 3)      # three launches queued behind the one that ends the alignment: they fall through
    try:
        for _ in range(2):
            cur = src
            for K in (1, 2):               # ended by the iteration limit, and the next object's first searches behind it
                icp = make_icp(gpu, scene, src, 1, K)
                icp.align()
                assert icp.nr_iterations_ == K
                assert same_pairs(icp.fetchCorrespondences(), scene["otree"].correspondences(cur, 0.1)), K
                cur = orc.transform_cloud(icp.getLastIncrementalTransformation(), cur, order=1)
            icp = make_icp(gpu, scene, src, 1)
            icp.align()                    # ended by the criteria
            assert (icp.nr_iterations_, icp.getConvergenceState(), icp.getFinalTransformation().tobytes()) == want
            assert same_pairs(icp.fetchCorrespondences(), pairs)
    finally:
        gpu.setOption("icp_lookahead", 1)


def lattice():
    g = np.arange(14, dtype=np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    tgt = np.stack([X.ravel(), Y.ravel(), Z.ravel(), np.ones(X.size, np.float32)], 1)
    tgt = np.ascontiguousarray(tgt[np.random.default_rng(3).permutation(len(tgt))])
    return tgt, tgt[::2].copy()


def test_lattice_ties_take_the_lowest_index(gpu, orc):
    import pcl_amd
    from test_gpu_lane import rigid
    tgt, src = lattice()
    otree = orc.KdTree(tgt)
    steps = [rigid(t=(0.5, 0, 0)), rigid(t=(0, 0.5, 0)), rigid(t=(0, 0, 0.5)), rigid(t=(0.25, 0, 0)), np.eye(4, dtype=np.float32),
             rigid(t=(-0.75, -0.5, -0.5))]
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp._ensure()
    q, m, d = icp.fetchCorrespondences()      # before any step: no search has run, nothing is matched
    assert len(q) == 0
    icp.reset()
    cur = src.copy()
    for it, T in enumerate(steps):            # host-driven: a launch that starts an alignment, then seeded ones
        icp.iterate(T, max_dist=10.0)
        cur = orc.transform_cloud(T, cur, order=0)
        want = otree.correspondences(cur, 10.0)
        assert same_pairs(icp.fetchCorrespondences(), want), it
        assert same_pairs(icp.fetchCorrespondences(), want), it       # ... and asked again
    # device-driven: the guess puts every query between two lattice points, the first search is all ties
    dev = pcl_amd.IterativeClosestPoint(gpu)
    dev.setInputTarget(tgt)
    dev.setInputSource(src)
    dev.setMaximumIterations(1)
    dev.setMaxCorrespondenceDistance(10.0)
    dev.align(steps[0])
    assert same_pairs(dev.fetchCorrespondences(), otree.correspondences(orc.transform_cloud(steps[0], src, order=0), 10.0))


def test_one_to_one_and_reciprocal_read_positions(gpu, orc, scene):
    import pcl_amd
    from oracle import rejectors as orej
    src = np.ascontiguousarray(scene["src"][:N_TGT + 1])
    tgt = scene["tgt"]
    for reciprocal in (False, True):
        icp = make_icp(gpu, scene, src, 0)
        icp.addCorrespondenceRejector(pcl_amd.CorrespondenceRejectorOneToOne())
        icp.setUseReciprocalCorrespondences(reciprocal)
        icp.align()
        ref = orej.icp_with_filters(orc, tgt, src, 0, reciprocal=reciprocal, rejectors=[orej.reject_one_to_one],
                                    max_iterations=20, max_correspondence_distance=0.1, transformation_epsilon=1e-10)
        assert icp.nr_iterations_ == ref["iterations"]
        assert np.abs(icp.getFinalTransformation() - ref["T"]).max() < 2e-5
        # the kept pairs of the last iteration, in the reference's output order (by match, then distance)
        q, m, d = icp.fetchCorrespondences()
        oq, om = ref["per_iter"][-1]
        assert np.all(np.diff(m) > 0)
        assert sorted(zip(q.tolist(), m.tolist())) == sorted(zip(np.asarray(oq).tolist(), np.asarray(om).tolist()))
        steps = icp.runSteps(ref["iterations"])
        assert [s["num_correspondences"] for s in steps] == [len(q) for q, _ in ref["per_iter"]][:len(steps)]


def test_gicp_pairs_read_positions(gpu, orc, scene):
    import gicp_restatement as rs
    import pcl_amd
    tgt, src = scene["tgt"], np.ascontiguousarray(scene["src"][:N_TGT + 1])
    ct = orc.KdTree(tgt[:, :3]).gicp_covariances(tgt[:, :3], 20, 1e-3)
    cs = orc.KdTree(src[:, :3]).gicp_covariances(src[:, :3], 20, 1e-3)
    reg = pcl_amd.GeneralizedIterativeClosestPoint(gpu)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    reg.setMaximumIterations(1)
    reg.setSourceCovariances(cs)
    reg.setTargetCovariances(ct)
    reg.align()
    want = rs.gicp_align(orc, tgt, src, src_cov=cs, tgt_cov=ct, max_iterations=1)
    si, ti, M_cpu = want["pairs"]
    assert reg.result.num_correspondences == len(si) > 0
    M = reg.mahalanobis()[si]      # (R C1 R^T + C2[match])^-1: the target covariance of the ORIGINAL index of every match
    assert np.all(np.abs(M - M_cpu) <= 1e-12 * np.abs(M_cpu).max(axis=(1, 2))[:, None, None]), np.abs(M - M_cpu).max()


def test_served_groups_under_a_region(gpu, orc, scene):
    # config 5's path: with a region the launch walks the list of served 64-point groups, and a group that stops being served
    # has its matches emptied.  The pairs are the oracle's for the queries whose current position lies in the region.
    # (tests/test_gpu_dist.py::test_served_group_lists_equal_the_full_pass compares the lists with the full pass.)
    src = np.ascontiguousarray(scene["src"][:N_TGT + 1])
    inf = np.inf
    region = np.array([0.10, -inf, -inf, 0.22, inf, inf], np.float32)    # a strip the cloud moves through
    guess = np.eye(4, dtype=np.float32)
    guess[0, 3] = 0.06
    gpu.setOption("icp_lookahead", 0)
    try:
        cur = orc.transform_cloud(guess, src, order=1)
        served = 0
        for K in range(1, 6):
            icp = make_icp(gpu, scene, src, 1, K)
            icp.setRegion(region)
            icp.align(guess)
            if icp.nr_iterations_ < K:
                break
            oq, om, od = scene["otree"].correspondences(cur, 0.1)
            inside = (cur[oq, 0] >= region[0]) & (cur[oq, 0] < region[3])
            assert same_pairs(icp.fetchCorrespondences(), (oq[inside], om[inside], od[inside])), K
            served += int(inside.sum())
            cur = orc.transform_cloud(icp.getLastIncrementalTransformation(), cur, order=1)
        assert 0 < served < 5 * len(src) // 4
    finally:
        gpu.setOption("icp_lookahead", 1)


def test_empty_and_all_non_finite_sources(gpu, scene):
    empty = np.zeros((0, 4), np.float32)
    nans = np.full((130, 4), np.nan, np.float32)
    for src in (empty, nans):
        for mode in (0, 1):
            icp = make_icp(gpu, scene, src, mode)
            icp.align()
            assert not icp.hasConverged() and icp.getConvergenceState() == "NO_CORRESPONDENCES" and icp.nr_iterations_ == 0
            steps = icp.runSteps(3)
            assert [s["state"] for s in steps] == ["NO_CORRESPONDENCES"] * 3
            assert len(icp.fetchCorrespondences()[0]) == 0
    # ... and a registration with pairs on the same context right behind them is untouched
    src = np.ascontiguousarray(scene["src"][:129])
    icp = make_icp(gpu, scene, src, 0, 1)
    icp.align()
    assert same_pairs(icp.fetchCorrespondences(), scene["otree"].correspondences(src, 0.1))
