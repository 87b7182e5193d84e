"""The 1-NN fast policy's half-leaf resolve (pcl_amd/csrc/traverse.hpp: NN1MinT) against the oracle, bit for bit.

NN1MinT keeps a leaf's minimum per half (slots 0-7, slots 8-15) and resolve() re-reads only the winning half.  What can go
wrong with that is a TIE: two slots of one half (resolve sees both), one slot in each half (equal half minima), an equal
minimum in another leaf, a seed found again in its own leaf -- each has to reach the exact (distance, index) policy, and
the winner has to be the slot the whole-leaf resolve found.  The cases are the smallest at which each path runs: more than
one batch under a node, more than one level-2 node, padded last leaves, non-finite and sparse sources, the stand-off
launch and its traverse() fallback, and five steps of the device-driven loop.

Every match is compared as (query, original index, float distance) with np.array_equal.  tests/test_resolve_half_wavesim.py
runs this module on the CPU emulation of the wavefront, the 2^17-point loop with both depths of the seeded body's
pipeline; which depth runs where, and which test covers the two-deep body on the device, is
test_pipeline_depth_of_the_loop_case's business.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuzz_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import pcl_amd
    return pcl_amd.Context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


def shift(x=0.0, y=0.0, z=0.0):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (x, y, z)
    return T


def launches(gpu, orc, tgt, src, steps, max_dist=1e3):
    """host-driven launches (the first starts an alignment, the others are seeded by their predecessor's matches) against
    the oracle's correspondences of the same moved cloud"""
    import pcl_amd
    otree = orc.KdTree(tgt)
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.reset()
    cur = src.copy()
    for it, T in enumerate(steps):
        icp.iterate(T, max_dist=max_dist)
        q, m, d = icp.fetchCorrespondences()
        cur = orc.transform_cloud(T, cur, order=0)
        oq, om, od = otree.correspondences(cur, max_dist)
        assert np.array_equal(q, oq), (it, len(q), len(oq))
        assert np.array_equal(m, om), (it, int((m != om).sum()))
        assert np.array_equal(d, od), it


def flat_patch(n, seed, spacing=1.0):
    """n points of a jittered square grid in z ~ 0"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float64)
    out = np.ones((n, 4), np.float32)
    out[:, :2] = ((g + rng.uniform(-0.3, 0.3, g.shape)) * spacing).astype(np.float32)
    out[:, 2] = (rng.uniform(-0.01, 0.01, n) * spacing).astype(np.float32)
    return out


def test_winner_from_an_earlier_batch_of_the_node(gpu, orc):
    # 2,000 points = 125 leaves under two level-2 nodes; seeds 10 spacings stale keep more than 16 leaves of a node alive,
    # so a lane's winner is often set in a batch that a later one overwrites in the staging buffer
    tgt = flat_patch(2000, 1)
    src = flat_patch(2000, 2)[::2].copy()
    src[:, 2] += 0.05
    launches(gpu, orc, tgt, src, [np.eye(4, dtype=np.float32), shift(10.0, 0.0, 0.0), shift(-0.5, 10.0, 0.0), shift(0.01, 0.0, 0.0)])


def test_winner_from_another_node_than_the_last_one_walked(gpu, orc):
    # 70k points: 4,375 leaves, 69 level-2 nodes; every 64-query group near a cut walks two or more of them
    from pcl_amd import synth
    tgt = synth.family_cloud("sheet", 70_000, 11)
    rng = np.random.default_rng(12)
    src = tgt[rng.integers(0, len(tgt), 20_000)].copy()
    ext = float(np.ptp(tgt[:, :2], axis=0).max())
    h = ext / np.sqrt(len(tgt))
    src[:, :3] += (rng.normal(size=(len(src), 3)) * 0.5 * h).astype(np.float32)
    launches(gpu, orc, tgt, src, [np.eye(4, dtype=np.float32), shift(3 * h, -2 * h, 0.0), shift(0.1 * h, 0.0, 0.0)])


def test_seed_wins_and_seed_found_again_in_its_own_leaf(gpu, orc):
    # queries ARE target points: after the first launch every seed is the answer at distance 0 and is found again in its
    # own leaf (eq && same); then nothing moves (the seed wins, no leaf improves); then a nudge far below the spacing
    tgt = flat_patch(5000, 3)
    src = tgt[::3].copy()
    I = np.eye(4, dtype=np.float32)
    launches(gpu, orc, tgt, src, [I, I, shift(1e-3, -1e-3, 0.0), I])


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.5, 0.0), (0.5, 0.5, 0.5)])
def test_exact_ties_inside_a_leaf_and_across_leaves(gpu, orc, offset):
    # 16^3 integer lattice with 512 of its points present twice, in an index order unrelated to position: duplicates share
    # a leaf (one half or both), queries between lattice points have 2, 4 or 8 equidistant targets in one or several leaves.
    # The match has to be the LOWEST original index every time.
    g = np.arange(16, dtype=np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    lat = np.stack([X.ravel(), Y.ravel(), Z.ravel(), np.ones(X.size, np.float32)], 1)
    rng = np.random.default_rng(5)
    tgt = np.concatenate([lat, lat[rng.choice(len(lat), 512, replace=False)]])
    tgt = np.ascontiguousarray(tgt[rng.permutation(len(tgt))])
    src = lat[::3].copy()
    I = np.eye(4, dtype=np.float32)
    launches(gpu, orc, tgt, src, [shift(*offset), I, shift(1.0, 0.0, 0.0), shift(-0.5, 0.0, 0.0)], max_dist=10.0)


@pytest.mark.parametrize("n_tgt", [1, 15, 16, 17])
def test_padded_last_leaf(gpu, orc, n_tgt):
    # the last leaf is padded with FLT_MAX sentinels: in the half that holds points, in the other half, or not at all
    for seed in range(3):
        ok, msg = fuzz_lib.knn_icp_round(gpu, orc, np.random.default_rng(1000 * n_tgt + seed), sizes=(n_tgt,))
        assert ok, msg


def test_non_finite_source_points(gpu, orc):
    tgt = flat_patch(3000, 7)
    src = flat_patch(3000, 8)[::2].copy()
    src[::7, 0] = np.nan
    src[3::31, 1] = np.inf
    src[5::53, 2] = -np.inf
    launches(gpu, orc, tgt, src, [np.eye(4, dtype=np.float32), shift(0.7, 0.2, 0.0), np.eye(4, dtype=np.float32)])


def test_sparse_source_against_a_large_target(gpu, orc):
    # 256 queries spread over 200k points: the launch runs with fewer than 64 queries per wavefront
    from pcl_amd import synth
    tgt = synth.family_cloud("sheet", 200_000, 21)
    rng = np.random.default_rng(22)
    src = tgt[rng.integers(0, len(tgt), 256)].copy()
    src[:, :3] += (rng.normal(size=(256, 3)) * 1e-3).astype(np.float32)
    launches(gpu, orc, tgt, src, [np.eye(4, dtype=np.float32), shift(2e-3, 0.0, 0.0), np.eye(4, dtype=np.float32)])


def first_launch_with_counters(gpu, orc, tgt, src, then=()):
    """launches() with the work counters armed around the launch that starts the alignment: (groups of the launch, groups
    the stand-off body finished)"""
    gpu.stats(True)   # arm (and clear)
    launches(gpu, orc, tgt, src, [np.eye(4, dtype=np.float32)])
    st = gpu.stats(False)
    if then:
        launches(gpu, orc, tgt, src, [np.eye(4, dtype=np.float32)] + list(then))
    return (len(src) + 63) // 64, st["so_done"]


def test_launch_that_starts_an_alignment_at_a_stand_off(gpu, orc):
    # a 200k-point sheet, the source about 25 point spacings off it: the stand-off body finishes groups (the first of a run
    # and the groups behind one it gave up on go through traverse(): how many is the scheduler's business, not checked)
    from pcl_amd import synth
    tgt = synth.family_cloud("sheet", 200_000, 31)
    h = float(np.ptp(tgt[:, :2], axis=0).max()) / np.sqrt(len(tgt))
    src = synth.family_cloud("sheet", 50_000, 32)
    src[:, 2] += np.float32(25 * h)
    groups, so_done = first_launch_with_counters(gpu, orc, tgt, src, then=[shift(0.0, 0.0, -20 * h)])
    print("stand-off: %d of %d groups finished by the stand-off body" % (so_done, groups))
    assert 0 < so_done <= groups


def test_stand_off_body_falls_back_to_traverse(gpu, orc):
    # the same launch, but half of the source lies ON the sheet: its groups' radii are below the stand-off threshold, the
    # stand-off body seeds their lanes, gives up and hands them to traverse() with the bounds reached so far -- the
    # fallback whose winners resolve() then finds.  One launch, so the counters prove both: some groups were finished by
    # the stand-off body (it ran), and the others were not (they went through the fallback).
    from pcl_amd import synth
    tgt = synth.family_cloud("sheet", 200_000, 31)
    h = float(np.ptp(tgt[:, :2], axis=0).max()) / np.sqrt(len(tgt))
    src = synth.family_cloud("sheet", 50_000, 33)
    off = src[:, 0] < np.median(src[:, 0])
    src[off, 2] += np.float32(25 * h)
    groups, so_done = first_launch_with_counters(gpu, orc, tgt, src)
    print("mixed: %d of %d groups finished by the stand-off body" % (so_done, groups))
    assert 0 < so_done < groups


def test_unseeded_launch_with_the_stand_off_gate_closed(gpu, orc):
    # gate closed: the launch that starts the alignment never enters the stand-off body; the seeded kernel walks from the
    # root with the disc bounds (loose walk, pair mode) -- another way to the same matches
    from pcl_amd import synth
    tgt = synth.family_cloud("sheet", 200_000, 31)
    h = float(np.ptp(tgt[:, :2], axis=0).max()) / np.sqrt(len(tgt))
    src = synth.family_cloud("sheet", 50_000, 32)
    src[:, 2] += np.float32(25 * h)
    gpu.setOption("standoff_thickness", 0.0)
    try:
        groups, so_done = first_launch_with_counters(gpu, orc, tgt, src)
    finally:
        gpu.setOption("standoff_thickness", 0.3)
    assert so_done == 0


# ---- five steps of the device-driven loop -----------------------------------------------------------------------------
LOOP_POINTS = 1 << 17


def seeded_body_runs_two_deep(n_src, cus, blocks_per_cu, deep_from):
    """the host's rule (search.hip: launch_icp_iterate / persistent_blocks): the seeded body's pipeline runs two groups deep
    from `deep_from` groups per wave of the persistent grid on"""
    groups = (n_src + 63) // 64
    grid = max(1, min((groups + 3) // 4, max(8, cus * blocks_per_cu)))
    return groups >= deep_from * grid * 4


def same_pairs(got, want):
    (q, m, d), (oq, om, od) = got, want
    return np.array_equal(q, oq) and np.array_equal(m, om) and np.array_equal(d.view(np.uint32), od.view(np.uint32))


def loop_icp(gpu, tgt, src, max_iterations):
    import pcl_amd
    icp = pcl_amd.IterativeClosestPoint(gpu)
    icp.setInputTarget(tgt)
    icp.setInputSource(src)
    icp.setMaximumIterations(max_iterations)
    icp.setMaxCorrespondenceDistance(0.1)
    icp.setTransformationEpsilon(1e-12)
    return icp


def test_pipeline_depth_of_the_loop_case():
    """Which seeded body the five-step case below runs.  On the device a 2^17-point launch is far below 12 groups per wave: the
    one-deep body; the two-deep body on the device is tests/test_gpu_fullsize.py::
    test_config3_device_driven_loop_correspondences_bit_exact_at_10m (10M points, every iteration's correspondences bit for
    bit) -- asserted here for every occupancy the kernel can have.  On the emulation (2 blocks per compute unit, two deep
    from 2 groups per wave) the number of compute units decides: tests/test_resolve_half_wavesim.py runs the case with 16
    (two deep) and with 1024 (one deep) and says which it expects in PCLHIP_EXPECT_DEEP."""
    import test_gpu_fullsize
    lib = os.environ.get("PCLHIP_LIB", "")
    if "wavesim" in lib:
        cus = int(os.environ.get("WAVESIM_CUS", "16"))
        deep = seeded_body_runs_two_deep(LOOP_POINTS, cus, 2, 2)
        if "PCLHIP_EXPECT_DEEP" in os.environ:
            assert deep == (os.environ["PCLHIP_EXPECT_DEEP"] == "1"), (cus, deep)
    else:
        # whatever the device's persistent grid is between 43 and 3,255 resident blocks (an MI355X: 256 compute units x 4
        # blocks by the dual kernel's LDS = 1,024): 2^17 points run one deep, the 10M points of that test two deep
        assert hasattr(test_gpu_fullsize, "test_config3_device_driven_loop_correspondences_bit_exact_at_10m")
        for resident in (43, 256, 512, 1024, 2048, 3255):
            assert not seeded_body_runs_two_deep(LOOP_POINTS, resident, 1, 12), resident
            assert seeded_body_runs_two_deep(test_gpu_fullsize.N3, resident, 1, 12), resident


def test_five_steps_of_the_device_driven_loop(gpu, orc):
    """One alignment of 5 steps through runSteps at 2^17 points (the pattern of tests/test_gpu_step_lean.py).  Every
    iteration's correspondences -- index and float distance bits -- equal the oracle's on a cloud moved by the device's own
    increments; the step records of runSteps equal the alignments that end after K = 1..5 iterations bit for bit
    (transformation, mean squared error, pair count), and what fetchCorrespondences returns behind the fifth step is the
    fifth search's oracle pairs."""
    import pcl_amd
    tgt, src, _ = pcl_amd.synth.icp_pair(LOOP_POINTS)
    otree = orc.KdTree(tgt)
    ends, want = [], []
    gpu.setOption("icp_lookahead", 0)
    try:
        cur = src.copy()
        for K in range(1, 6):
            icp = loop_icp(gpu, tgt, src, K)
            icp.align()
            assert icp.nr_iterations_ == K
            want.append(otree.correspondences(cur, 0.1))
            assert same_pairs(icp.fetchCorrespondences(), want[-1]), K
            ends.append((icp.getFinalTransformation().copy(), float(icp.result.mse), int(icp.result.num_correspondences)))
            cur = orc.transform_cloud(icp.getLastIncrementalTransformation(), cur, order=0)
    finally:
        gpu.setOption("icp_lookahead", 1)
    dev = loop_icp(gpu, tgt, src, 20)
    steps = dev.runSteps(5)
    assert [s["iteration"] for s in steps] == [1, 2, 3, 4, 5] and not any(s["alignment_ended"] for s in steps)
    for K, (s, (T, mse, pairs), (oq, om, od)) in enumerate(zip(steps, ends, want), 1):
        assert np.array_equal(s["final_transformation"], T), K
        assert s["num_correspondences"] == pairs == len(oq), K
        print("step %d: mse %.9g (alignment of %d iterations %.9g, oracle's pairs %.9g)" % (K, s["mse"], K, mse, od.astype(np.float64).mean()))
        assert s["mse"] == mse, K
        assert abs(s["mse"] - od.astype(np.float64).mean()) <= 1e-6 * od.astype(np.float64).mean(), K
    assert same_pairs(dev.fetchCorrespondences(), want[4])


WORKER = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import pcl_amd
tgt, src, _ = pcl_amd.synth.icp_pair(1 << 17)
icp = pcl_amd.IterativeClosestPoint(pcl_amd.Context(0))
icp.setInputTarget(tgt)
icp.setInputSource(src)
icp.setMaximumIterations(20)
icp.setMaxCorrespondenceDistance(0.1)
icp.setTransformationEpsilon(1e-12)
steps = icp.runSteps(5)
q, m, d = icp.fetchCorrespondences()
np.savez(sys.argv[2], T=np.stack([s["final_transformation"] for s in steps]), mse=np.array([s["mse"] for s in steps]),
         pairs=np.array([s["num_correspondences"] for s in steps]), it=np.array([s["iteration"] for s in steps]), q=q, m=m, d=d)
"""


def run_worker(lib, out):
    env = dict(os.environ)
    if lib is not None:
        env["PCLHIP_LIB"] = lib
    r = subprocess.run([sys.executable, "-c", WORKER, ROOT, out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return np.load(out)


def test_five_steps_byte_equal_to_a_build_of_the_parent_commit(tmp_path):
    """Where somebody has put a library built from the parent commit under pcl_amd/variants/ (an A/B artefact, never part of
    the tree): the same five steps in two processes, records and correspondences byte for byte.  Without it the case above,
    against the oracle, is the whole check and this one has nothing to add."""
    parent = os.path.join(ROOT, "pcl_amd", "variants", "libpclhip_parent.so")
    if not os.path.exists(parent) or "wavesim" in os.environ.get("PCLHIP_LIB", ""):
        return
    new, old = run_worker(None, str(tmp_path / "new.npz")), run_worker(parent, str(tmp_path / "old.npz"))
    for k in ("T", "mse", "pairs", "it", "q", "m", "d"):
        assert new[k].tobytes() == old[k].tobytes(), k
