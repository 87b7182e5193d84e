"""tests/voxelgrid_restatement.py pinned without a GPU, before the device is compared with it
(tests/test_gpu_voxelgrid_regimes.py):

  * against the CPU oracle (oracle/pcl_oracle.c: orc_voxelgrid), x y z 1 and voxel ids, exact, on 300 small random clouds
    (sizes 1 ... 5,000, anisotropic leaves, negative coordinates, NaN / inf records, every filter field, both signs of
    `negative`, min_points 0 ... 5) and on grids that the oracle refuses;
  * against tests/golden/golden.json: voxelgrid_bun0;
  * against the reference's own 16-point VoxelGrid_XYZNormal scene (test/filters/test_filters.cpp:1088-1231);
  * the two deliberately wrong variants (descending summation, unstable ties) must differ on a stated share of the voxels
    of a fixed cloud: the comparison is exact, and the inputs are order-sensitive.

All comparisons are exact (bytes; NaN positions only)."""
import numpy as np
import pytest

import voxelgrid_restatement as vr
from oracle import pcl_oracle as orc

F = np.float32
FIELDS = (0, 1, 2, 4, 5, 6, 8)


def fuzz_case(seed):
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([1, 2, 3, 17, 100, 700, 2000, 5000])) if seed % 3 else int(rng.integers(1, 5001))
    wide = bool(rng.random() < 0.6)
    cloud = np.zeros((n, 12 if wide else 4), F)
    kind = int(rng.integers(0, 4))
    if kind == 0:   xyz = rng.uniform(-1, 1, (n, 3))
    elif kind == 1: xyz = rng.normal(size=(n, 3)) * np.array([5.0, 0.2, 1.0])
    elif kind == 2: xyz = np.round(rng.uniform(-4, 4, (n, 3)))                         # points on cell faces, duplicates
    else:           xyz = rng.uniform(-1, 0, (n, 3)) * np.array([1.0, 1e-3, 50.0])     # all negative, anisotropic
    cloud[:, :3] = (xyz * float(10 ** rng.uniform(-1, 1)) + rng.uniform(-3, 3, 3) * (rng.random() < 0.5)).astype(F)
    cloud[:, 3] = 1
    if wide:
        cloud[:, 4:7] = rng.normal(size=(n, 3)).astype(F)
        cloud[:, 8] = rng.uniform(0, 1, n).astype(F)
    if n > 5 and rng.random() < 0.5:
        k = max(1, n // 20)
        cloud[rng.integers(0, n, k), rng.integers(0, 3, k)] = rng.choice([np.nan, np.inf, -np.inf], k)
        if wide:
            cloud[rng.integers(0, n, k), rng.choice([4, 8], k)] = rng.choice([np.nan, np.inf, -np.inf], k)
    fin = cloud[:, :3][np.isfinite(cloud[:, :3]).all(1)]
    ext = float(np.ptp(fin)) + 1e-3 if len(fin) else 1.0
    leaf = (ext * 10 ** rng.uniform(-2.0, -0.2, 3)).astype(F)
    if seed % 10 == 9:
        leaf = (leaf * F(1e-4)).astype(F)                                              # grids that are refused
    kw = dict(min_points=int(rng.integers(0, 6)))
    if rng.random() < 0.7:
        col = int(rng.choice([f for f in FIELDS if f < cloud.shape[1]]))
        v = cloud[:, col][np.isfinite(cloud[:, col])]
        lo, hi = sorted(np.quantile(v, rng.uniform(0, 1, 2)).tolist()) if len(v) else (0.0, 1.0)
        if rng.random() < 0.3:
            lo, hi = lo + 1e-9, hi - 1e-9 if hi - lo > 1e-6 else hi                     # limits that are not floats
        kw.update(field=col, limits=(lo, hi), negative=bool(rng.random() < 0.5))
    return cloud, leaf, kw


@pytest.mark.parametrize("block", range(10))
def test_restatement_equals_the_oracle_on_small_random_clouds(block):
    refused = 0
    for seed in range(block * 30, block * 30 + 30):
        cloud, leaf, kw = fuzz_case(seed)
        okw = dict(min_points_per_voxel=kw["min_points"])
        if "field" in kw:
            okw.update(limits=kw["limits"], field=kw["field"], negative=kw["negative"])
        got = vr.voxelgrid(cloud, leaf, **kw)
        if got is not None and not got["box"]:
            continue                                    # no record in the box: the reference's grid is undefined
        want, ids = orc.voxelgrid(cloud, leaf, **okw)
        if want is None:
            assert got is None, seed
            refused += 1
            continue
        assert got is not None, seed
        assert np.array_equal(got["ids"], ids), seed
        assert vr.same_bytes(got["out"][:, :4], want), (seed, vr.first_difference(got["out"][:, :4], want))
        if cloud.shape[1] == 12:                        # the coordinates do not depend on downsample_all_data
            xyz_only = vr.voxelgrid(cloud, leaf, downsample_all_data=False, **kw)
            assert vr.same_bytes(xyz_only["out"][:, :4], want) and not xyz_only["out"][:, 4:].any()
            assert not got["out"][:, [7, 9, 10, 11]].any()
        lay = got["layout"]
        if lay is not None:
            assert np.array_equal(np.flatnonzero(lay >= 0), ids) and np.array_equal(lay[ids], np.arange(len(ids)))
    assert refused >= 1                                 # seeds 9, 19, 29 of every block shrink their leaf by 1e-4


def test_the_refusal_sits_where_the_oracle_puts_it():
    """1290^3 cells are the largest cube below 2^31; one more layer is refused (:624)"""
    for cells, refused in (((1290, 1290, 1290), False), ((1291, 1290, 1290), True)):
        corners = np.array([[0.5, 0.5, 0.5], [cells[0] - 0.5, cells[1] - 0.5, cells[2] - 0.5]], F)
        got = vr.voxelgrid(corners, 1.0, with_layout=False)
        want, ids = orc.voxelgrid(np.c_[corners, np.ones(2, F)], 1.0)
        assert (got is None) == refused and (want is None) == refused
        if not refused:
            assert np.array_equal(got["ids"], ids) and ids[-1] == 1290 ** 3 - 1
            assert (got["sort_bits"], got["passes"]) == (32, 4)


def test_restatement_bunny_golden(bunny, golden):
    # test/filters/test_filters.cpp:566-596
    g = golden["voxelgrid_bun0"]
    cloud = bunny["bun0"]
    assert len(vr.voxelgrid(cloud, g["leaf"])["out"]) == g["count"]
    out = vr.voxelgrid(cloud, g["leaf"], field=2, limits=(g["z_min"], g["z_max"]))["out"]
    assert len(out) == g["count_z"]
    assert np.allclose(out[0, :3], g["first_z"], atol=g["tol"])
    assert np.allclose(out[-1, :3], g["last_z"], atol=g["tol"])


def xyznormal_scene(seed=1088):
    """The 16 points of TEST (VoxelGrid_XYZNormal, Filters), test/filters/test_filters.cpp:1098-1201, from a fixed seed:
    2 x 2 x 2 voxels of two points each.  -> (cloud (16, 12), per voxel in output order: (a, b, kind))"""
    rng = np.random.default_rng(seed)
    cloud = np.zeros((16, 12), F)
    cloud[:, 3] = 1
    voxels = []
    for z in range(2):
        for y in range(2):
            for x in range(2):
                a = np.zeros(12, F)
                a[3] = 1
                a[:3] = F(1.99) * np.array([x, y, z], F)
                nrm = rng.uniform(-1, 1, 3).astype(F)
                a[4:7] = nrm / np.sqrt((nrm * nrm).sum(dtype=F))
                b = a.copy()
                if x != 0:
                    b[:3] = (rng.uniform(0, 0.99, 3) + np.array([x, y, z])).astype(F)
                if (y, z) == (0, 0):   kind = "opposite";   b[4:7] = -a[4:7]
                elif (y, z) == (0, 1): kind = "nan";        b[4:7] = np.nan
                elif (y, z) == (1, 0): kind = "orthogonal"; b[4:7] = [a[5] - a[6], a[6] - a[4], a[4] - a[5]]
                else:                  kind = "random";     b[4:7] = rng.uniform(-1, 1, 3).astype(F)
                cloud[2 * len(voxels)] = a
                cloud[2 * len(voxels) + 1] = b
                voxels.append((a, b, kind))
    return cloud, voxels


def test_restatement_on_the_reference_xyznormal_scene():
    """Leaf 1, filter field unset as in the reference test (its setFilterLimits (0, 2) has no field to act on).  Centroids are
    the scene's own (a + b) * 0.5, exactly.  Opposite normals sum to 0 and normalise to NaN.  A NaN member makes the sum
    and so the normal NaN: AccumulatorNormal::add adds whatever it is given and get() normalises the sum
    (accumulators.hpp:99-105).  The reference test's ground truth keeps the first member's normal for that voxel and its
    comparison would fail on it; the code is followed here, not that table.  The orthogonal and the random voxels are the
    sum of the two members (the second NOT normalised first, as add() takes it) over its float norm."""
    cloud, voxels = xyznormal_scene()
    got = vr.voxelgrid(cloud, 1.0)
    assert np.array_equal(got["ids"], np.arange(8)) and np.array_equal(got["div_b"], [2, 2, 2])
    assert np.array_equal(got["counts"], np.full(8, 2))
    out = got["out"]
    seen = set()
    for v, (a, b, kind) in enumerate(voxels):
        seen.add(kind)
        assert np.array_equal(out[v, :3], ((a[:3] + b[:3]).astype(F) * F(0.5)).astype(F)), v
        assert out[v, 3] == 1 and not out[v, [7, 9, 10, 11]].any() and out[v, 8] == 0
        if kind in ("opposite", "nan"):
            assert np.isnan(out[v, 4:7]).all(), (v, kind)
            continue
        s = (a[4:7] + b[4:7]).astype(F)
        q = (s * s).astype(F)
        want = s / np.sqrt(F(F(q[0] + q[1]) + q[2]))
        assert np.array_equal(out[v, 4:7], want), (v, kind)
        assert abs(np.linalg.norm(out[v, 4:7].astype(np.float64)) - 1) < 1e-6
    assert seen == {"opposite", "nan", "orthogonal", "random"}
    # without downsample_all_data only x y z 1
    bare = vr.voxelgrid(cloud, 1.0, downsample_all_data=False)["out"]
    assert np.array_equal(bare[:, :4], out[:, :4]) and not bare[:, 4:].any()


def order_cloud():
    rng = np.random.default_rng(50_000)
    cloud = np.zeros((50_000, 12), F)
    cloud[:, :3] = rng.normal(size=(50_000, 3)).astype(F)
    cloud[:, 3] = 1
    cloud[:, 4:7] = rng.normal(size=(50_000, 3)).astype(F)
    cloud[:, 8] = rng.uniform(0, 1, 50_000).astype(F)
    return cloud


def test_wrong_variants_are_seen_on_a_fixed_cloud():
    """50,000 normal points, leaf 0.25.  A voxel of one or two points has one possible sum, so only voxels of three and
    more can tell an order.  Reversing the run or the ties changes the float sum of three random values in at least one of
    the seven summed columns far more often than not: at least HALF of those voxels must differ for either variant (the
    shares observed are printed), and no voxel of one or two points may.  The two variants reverse the same runs, so their
    sums -- not their ids -- agree with each other."""
    cloud = order_cloud()
    right = vr.voxelgrid(cloud, 0.25)
    oracle_xyz, ids = orc.voxelgrid(cloud, 0.25)
    assert np.array_equal(right["ids"], ids) and vr.same_bytes(right["out"][:, :4], oracle_xyz)
    many = right["counts"] >= 3
    assert many.sum() > 3000 and right["longest"] >= 40
    outs = {}
    for order in ("descending", "unstable"):
        wrong = vr.voxelgrid(cloud, 0.25, order=order)
        assert np.array_equal(wrong["ids"], right["ids"]) and np.array_equal(wrong["counts"], right["counts"])
        differs = (wrong["out"].view(np.uint32) != right["out"].view(np.uint32)).any(1)
        xyz_differs = (wrong["out"][:, :3].view(np.uint32) != right["out"][:, :3].view(np.uint32)).any(1)
        print("%s: %d of %d voxels of three and more differ (%d in x y z alone)" % (order, differs[many].sum(), many.sum(),
                                                                                     xyz_differs[many].sum()))
        assert not differs[~many].any()
        assert differs[many].sum() >= many.sum() // 2
        assert xyz_differs[many].sum() >= many.sum() // 2
        outs[order] = wrong["out"]
    assert vr.same_bytes(outs["descending"], outs["unstable"])


def test_run_sums_is_a_sequential_sum():
    """the helper on float sums worked out by hand: 2^24, 1, 1, -2^24 is 0 from the front (each 1 is absorbed) and 2 from
    the back; 1, 2^24, -2^24, 1 is 1 from the front and 2 from the back"""
    big = F(2 ** 24)
    v = np.array([[big], [1], [1], [-big], [1], [big], [-big], [1], [3]], F)
    order = np.arange(9)
    s = vr.run_sums(v, order, np.array([0, 4, 8]), np.array([4, 4, 1]))
    assert s[:, 0].tolist() == [0.0, 1.0, 3.0]            # (2^24 + 1 + 1) - 2^24 = 0;  ((1 + 2^24) - 2^24) + 1 = 1
    s = vr.run_sums(v, order, np.array([0, 4, 8]), np.array([4, 4, 1]), descending=True)
    assert s[:, 0].tolist() == [2.0, 2.0, 3.0]            # ((-2^24 + 1) + 1) + 2^24 = 2;  ((1 - 2^24) + 2^24) + 1 = 2
