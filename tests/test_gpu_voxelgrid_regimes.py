"""VoxelGrid off the easy path: the device (pcl_amd/csrc/voxelgrid.hip) against tests/voxelgrid_restatement.py.

Contract of every case: the WHOLE output record (x y z 1 | nx ny nz 0 | curvature 0 0 0 for 12-column pcl::PointNormal
clouds), the grid dims and, where it is on, the whole leaf layout are compared EXACTLY (bytes; NaN positions must agree, a
NaN's sign and payload are not pinned); every device call is made TWICE and the two results are the same bytes; both values
of downsample_all_data.  No tolerance anywhere.  Where a box exists the coordinates and voxel ids are compared with the CPU
oracle as well.  Normals are random and NOT normalised, curvatures are random, and in some voxels four members carry
2^24, 1, 1, -2^24 in input order: the float sums tell every other order of summation apart
(tests/test_voxelgrid_restatement.py proves that for the restatement's two wrong variants).

What each group is aimed at (lines of voxelgrid.hip):
  a. switch          `nv > nruns * 8` in voxelgrid_run (:892): vg_centroid_kernel at 800 points in 100 voxels,
                     vg_centroid_row_kernel with one point more
  b. run lengths     vg_centroid_row_kernel (:505-589): chunks of 16 (`on = c + j < len`, :552), the two-chunk prefetch and
                     its hand-over (:540-547, :564-565), `longest` over the four rows of a wave (:518-520), dropped runs
                     (`keep[r]`, :515), rows without a run, vg_keep_kernel and vg_layout_kernel
                     (the `longest` exchange itself cannot be told from `len` by any output: a row's shuffles read the
                     row's own sixteen lanes only, and those share one `len`; what the cases pin is that rows of 1 to
                     1,000 members in one wave do not disturb each other)
  c. second round    `rounds` / `it` (:512-514) and the second trip of vg_key_kernel's grid-stride loop (:109)
  d. key widths      `sort_bits = id_bits + 1` (:823-825), the all-ones key of rejected records (:134), one to four passes
                     of the filter's own sort loop (:829-837), the refusal (:776-781)
  e. seams           4,096 keys per sort / run block, 1,024 per wave (rs_scatter_kernel :347, vg_load_pairs :166-174),
                     the end sentinel of vg_runstart_kernel (:240), nv < n, nv = 0 (:863), n = 0 (:693)
  f. filter edges    vg_minmax_kernel (:62-68: float limits) against vg_key_kernel (:130-133: double limits)
  g. coordinates     the key expression (:136-139) and the grid (:774-791) on cell faces, far from the origin, on
                     degenerate boxes, anisotropic leaves and denormals
  h. layouts         record strides, device-resident clouds, a context's scratch after a larger cloud (:733)

Cases whose name holds `fullgrid` size themselves from the device's CU count and cases with `torch` need device tensors:
tests/test_voxelgrid_wavesim.py runs all the others on the wavefront emulation in the CPU tier."""
import numpy as np
import pytest

import voxelgrid_restatement as vr

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
NAMES = {0: "x", 1: "y", 2: "z", 4: "normal_x", 5: "normal_y", 6: "normal_z", 8: "curvature"}
BIG = F(2 ** 24)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


# ---- clouds ----------------------------------------------------------------------------------------------------------------
def wide(xyz, rng):
    """(n, 12) PointNormal records over the coordinates: random normals that are not normalised, random curvature"""
    n = len(xyz)
    cloud = np.zeros((n, 12), F)
    cloud[:, :3] = np.asarray(xyz, F)
    cloud[:, 3] = 1
    cloud[:, 4:7] = rng.normal(size=(n, 3)).astype(F)
    cloud[:, 8] = rng.uniform(0, 1, n).astype(F)
    return cloud


def plant(cloud, cell, rng, valid=None, share=0.4):
    """in `share` of the cells with four valid records and more, four members that follow each other in input order get the
    curvatures 2^24, 1, 1, -2^24: summed in that order the ones are absorbed, in any other order they are not"""
    idx = np.arange(len(cloud)) if valid is None else np.flatnonzero(valid)
    order = idx[np.argsort(cell[idx], kind="stable")]
    sc = cell[order]
    heads = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
    counts = np.diff(np.r_[heads, len(sc)])
    for h, c in zip(heads, counts):
        if c >= 4 and rng.random() < share:
            s = h + int(rng.integers(0, c - 3))
            cloud[order[s:s + 4], 8] = [BIG, 1, 1, -BIG]
    return cloud


def line_cloud(lengths, rng, shuffle=True):
    """cell i of a line along x (leaf 1) holds lengths[i] records at i + U(0.1, 0.9), U(0.1, 0.9), U(0.1, 0.9); consecutive
    voxel ids are consecutive runs.  -> (cloud (n, 12), cell of every record)"""
    cell = np.repeat(np.arange(len(lengths)), lengths)
    if shuffle:
        cell = cell[rng.permutation(len(cell))]
    xyz = rng.uniform(0.1, 0.9, (len(cell), 3))
    xyz[:, 0] += cell
    return plant(wide(xyz, rng), cell, rng), cell


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def device(gpu, cloud, leaf, all_data, min_points=0, field=None, limits=None, negative=False, layout=False):
    """-> (records, VoxelGrid) of two calls that gave the same bytes"""
    import pcl_amd
    vg = pcl_amd.VoxelGrid(gpu)
    vg.setInputCloud(cloud)
    vg.setLeafSize(*[float(v) for v in np.broadcast_to(np.asarray(leaf, F), 3)])
    vg.setMinimumPointsNumberPerVoxel(min_points)
    vg.setDownsampleAllData(all_data)
    vg.setSaveLeafLayout(layout)
    if field is not None:
        vg.setFilterFieldName(NAMES[field])
        if limits is not None:
            vg.setFilterLimits(*limits)
        vg.setFilterLimitsNegative(negative)
    out = np.array(vg.filter())
    lay = np.array(vg.getLeafLayout())
    again = vg.filter()
    assert out.tobytes() == again.tobytes() and out.shape == again.shape, "two runs differ"
    assert lay.tobytes() == vg.getLeafLayout().tobytes(), "two runs: layouts differ"
    return out, vg


def check(gpu, orc, cloud, leaf, layout=True, min_points=0, field=None, limits=None, negative=False):
    """the device against the restatement for both values of downsample_all_data -> the restatement's dict"""
    first = None
    for all_data in (True, False):
        lim = None if field is None else ((-FLT_MAX, FLT_MAX) if limits is None else limits)   # voxel_grid.h:503-512
        ref = vr.voxelgrid(cloud, leaf, min_points=min_points, field=field, limits=lim, negative=negative,
                           downsample_all_data=all_data, with_layout=layout)
        assert ref is not None, "the restatement refuses this grid"
        first = first or ref
        out, vg = device(gpu, cloud, leaf, all_data, min_points, field, limits, negative, layout)
        assert vr.same_bytes(out, ref["out"]), (all_data, vr.first_difference(out, ref["out"]))
        if not ref["box"]:
            continue
        assert np.array_equal(vg.getMinBoxCoordinates(), ref["min_b"]) and np.array_equal(vg.getNrDivisions(), ref["div_b"])
        assert np.array_equal(vg.getMaxBoxCoordinates(), ref["max_b"]) and np.array_equal(vg.getDivisionMultiplier(), ref["mul"])
        if layout:
            assert ref["layout"] is not None and np.array_equal(vg.getLeafLayout(), ref["layout"]), all_data
        else:
            assert len(vg.getLeafLayout()) == 0
        if all_data:
            okw = {} if field is None else dict(limits=lim, field=field, negative=negative)
            want, ids = orc.voxelgrid(cloud, np.array(np.broadcast_to(np.asarray(leaf, F), 3)), min_points_per_voxel=min_points, **okw)
            assert np.array_equal(ids, ref["ids"]) and vr.same_bytes(out[:, :4], want)
    return first


# ---- a. the switch between the two centroid kernels ------------------------------------------------------------------------
def switch_cloud(extra):
    rng = np.random.default_rng(800)
    cloud, cell = line_cloud([8] * 100, rng)
    if extra:
        one = wide([[37.5, 0.5, 0.5]], rng)
        cloud, cell = np.r_[cloud, one], np.r_[cell, 37]
    # 60 rejected records in between (a NaN coordinate): n > nv
    at = np.sort(rng.choice(len(cloud), 60, replace=False))
    bad = wide(rng.uniform(0.1, 0.9, (60, 3)) + [[50, 0, 0]], rng)
    bad[np.arange(60), rng.integers(0, 3, 60)] = np.nan
    return np.insert(cloud, at, bad, axis=0)


@pytest.mark.parametrize("extra", [0, 1])
def test_a_switch_between_the_centroid_kernels(gpu, orc, extra):
    """voxelgrid_run launches the row kernel when `uint64_t(nv) > uint64_t(nruns) * 8`.  100 voxels of 8 valid points:
    nv = 800, nruns = 100, 800 > 800 is false -> vg_centroid_kernel (a thread per voxel).  One more point in voxel 37:
    801 > 800 -> vg_centroid_row_kernel.  Derived from that line, not probed."""
    cloud = switch_cloud(extra)
    ref = check(gpu, orc, cloud, 1.0)
    assert (ref["nv"], ref["nruns"]) == (800 + extra, 100) and len(cloud) == 860 + extra
    assert (ref["nv"] > 8 * ref["nruns"]) == bool(extra)


# ---- b. run lengths in the row kernel ---------------------------------------------------------------------------------------
WAVES = [(1, 49, 16, 1000), (33, 1, 1, 17), (15, 31, 32, 47), (48, 100, 17, 16)]   # four consecutive runs share a wave
PATTERN = [v for w in WAVES for v in w]
RUN_LENGTHS = [PATTERN[i % 16] for i in range(38)]


@pytest.fixture(scope="module")
def runs_cloud():
    return line_cloud(RUN_LENGTHS, np.random.default_rng(38))


@pytest.mark.parametrize("min_points", [0, 16, 17, 1000, 1001])
def test_b_run_lengths_in_the_row_kernel(gpu, orc, runs_cloud, min_points):
    """Lengths at the chunk size (16) and at the prefetch depth (32, 48), each with its neighbours; the four rows of a wave
    from 1 to 1,000 long; 38 runs leave two rows of the last wave and ten rows of the last block without a run.  With
    min_points at a present length and one above it the dropped runs sit between kept ones and their cells read -1."""
    cloud, cell = runs_cloud
    lengths = np.bincount(cell)
    assert np.array_equal(lengths, RUN_LENGTHS) and set(PATTERN) == {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 1000}
    assert tuple(lengths[0:4]) == WAVES[0] and tuple(lengths[4:8]) == WAVES[1]           # runs 4w .. 4w + 3: wave w
    nruns, nv = len(lengths), int(lengths.sum())
    assert nruns % 4 != 0 and nruns % 16 != 0 and nv > 8 * nruns                         # the row kernel, partly filled
    ref = check(gpu, orc, cloud, 1.0, min_points=min_points)
    assert (ref["nv"], ref["nruns"], ref["longest"]) == (nv, nruns, 1000)
    kept = lengths >= min_points
    assert np.array_equal(ref["ids"], np.flatnonzero(kept)) and np.array_equal(ref["layout"] >= 0, kept)
    if min_points:
        assert min_points in lengths or min_points - 1 in lengths
        dropped = np.flatnonzero(~kept)
        between = [d for d in dropped if kept[:d].any() and kept[d + 1:].any()]
        assert (len(between) >= 3 or not kept.any()) and (ref["layout"][dropped] == -1).all()   # 1,001: nothing is kept


# ---- c. a second round of the row kernel, a second trip of the key kernel -------------------------------------------------
def nine_each(voxels, seed):
    cloud, _ = line_cloud([9] * voxels, np.random.default_rng(seed))
    return cloud


def test_c_second_round_at_sixteen_cus(gpu, orc):
    """The row kernel's grid is min(ceil(nruns / 16), 16 * CUs) blocks of 16 rows.  With the emulation's 16 CUs that is at
    most 4,096 rows: 4,133 voxels give the first 37 rows a second round (`it` = 1) and leave the others without a run in it.
    9 points a voxel keep the row kernel (9 > 8) and give vg_key_kernel (2 * CUs blocks, 4 records per thread and trip:
    2,048 * CUs = 32,768 records) a second trip.  On a larger device this is one round; the fullgrid case below scales."""
    cloud = nine_each(4133, 4133)
    ref = check(gpu, orc, cloud, 1.0)
    assert (ref["nv"], ref["nruns"]) == (9 * 4133, 4133) and ref["nv"] > 8 * ref["nruns"]
    assert 16 * min(-(-4133 // 16), 16 * 16) == 4096 and 9 * 4133 > 2048 * 16


def test_c_fullgrid_second_round(gpu, orc):
    """256 * CUs + 37 voxels of 9 points: rows = 16 * 16 * CUs, 37 voxels over; 9 * 256 * CUs > 2,048 * CUs records"""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    voxels = 256 * cus + 37
    print("fullgrid voxels: %d CUs -> %d voxels, %d points" % (cus, voxels, 9 * voxels))
    cloud = nine_each(voxels, 37)
    ref = check(gpu, orc, cloud, 1.0, layout=False)
    assert ref["nruns"] == voxels and 16 * min(-(-voxels // 16), 16 * cus) == voxels - 37


# ---- d. sort key widths ------------------------------------------------------------------------------------------------------
KEY_GRIDS = [((128, 1, 1), 1, 8), ((129, 1, 1), 2, 9), ((32, 32, 32), 2, 16), ((33, 32, 32), 3, 17),
             ((256, 256, 128), 3, 24), ((256, 256, 129), 4, 25), ((1290, 1290, 1290), 4, 32)]


def grid_cloud(cells, seed):
    """about 3,000 random occupied cells of an a x b x c grid of leaf 1 plus both corner cells, one to four records a cell
    at cell + U(0.1, 0.9).  Every seventh record has a NaN coordinate and normal_x < -1 rejects some more (their curvature
    is inf: a rejected record that reached a sum would show); the corner records are valid.
    -> (cloud, valid, voxel id of every record)"""
    rng = np.random.default_rng(seed)
    a, b, c = cells
    total = a * b * c
    occupied = np.unique(np.r_[rng.integers(0, total, min(3000, 4 * total)), 0, total - 1])
    per = rng.integers(1, 5, len(occupied))
    ids = np.repeat(occupied, per)
    ids = ids[rng.permutation(len(ids))]
    ids[1], ids[2] = 0, total - 1                                              # the corners, at valid positions
    ijk = np.c_[ids % a, (ids // a) % b, ids // (a * b)]
    cloud = wide(ijk + rng.uniform(0.1, 0.9, (len(ids), 3)), rng)
    cloud[1:3, 4] = 0
    by_field = cloud[:, 4] < -1
    nan = np.arange(len(ids)) % 7 == 0
    valid = ~nan & ~by_field
    plant(cloud, ids, rng, valid)
    cloud[by_field, 8] = np.inf
    cloud[nan, rng.integers(0, 3, int(nan.sum()))] = np.nan
    return cloud, valid, ids


@pytest.mark.parametrize("cells,passes,sort_bits", KEY_GRIDS, ids=["x".join(map(str, g[0])) for g in KEY_GRIDS])
def test_d_key_widths(gpu, orc, cells, passes, sort_bits):
    """One to four passes of 8 bits, each width at its pass boundary; at a power of two the last voxel id is all ones in
    id_bits bits, one bit below the rejected records' key; 1290^3 has sort_bits = 32 and the key 0xFFFFFFFF."""
    cloud, valid, ids = grid_cloud(cells, sort_bits)
    assert (~valid).sum() > len(cloud) // 7 and valid[1] and valid[2]
    assert np.flatnonzero(~valid).max() > len(cloud) - 8 and (np.diff(np.flatnonzero(~valid)) < 40).all()   # interleaved
    total = cells[0] * cells[1] * cells[2]
    layout = total <= 256 * 256 * 129
    ref = check(gpu, orc, cloud, 1.0, layout=layout, field=4, limits=(-1.0, 100.0))
    assert np.array_equal(ref["div_b"], cells) and (ref["sort_bits"], ref["passes"]) == (sort_bits, passes)
    want_ids = np.unique(ids[valid])
    assert np.array_equal(ref["ids"], want_ids) and ref["ids"][0] == 0 and ref["ids"][-1] == total - 1
    assert ref["nv"] == valid.sum() and np.isfinite(ref["out"]).all()           # no rejected record in any sum
    if layout:
        assert len(ref["layout"]) == total and (ref["layout"] >= 0).sum() == len(want_ids)


def test_d_one_layer_more_is_refused(gpu, orc):
    """1291 x 1290 x 1290 > INT32_MAX cells: status -5, as the oracle and the restatement refuse it"""
    import pcl_amd
    cloud, valid, ids = grid_cloud((1291, 1290, 1290), 33)
    assert vr.voxelgrid(cloud, 1.0, with_layout=False) is None and orc.voxelgrid(cloud, 1.0)[0] is None
    for all_data in (True, False):
        vg = pcl_amd.VoxelGrid(gpu)
        vg.setInputCloud(cloud)
        vg.setLeafSize(1.0)
        vg.setDownsampleAllData(all_data)
        with pytest.raises(pcl_amd.PclHipError) as e:
            vg.filter()
        assert e.value.status == -5


# ---- e. seams ---------------------------------------------------------------------------------------------------------------
def seam_cloud(nv, k, where, dense, seed):
    """nv valid records (dense: 40 voxels on a line, the row kernel; else a 40 x 40 sheet, the thread kernel) and k
    rejected ones (a NaN coordinate) first, last or interleaved"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 40, (nv, 3)) * ([1, 0.02, 0.02] if dense else [1, 1, 0.02])
    cell = np.floor(xyz[:, 0]).astype(np.int64) + 40 * np.floor(xyz[:, 1]).astype(np.int64)
    cloud = plant(wide(xyz, rng), cell, rng)
    if k:
        bad = wide(rng.uniform(0, 40, (k, 3)), rng)
        bad[np.arange(k), rng.integers(0, 3, k)] = np.nan
        at = {"first": np.zeros(k, np.int64), "last": np.full(k, nv), "interleaved": np.sort(rng.integers(0, nv + 1, k))}[where]
        cloud = np.insert(cloud, at, bad, axis=0)
    return cloud


SEAMS = [4095, 4096, 4097, 8193, 1023, 1024, 1025]


@pytest.mark.parametrize("dense", [True, False], ids=["rows", "threads"])
@pytest.mark.parametrize("n", SEAMS)
def test_e_n_on_a_seam(gpu, orc, n, dense):
    ref = check(gpu, orc, seam_cloud(n, 0, None, dense, n), 1.0)
    assert ref["nv"] == n and (ref["nv"] > 8 * ref["nruns"]) == dense


@pytest.mark.parametrize("where,k", [("first", 5), ("last", 5), ("interleaved", 700), ("interleaved", 1)])
@pytest.mark.parametrize("nv", SEAMS)
def test_e_nv_on_a_seam_with_rejected_records(gpu, orc, nv, where, k):
    """the sentinel run_start[nruns] = nv is written by the thread that owns sorted position nv - 1: the last of a block,
    the first of the next, the last of a wave; the rejected records sort behind it"""
    cloud = seam_cloud(nv, k, where, True, nv + k)
    assert len(cloud) == nv + k
    ref = check(gpu, orc, cloud, 1.0)
    assert ref["nv"] == nv and np.isfinite(ref["out"]).all()


@pytest.mark.parametrize("lengths,heads,across", [([4000, 96, 50, 7], [4096], []), ([4000, 200, 50], [], [4096]),
                                                  ([4096, 1], [4096], []), ([4095, 1, 4096, 1], [4095, 4096, 8192], []),
                                                  ([4097], [], [1024, 4096]), ([1000, 24, 3000, 72, 4096, 1], [1024, 4096, 8192], [])],
                         ids=["head-at-4096", "run-across-4096", "last-run-of-one", "heads-at-4095-4096-8192", "one-voxel",
                              "heads-at-1024-4096-8192"])
def test_e_run_heads_and_runs_on_block_seams(gpu, orc, lengths, heads, across):
    """sorted positions: a run head exactly at 4,096 (first key of the second run block), a run across it, a sentinel
    behind a last run of one, and one voxel that holds all 4,097 points (one head, the sentinel in the second block)"""
    cloud, cell = line_cloud(lengths, np.random.default_rng(len(lengths) + 4096))
    ref = check(gpu, orc, cloud, 1.0)
    assert np.array_equal(ref["counts"], lengths)
    starts = np.cumsum([0] + lengths[:-1])
    assert all(h in starts for h in heads)
    assert all(((starts < a) & (starts + np.asarray(lengths) > a)).any() for a in across)


@pytest.mark.parametrize("n", [1, 2])
def test_e_one_and_two_records(gpu, orc, n):
    rng = np.random.default_rng(n)
    for spread in (0.0, 3.0):                      # the same cell, then (for n = 2) two cells
        cloud = wide(rng.uniform(0.1, 0.9, (n, 3)) + spread * np.arange(n)[:, None], rng)
        ref = check(gpu, orc, cloud, 1.0)
        assert ref["nv"] == n and len(ref["out"]) == (n if spread else 1)


def test_e_every_record_rejected(gpu, orc):
    """nv = 0.  (1) no finite record: no box, the reference's grid is undefined; the output is empty.  (2) a box exists but
    the key pass rejects every record: z = float(0.1) passes the box pass (limits cast to float: not > float(0.1)) and fails
    the key pass (> 0.1 as a double); the output is empty and every cell of the layout reads -1."""
    rng = np.random.default_rng(0)
    cloud = wide(rng.uniform(0, 5, (300, 3)), rng)
    cloud[np.arange(300), rng.integers(0, 3, 300)] = np.nan
    for all_data in (True, False):
        out, vg = device(gpu, cloud, 1.0, all_data)
        assert out.shape == (0, 12)
    cloud = wide(rng.uniform(0, 5, (300, 3)), rng)
    cloud[:, 2] = F(0.1)
    ref = check(gpu, orc, cloud, 1.0, field=2, limits=(-1.0, 0.1))
    assert ref["box"] and ref["nv"] == 0 and len(ref["out"]) == 0
    assert np.array_equal(ref["div_b"], [5, 5, 1]) and len(ref["layout"]) == 25 and (ref["layout"] == -1).all()


def test_e_empty_cloud(gpu):
    for cols in (4, 12):
        out, vg = device(gpu, np.zeros((0, cols), F), 1.0, True, layout=True)
        assert out.shape == (0, cols) and len(vg.getLeafLayout()) == 0


# ---- f. the field filter's edges ---------------------------------------------------------------------------------------------
def edge_values(lo, hi):
    flo, fhi = F(lo), F(hi)
    with np.errstate(over="ignore"):               # one float beyond FLT_MAX is inf
        return np.array([flo, fhi, np.nextafter(flo, F(-np.inf)), np.nextafter(flo, F(np.inf)), np.nextafter(fhi, F(-np.inf)),
                         np.nextafter(fhi, F(np.inf)), (flo + fhi) / 2, flo - 1, fhi + 1, np.nan, np.inf, -np.inf, 0.0, -0.0], F)


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("lo,hi", [(0.25, 0.75), (0.1, 0.7), (0.0, 0.5), (-0.5, 0.0), (None, None)],
                         ids=["floats", "not-floats", "zero-lo", "zero-hi", "default-limits"])
@pytest.mark.parametrize("field", [8, 5, 0])
def test_f_filter_edges(gpu, orc, field, lo, hi, negative):
    """Field values exactly on a limit stay for both signs of `negative` (only the open inside / outside is cut); limits
    that are no floats are floats in the box pass and doubles in the key pass, so float(0.1) > 0.1 and float(0.7) < 0.7
    decide differently there; NaN compares false and stays; -0.0 equals 0.0; with the default limits only +-inf go.  20 runs of 60:
    the row kernel runs while `curvature` is the field.  Cell 0 holds on-limit values only."""
    rng = np.random.default_rng(field * 10 + negative)
    cloud, cell = line_cloud([60] * 20, rng)
    limits = None if lo is None else ((lo + 7, hi + 7) if field == 0 else (lo, hi))   # x: inside the line of cells
    lim = limits or (-FLT_MAX, FLT_MAX)
    vals = edge_values(*lim)
    on = vals[:2]                                              # float(lo), float(hi)
    if field == 0:
        vals = vals[np.isfinite(vals) & (np.abs(vals) < 1e6)]  # a non-finite x is rejected before the filter
        on = on if lo is not None else np.array([7.25, 7.25], F)
    pick = rng.random(len(cloud)) < 0.4
    cloud[pick, field] = rng.choice(vals, int(pick.sum()))
    cloud[cell == 0, field] = on[np.arange(60) % 2]
    exact = all(float(F(v)) == v for v in lim)                 # limits that are floats: on the limit is kept, both signs
    plain = field == 0 and lo is None                          # every finite x lies inside the default limits
    if exact and not plain:
        assert vr.field_pass(on.astype(np.float64), lim[0], lim[1], negative).all()
        assert vr.field_pass(on, F(lim[0]), F(lim[1]), negative).all()
    ref = check(gpu, orc, cloud, 1.0, field=field, limits=limits, negative=negative)
    if plain:
        assert ref["nv"] == (0 if negative else len(cloud))
        return
    assert ref["nv"] > 8 * ref["nruns"] and 0 < ref["nv"] < len(cloud)     # the row kernel
    if field != 0 and exact:
        assert ref["ids"][0] == 0 and ref["counts"][0] == 60


# ---- g. coordinates ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [0.01, 0.3])
def test_g_points_on_cell_faces(gpu, orc, leaf):
    """x, y, z = float(k * leaf) for k in -60 ... 60: floor(x * (1 / leaf)) decides the cell, one float either way"""
    rng = np.random.default_rng(int(leaf * 100))
    k = rng.integers(-60, 61, (6000, 3))
    xyz = (k * leaf).astype(F)
    ref = check(gpu, orc, wide(xyz, rng), leaf)
    assert ref["min_b"].min() < -55 and ref["nruns"] > 1000


def test_g_offset_cloud(gpu, orc):
    rng = np.random.default_rng(10_000)
    ref = check(gpu, orc, wide(1e4 + rng.uniform(0, 0.5, (9000, 3)) * [1, 1, 0.1], rng), 0.01)
    assert ref["min_b"].min() >= 999_000 and ref["nruns"] > 1000


@pytest.mark.parametrize("axes", [1, 0])
def test_g_collinear_and_single_cell(gpu, orc, axes):
    """div_b = 1 on two axes (a line along y) and on all three (one cell)"""
    rng = np.random.default_rng(axes)
    xyz = rng.uniform(0.1, 0.9, (3000, 3))
    if axes:
        xyz[:, 1] += rng.integers(-20, 20, 3000)
        xyz[:, [0, 2]] = [0.3, -0.7]
    ref = check(gpu, orc, wide(xyz, rng), 1.0)
    assert np.array_equal(ref["div_b"], [1, 40, 1] if axes else [1, 1, 1])


def test_g_anisotropic_leaf(gpu, orc):
    rng = np.random.default_rng(1000)
    xyz = rng.uniform(-1, 1, (5000, 3)) * [0.02, 20, 2e4]
    ref = check(gpu, orc, wide(xyz, rng), (1e-3, 1.0, 1e3))
    assert np.array_equal(ref["div_b"], [40, 40, 40])


@pytest.mark.parametrize("leaf", [1.0, 2e-38])
def test_g_denormal_coordinates(gpu, orc, leaf):
    """|coordinates| below the smallest normal float (1.18e-38) and a little above: in one cell pair at leaf 1 (negative
    ones floor to -1), some fifty cells an axis at leaf 2e-38; sums and quotients of denormals are not flushed"""
    rng = np.random.default_rng(38)
    xyz = (rng.uniform(-1, 1, (4000, 3)) * 10.0 ** rng.uniform(-44, -36.3, (4000, 3))).astype(F)
    assert (np.abs(xyz) < np.finfo(F).tiny).mean() > 0.5
    ref = check(gpu, orc, wide(xyz, rng), leaf)
    assert np.array_equal(ref["div_b"], [2, 2, 2]) if leaf == 1.0 else ref["div_b"].min() > 20


# ---- h. layouts and residency --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [3, 4, 8, 12])
def test_h_record_layouts(gpu, orc, cols):
    """(n, 3), (n, 4) and (n, 8) clouds are coordinates with padding and come back as x y z 1; 12 columns are PointNormal"""
    rng = np.random.default_rng(cols)
    full = wide(rng.uniform(-2, 2, (5000, 3)) * [1, 1, 0.1], rng)
    full[::11, 1] = np.nan
    cloud = np.ascontiguousarray(full[:, :cols])
    for kw in ({}, dict(field=2, limits=(-0.1, 0.15)), dict(min_points=3)):
        ref = check(gpu, orc, cloud, 0.5, **kw)
        assert ref["out"].shape[1] == (12 if cols == 12 else 4) and len(ref["out"]) > 20


def test_h_torch_device_cloud(gpu, orc, runs_cloud):
    """a device tensor in, device records out: the host path's bytes"""
    import pcl_amd
    import torch
    cloud, _ = runs_cloud
    for all_data in (True, False):
        host, _ = device(gpu, cloud, 1.0, all_data, min_points=16)
        vg = pcl_amd.VoxelGrid(gpu)
        vg.setInputCloud(torch.from_numpy(cloud).cuda())
        vg.setLeafSize(1.0)
        vg.setMinimumPointsNumberPerVoxel(16)
        vg.setDownsampleAllData(all_data)
        dev = vg.filter()
        assert dev.is_cuda and dev.cpu().numpy().tobytes() == host.tobytes()
        assert vg.filter().cpu().numpy().tobytes() == host.tobytes()


def test_h_scratch_reuse_after_a_larger_cloud(gpu, orc):
    """one context filters 100,000 points, then 700: its scratch block still holds the larger cloud's keys, run starts and
    sentinel behind the smaller one's.  The second result equals the same call on a fresh context, and the restatement."""
    from conftest import make_context
    rng = np.random.default_rng(700)
    large = wide(rng.uniform(0, 30, (100_000, 3)) * [1, 1, 0.1], rng)
    small = wide(rng.uniform(0, 6, (700, 3)) * [1, 1, 0.1], rng)
    small[::9, 0] = np.nan
    used = make_context(0)
    for all_data in (True, False):
        big, _ = device(used, large, 1.0, all_data, layout=True)
        assert vr.same_bytes(big, vr.voxelgrid(large, 1.0, downsample_all_data=all_data)["out"])
        after, vg = device(used, small, 1.0, all_data, layout=True)
        fresh, vg2 = device(make_context(0), small, 1.0, all_data, layout=True)
        assert after.tobytes() == fresh.tobytes() and np.array_equal(vg.getLeafLayout(), vg2.getLeafLayout())
    check(used, orc, small, 1.0)
