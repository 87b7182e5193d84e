"""pclhip_fpfh / pcl_amd.FPFHEstimation on the device against the numpy restatement (tests/fpfh_restatement.py) and the
reference's own numbers on bun0 (tests/golden/fpfh_bun0.json).

SPFH rows: bit for bit for every point without an unstable pair (a pair whose bin a different acos / atan2 may move, see
the restatement); a point with u unstable pairs may differ by 2u in the L1 norm of its integer counts.  FPFH rows: the
restatement's float64 weighting of the DEVICE's SPFH rows within (m + 4) * 2^-24 * 100 per bin, m the neighbour count --
the bound of a sequential float32 sum of m non-negative products whose bins sum to 100 (any order), which the reference's
own order meets (tests/test_fpfh_restatement.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fpfh_restatement as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_EMULATION = os.environ.get("PCLHIP_ALLOW_WAVESIM") == "1"


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "fpfh_bun0.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def bun0():
    return fr.load_bun0()


@pytest.fixture(scope="module")
def bun0_restated(bun0):
    pts, nrm = bun0
    return {r: fr.restate(pts, nrm, r) for r in (0.02, 1.0)}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def run(gpu, pts, nrm, radius, indices=None, tree=None):
    import pcl_amd
    f = pcl_amd.FPFHEstimation(gpu)
    f.setInputCloud(pts)
    if nrm is not None:
        f.setInputNormals(nrm)
    if tree is not None:
        f.setSearchMethod(tree)
    f.setRadiusSearch(radius)
    assert f.getRadiusSearch() == radius
    f.setIndices(indices)
    out, spfh = f.computeBoth()
    return out, spfh, f.nan_count


def check_spfh(spfh, ref, label):
    """check 1: the device's SPFH rows against the restatement's"""
    u = ref["unstable"]
    share = float((u > 0).mean())
    print("%s: %d of %d points own an unstable pair (%.1f %%)" % (label, int((u > 0).sum()), len(u), 100 * share))
    assert share <= 0.10
    same = (bits(spfh) == bits(ref["spfh"])).all(axis=1)
    print("%s: %d rows differ, %d of them in points without an unstable pair" % (label, int((~same).sum()),
                                                                                 int((~same & (u == 0)).sum())))
    assert same[u == 0].all()
    counts = fr.counts_from_rows(spfh, ref["m"])
    live = ~np.isnan(ref["spfh"][:, 0])
    assert (counts[live] >= 0).all()  # every value is hist_incr added an integer number of times
    l1 = np.abs(counts - ref["counts"]).sum(axis=1)
    assert (l1[live] <= 2 * u[live]).all(), (l1[live & (l1 > 2 * u)], u[live & (l1 > 2 * u)])


def check_weighting(out, spfh, pts, radius, hoods, label):
    """check 3: the weighting pass alone -- the float64 weighting of the device's own SPFH rows"""
    _f32, f64, m = fr.weigh(spfh, pts, radius, hoods)
    assert np.array_equal(np.isnan(out), np.isnan(f64))
    bound = (m + 4) * 2.0 ** -24 * 100.0
    live = ~np.isnan(f64[:, 0])
    err = np.abs(out[live].astype(np.float64) - f64[live]).max(axis=1)
    print("%s: largest error / bound = %.4f" % (label, float((err / bound[live]).max()) if live.any() else 0.0))
    assert (err <= bound[live]).all()


def test_bun0_radius_002(gpu, bun0, bun0_restated):
    pts, nrm = bun0
    ref = bun0_restated[0.02]
    out, spfh, nans = run(gpu, pts, nrm, 0.02)
    assert nans == 0 and out.shape == (397, 33) and spfh.shape == (397, 33)
    check_spfh(spfh, ref, "bun0 r=0.02")
    check_weighting(out, spfh, pts, 0.02, ref["hoods"], "bun0 r=0.02")
    # the two outputs one at a time: the same bits
    import pcl_amd
    f = pcl_amd.FPFHEstimation(gpu)
    f.setInputCloud(pts)
    f.setInputNormals(nrm)
    f.setRadiusSearch(0.02)
    assert np.array_equal(bits(f.computeSPFH()), bits(spfh)) and np.array_equal(bits(f.compute()), bits(out))
    assert f.lastPassMs()[0] >= 0.0 and f.getSearchMethod().lastKernelMs() >= 0.0


def test_bun0_every_point_a_neighbour(gpu, bun0, bun0_restated, gold):
    """r = 1.0: 396 neighbours per point, the neighbourhood of the reference's golden test -- longer than any fixed per-lane
    list, spanning every leaf"""
    pts, nrm = bun0
    ref = bun0_restated[1.0]
    assert (ref["m"] == 397).all()
    out, spfh, nans = run(gpu, pts, nrm, 1.0)
    assert nans == 0
    g = gold["fpfhs0"]
    assert np.abs(out[0] - np.array(g["values"])).max() <= g["tolerance"]
    g = gold["spfh_row0"]
    assert np.abs(spfh[0] - np.array(g["values"])).max() <= g["tolerance"]
    check_spfh(spfh, ref, "bun0 r=1.0")
    check_weighting(out, spfh, pts, 1.0, ref["hoods"], "bun0 r=1.0")


SYNTH_N, SYNTH_SEED, SYNTH_RADIUS = 5003, 20260, 0.235


def test_synthetic_5003(gpu):
    """5,003 points (no multiple of 16 or 64) of synth's "cube" family, k = 10 normals from pclhip_normals kept in the tree,
    r = 0.235: 29.4 neighbours per point on average, and the restatement gives 6.1 % of the points an unstable pair.  Seed
    picked once.  (The "sheet" family does not meet the 10 % condition at any seed: neighbours that share their 10 nearest neighbours get normals that
    are equal up to rounding, |angle1| - |angle2| is then rounding noise, and 19 % of the points own such a pair.)"""
    import pcl_amd
    pts = np.ascontiguousarray(pcl_amd.synth.family_cloud("cube", SYNTH_N, seed=SYNTH_SEED)[:, :3])
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(pts)
    ne.setSearchMethod(tree)
    ne.setKSearch(10)
    nrm = np.ascontiguousarray(ne.compute()[:, :3])
    ref = fr.restate(pts, nrm, SYNTH_RADIUS)
    print("synthetic: %.1f neighbours per point" % float(ref["m"].mean() - 1))
    assert 25 <= ref["m"].mean() - 1 <= 35
    out, spfh, nans = run(gpu, pts, None, SYNTH_RADIUS, tree=tree)  # the normals the tree holds
    assert nans == 0
    check_spfh(spfh, ref, "synthetic")
    check_weighting(out, spfh, pts, SYNTH_RADIUS, ref["hoods"], "synthetic")


def test_edge_cases(gpu):
    rng = np.random.default_rng(11)
    pts = rng.uniform(0, 1, (200, 3)).astype(np.float32)
    pts[:, 2] *= 0.1
    nrm = rng.normal(size=(200, 3)).astype(np.float32) * np.float32([0.3, 0.3, 1.0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ISO, TWIN, DUP, BAD, NONRM = 20, 40, 41, 60, 80
    pts[ISO] = (30, 30, 30)   # no neighbour but itself
    pts[DUP] = pts[TWIN]      # an exact duplicate
    pts[BAD] = np.nan         # a record the index drops
    nrm[NONRM] = np.nan       # a point without a normal
    r = 0.2
    ref = fr.restate(pts, nrm, r)
    out, spfh, nans = run(gpu, pts, nrm, r)
    out2, spfh2, nans2 = run(gpu, pts, nrm, r)
    assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(spfh), bits(spfh2)) and nans == nans2
    check_spfh(spfh, ref, "edges")
    check_weighting(out, spfh, pts, r, ref["hoods"], "edges")
    # isolated: zeros, not NaN
    assert (spfh[ISO] == 0).all() and (out[ISO] == 0).all()
    # the duplicate is binned with f1 = f2 = f3 = 0 (bins 5 / 16 / 27) and weighs nothing (d2 == 0)
    counts = fr.counts_from_rows(spfh, ref["m"])
    others = ref["hoods"][TWIN][0]
    others = others[(others != TWIN) & (others != DUP) & (others != NONRM)]
    f1, f2, f3 = fr.pair_features(pts[TWIN], nrm[TWIN], pts[others], nrm[others])[:3]
    without = np.zeros(33, np.int64)
    b = fr.bins_of(fr.bin_coords(f1, f2, f3))
    for h in range(3):
        without[11 * h:11 * h + 11] = np.bincount(b[:, h], minlength=11)
    extra = np.zeros(33, np.int64)
    extra[[5, 16, 27]] = 1
    if ref["unstable"][TWIN] == 0:
        assert np.array_equal(counts[TWIN], without + extra)
    assert counts[TWIN][[5, 16, 27]].min() >= 1
    nb, d2 = ref["hoods"][TWIN]
    keep = nb != DUP
    assert (d2[~keep] == 0).all()
    no_dup = fr.weight_float64(spfh, nb[keep & (nb != TWIN)], d2[keep & (nb != TWIN)])
    assert np.abs(out[TWIN] - no_dup).max() <= (len(nb) + 4) * 2.0 ** -24 * 100.0
    # dropped record and missing normal: NaN rows, both counted
    assert np.isnan(out[BAD]).all() and np.isnan(spfh[BAD]).all()
    assert np.isnan(out[NONRM]).all() and np.isnan(spfh[NONRM]).all()
    assert nans == 2
    # a neighbour of the point without a normal: it counts towards hist_incr but is not binned
    near = [i for i in ref["hoods"][NONRM][0] if i != NONRM]
    assert near
    for i in near:
        assert counts[i, :11].sum() == ref["m"][i] - 2
    assert not np.isnan(out[near]).any()


def test_indices(gpu, bun0):
    pts, nrm = bun0
    full, _, _ = run(gpu, pts, nrm, 0.02)
    sel = np.arange(0, 397, 3, dtype=np.int32)
    sub, spfh, nans = run(gpu, pts, nrm, 0.02, indices=sel)
    assert sub.shape == (len(sel), 33) and nans == 0
    assert np.array_equal(bits(sub), bits(full[sel]))
    back = sel[::-1].copy()  # the queries' order is the caller's
    sub, _, _ = run(gpu, pts, nrm, 0.02, indices=back)
    assert np.array_equal(bits(sub), bits(full[back]))
    if not ON_EMULATION:  # device buffers need the GPU: everything above also runs on the emulation of the CPU tier
        import torch
        t, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
        dev, dev_spfh, nans = run(gpu, t, tn, 0.02, indices=sel)
        assert dev.is_cuda and dev_spfh.is_cuda and nans == 0
        assert np.array_equal(bits(dev.cpu().numpy()), bits(full[sel]))
        assert np.array_equal(bits(dev_spfh.cpu().numpy()), bits(spfh))


def test_errors(gpu, bun0):
    import pcl_amd
    from pcl_amd import _lib
    pts, nrm = bun0
    lib = _lib.load()
    out = np.empty((397, 33), np.float32)
    nan = C.c_uint64(0)

    def call(tree, radius):
        return lib.pclhip_fpfh(tree.h, None, 0, float(radius), C.c_void_p(out.ctypes.data), 132, None, C.byref(nan))

    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(pts)
    assert call(tree, 0.02) == -4  # PCLHIP_ERR_STATE: no normals in the index
    tree.setNormals(nrm)
    assert call(tree, 0.0) == -1 and call(tree, -1.0) == -1  # PCLHIP_ERR_INVALID
    assert call(tree, 0.02) == 0
    scaled = pcl_amd.KdTree(gpu)
    scaled.setPointRepresentation([1.0, 2.0, 1.0])
    scaled.setInputCloud(pts)
    assert call(scaled, 0.02) == -1
    f = pcl_amd.FPFHEstimation(gpu)
    f.setInputCloud(pts)
    f.setRadiusSearch(0.02)
    with pytest.raises(pcl_amd.PclHipError) as e:
        f.compute()
    assert e.value.status == -4
    bad = np.array([0, 397], np.int32)
    f.setInputNormals(nrm)
    f.setIndices(bad)
    with pytest.raises(pcl_amd.PclHipError):
        f.compute()
