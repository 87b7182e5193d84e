"""StatisticalOutlierRemoval / RadiusOutlierRemoval on the device against the reference's answers on bun0
(tests/golden/outlier_removal_bun0.json) and against the numpy restatement (tests/outlier_restatement.py): per-point
mean distances bit for bit, kept and removed lists identical, the statistics within 1e-12 relative (the device sums in a
fixed-order tree, the restatement sequentially)."""
import json
import os

import numpy as np
import pytest

import outlier_restatement as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "outlier_removal_bun0.json")) as f:
        return json.load(f)


def sor(gpu, cloud, mean_k, std_mul, negative=False, indices=None, extract=True):
    import pcl_amd
    f = pcl_amd.StatisticalOutlierRemoval(gpu, extract_removed_indices=extract)
    f.setInputCloud(cloud)
    f.setMeanK(mean_k)
    f.setStddevMulThresh(std_mul)
    f.setNegative(negative)
    if indices is not None:
        f.setIndices(indices)
    kept = f.filterIndices()
    return f, kept


def ror(gpu, cloud, radius, min_pts, negative=False, indices=None, is_dense=None):
    import pcl_amd
    f = pcl_amd.RadiusOutlierRemoval(gpu, extract_removed_indices=True)
    f.setInputCloud(cloud, is_dense)
    f.setRadiusSearch(radius)
    f.setMinNeighborsInRadius(min_pts)
    f.setNegative(negative)
    if indices is not None:
        f.setIndices(indices)
    return f, f.filterIndices()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def check_sor(f, kept, ref, label=""):
    """bit-exact distances, statistics to 1e-12, identical lists up to points inside that band of the threshold"""
    d = np.asarray(f.lastMeanDistances())
    assert np.array_equal(bits(d), bits(ref["dist"])), label + ": mean distances differ in %d entries" % int(
        (bits(d) != bits(ref["dist"])).sum())
    st = f.lastStatistics()
    assert st["valid"] == ref["valid"]
    for k in ("mean", "stddev", "threshold", "sum", "sq_sum"):
        a, b = st[k], ref[k]
        if np.isnan(b):
            assert np.isnan(a), k
        else:
            assert abs(a - b) <= REL * max(abs(b), 1e-300), (label, k, a, b)
    kept = np.asarray(kept)
    if not np.array_equal(kept, ref["kept"]):
        diff = np.setxor1d(kept, ref["kept"])
        thr = ref["threshold"]
        q = np.arange(len(d)) if f.getIndices() is None else None
        assert q is not None, label + ": kept sets differ on an indexed run"
        near = np.abs(d[diff].astype(np.float64) - thr) <= REL * abs(thr)
        assert near.all(), label + ": kept sets differ away from the threshold"
        print("%s: %d point(s) within 1e-12 of the threshold classified differently" % (label, len(diff)))
    else:
        assert np.array_equal(np.asarray(f.getRemovedIndices()), ref["removed"]), label


def test_bun0_goldens(gpu, bunny, gold):
    b = bunny["bun0"][:, :3].copy()
    g = gold["sor"]
    f, kept = sor(gpu, b, g["mean_k"], g["std_mul"])
    assert len(kept) == g["kept"] and len(f.getRemovedIndices()) == len(b) - g["kept"]
    np.testing.assert_allclose(b[kept[-1]], g["last_kept"], atol=1e-4)
    out = f.filter()
    assert out.shape == (g["kept"], 3)
    check_sor(f, kept, rs.statistical_outlier_removal(b, g["mean_k"], g["std_mul"]), "bun0")
    f, kept = sor(gpu, b, g["mean_k"], g["std_mul"], negative=True)
    assert len(kept) == g["negative_kept"] and len(f.getRemovedIndices()) == g["kept"]
    np.testing.assert_allclose(b[kept[-1]], g["negative_last_kept"], atol=1e-4)
    g = gold["ror"]
    f, kept = ror(gpu, b, g["radius"], g["min_pts"])
    assert len(kept) == g["kept"] and len(f.getRemovedIndices()) == len(b) - g["kept"]
    np.testing.assert_allclose(b[kept[-1]], g["last_kept"], atol=1e-4)
    f, kept = ror(gpu, b, g["radius"], g["min_pts"], negative=True)
    assert len(kept) == g["negative_kept"] and len(f.getRemovedIndices()) == g["kept"]


def noisy_cloud(n, seed=7, outliers=0.02, nans=0.01, dups=0.01):
    from pcl_amd import synth
    rng = np.random.default_rng(seed)
    c = synth.gaussian_surface(n)[:, :3].astype(np.float32).copy()
    lo, hi = c.min(0), c.max(0)
    m = len(c)
    o = rng.choice(m, int(m * outliers), replace=False)
    c[o] = rng.uniform(lo, hi, size=(len(o), 3)).astype(np.float32)
    d = rng.choice(m, int(m * dups), replace=False)
    c[d] = c[rng.choice(m, len(d))]
    z = rng.choice(m, int(m * nans), replace=False)
    c[z, rng.integers(0, 3, len(z))] = np.nan
    return c


@pytest.fixture(scope="module")
def cloud20():
    return noisy_cloud(1 << 20)


def test_sor_parity_2p20(gpu, cloud20):
    from oracle import pcl_oracle
    tree = pcl_oracle.KdTree(cloud20)
    for neg in (False, True):
        f, kept = sor(gpu, cloud20, 50, 1.0, negative=neg)
        check_sor(f, kept, rs.statistical_outlier_removal(cloud20, 50, 1.0, negative=neg, tree=tree), "2^20 neg=%s" % neg)


def test_ror_parity_2p20(gpu, cloud20):
    from oracle import pcl_oracle
    tree = pcl_oracle.KdTree(cloud20)
    for dense in (True, False):
        for neg in (False, True):
            f, kept = ror(gpu, cloud20, 0.004, 6, negative=neg, is_dense=dense)
            ref = rs.radius_outlier_removal(cloud20, 0.004, 6, negative=neg, dense=dense, tree=tree)
            assert np.array_equal(np.asarray(kept), ref["kept"]), (dense, neg)
            assert np.array_equal(np.asarray(f.getRemovedIndices()), ref["removed"]), (dense, neg)


def test_indices_subset(gpu, cloud20):
    rng = np.random.default_rng(3)
    nan_rows = np.flatnonzero(~np.isfinite(cloud20).all(1))[:50]
    idx = np.concatenate([rng.choice(len(cloud20), 20000, replace=False), nan_rows]).astype(np.int32)
    rng.shuffle(idx)
    idx = np.concatenate([idx, idx[:100]])  # repeated entries count twice, as in the reference's loop
    f, kept = sor(gpu, cloud20, 20, 0.5, indices=idx)
    ref = rs.statistical_outlier_removal(cloud20, 20, 0.5, indices=idx)
    assert np.array_equal(bits(f.lastMeanDistances()), bits(ref["dist"]))
    assert np.array_equal(np.asarray(kept), ref["kept"])
    assert np.array_equal(np.asarray(f.getRemovedIndices()), ref["removed"])
    for dense in (True, False):
        f, kept = ror(gpu, cloud20, 0.004, 6, indices=idx, is_dense=dense)
        ref = rs.radius_outlier_removal(cloud20, 0.004, 6, dense=dense, indices=idx)
        assert np.array_equal(np.asarray(kept), ref["kept"])
        assert np.array_equal(np.asarray(f.getRemovedIndices()), ref["removed"])
    with pytest.raises(Exception):
        sor(gpu, cloud20, 20, 0.5, indices=np.array([0, len(cloud20)], np.int32))


@pytest.mark.parametrize("mean_k", [1, 8, 31, 50, 64, 100])
def test_sor_mean_k_buckets(gpu, bunny, mean_k):
    b = bunny["bun0"][:, :3].copy()
    f, kept = sor(gpu, b, mean_k, 1.0)
    check_sor(f, kept, rs.statistical_outlier_removal(b, mean_k, 1.0), "mean_k=%d" % mean_k)


def _butterfly_then_waves(x):
    """x[..., 256]: per column the 64-lane xor butterfly (every lane adds its partner's value, offsets 32 .. 1; lane 0
    is read), then the four waves in order from 0.0"""
    x = x.reshape(x.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    a = np.zeros(x.shape[:-2], np.float64)
    for w in range(4):
        a = a + x[..., w, 0]
    return a


def sor_sums_in_kernel_order(d, valid):
    """(sum, sq_sum, valid) of the float32 distances d as sor_partial_kernel / sor_finalize_kernel add them
    (pcl_amd/csrc/block_sums.hpp; OR_BLOCK 256 threads, OR_PER 16 entries per thread, OR_CHUNK 4096 entries per block)."""
    m = len(d)
    nb = (m + 4095) // 4096
    cols = np.zeros((3, nb * 4096), np.float64)  # (entries past m are skipped by the kernel; x + 0.0 has the bits of x here:
    cols[0, :m] = d                              # no sum is -0.0)
    cols[1, :m] = d * d                          # the square in float, then widened
    cols[2, :m] = valid
    cols = cols.reshape(3, nb, 256, 16)
    acc = np.zeros((3, nb, 256), np.float64)
    for e in range(16):  # a thread's 16 entries in order
        acc = acc + cols[..., e]
    rows = _butterfly_then_waves(acc)  # [3, nb]: one row per block
    acc = np.zeros((3, 256), np.float64)
    for b in range(0, nb, 256):  # finalize: thread t adds the rows t, t + 256, ...
        part = rows[:, b:b + 256]
        acc[:, :part.shape[1]] = acc[:, :part.shape[1]] + part
    return _butterfly_then_waves(acc)


# the smallest sizes at which a level of the order can go wrong: several blocks and a ragged last thread (4 rows: the
# finalize stride does not wrap); 259 rows: the finalize stride wraps for the first three threads, the last row has one entry
@pytest.mark.parametrize("m", [3 * 4096 + 5, 257 * 4096 + 4097], ids=["blocks", "stride_wraps"])
def test_sor_sums_have_the_documented_order(gpu, m):
    """sum, sq_sum and valid are not just repeatable: they are the sums in the order block_sums.hpp documents, restated
    here from the returned distances, bit for bit -- and mean, stddev, threshold follow from them by the kernel's three
    expressions."""
    from pcl_amd import synth
    c = synth.gaussian_surface(m)[:, :3].copy()
    nan_rows = np.random.default_rng(5).choice(m, 37, replace=False)
    c[nan_rows, 1] = np.nan
    std_mul = 1.5
    f, _ = sor(gpu, c, 4, std_mul)
    d = np.asarray(f.lastMeanDistances())
    valid = np.isfinite(c).all(1)
    assert d.dtype == np.float32 and len(d) == m and not d[~valid].any() and np.isfinite(d).all()
    a, b, n = sor_sums_in_kernel_order(d, valid)
    assert n == m - 37
    mean = a / n
    sd = np.sqrt((b - a * a / n) / (n - 1.0))
    ref = dict(sum=a, sq_sum=b, valid=n, mean=mean, stddev=sd, threshold=mean + np.float64(std_mul) * sd)
    st = f.lastStatistics()
    for k, r in ref.items():
        got = np.float64(st[k])
        print("%s: device %r restated %r" % (k, float(got), float(r)))
        assert got.view(np.uint64) == np.float64(r).view(np.uint64), (k, float(got), float(r))


def test_edges(gpu):
    import pcl_amd
    nan = np.float32("nan")
    small = np.array([[0, 0, 0], [nan, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float32)
    for mk in (3, 4, 50):  # K = mean_k + 1 > finite points
        f, kept = sor(gpu, small, mk, 1.0)
        check_sor(f, kept, rs.statistical_outlier_removal(small, mk, 1.0), "small k=%d" % mk)
    one = np.array([[nan, 0, 0], [1, 2, 3]], np.float32)
    f, kept = sor(gpu, one, 5, 1.0)
    ref = rs.statistical_outlier_removal(one, 5, 1.0)
    check_sor(f, kept, ref, "one finite")
    assert list(kept) == [0, 1]  # NaN distance and NaN threshold: nothing is removed
    for cloud in (np.zeros((0, 3), np.float32), np.full((7, 3), nan, np.float32)):
        f, kept = sor(gpu, cloud, 5, 1.0)
        assert list(kept) == list(range(len(cloud))) and f.lastStatistics()["valid"] == 0
        f, kept = ror(gpu, cloud, 0.1, 1, is_dense=False)
        assert len(kept) == 0 and len(f.getRemovedIndices()) == len(cloud)
        f, kept = ror(gpu, cloud, 0.1, 1, negative=True, is_dense=True)
        assert list(kept) == list(range(len(cloud)))
    f = pcl_amd.StatisticalOutlierRemoval(gpu)
    f.setInputCloud(small)
    f.setMeanK(0)
    with pytest.raises(pcl_amd.PclHipError):
        f.filterIndices()
    f = pcl_amd.RadiusOutlierRemoval(gpu)
    f.setInputCloud(small)
    with pytest.raises(pcl_amd.PclHipError):
        f.filterIndices()  # radius 0


def test_ror_boundary_lattice(gpu):
    g = np.arange(8, dtype=np.float32) * np.float32(0.5)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    # interior points have 6 neighbours at d2 == 0.25 == r*r exactly
    f, kept = ror(gpu, lat, 0.5, 6, is_dense=True)
    ref = rs.radius_outlier_removal(lat, 0.5, 6, dense=True)
    assert np.array_equal(np.asarray(kept), ref["kept"]) and len(kept) == 6 ** 3
    f, kept = ror(gpu, lat, 0.5, 6, is_dense=False)
    assert len(kept) == 0
    f, kept = ror(gpu, lat, 0.5, 0, is_dense=False)
    assert len(kept) == len(lat)  # the point itself is within


def test_negative_keep_organized_pointnormal(gpu, bunny):
    import pcl_amd
    b = bunny["bun0"]
    rec = np.zeros((len(b), 12), np.float32)  # PointNormal: x y z 1 nx ny nz 0 curvature ...
    rec[:, :3] = b[:, :3]
    rec[:, 3] = 1.0
    rec[:, 4:7] = 0.5
    f = pcl_amd.StatisticalOutlierRemoval(gpu)
    f.setInputCloud(rec)
    f.setMeanK(50)
    f.setStddevMulThresh(1.0)
    out = f.filter()
    assert out.shape == (352, 12) and np.array_equal(out[:, 4:7], np.full((352, 3), 0.5, np.float32))
    f.setKeepOrganized(True)
    f.setUserFilterValue(-7.0)
    org = f.filter()
    rem = np.asarray(f.getRemovedIndices())
    assert org.shape == rec.shape and len(rem) == 45
    assert (org[rem, :3] == -7.0).all() and np.array_equal(org[rem, 3:], rec[rem, 3:])
    keep = np.setdiff1d(np.arange(len(rec)), rem)
    assert np.array_equal(org[keep], rec[keep])
    f.setNegative(True)
    f.setKeepOrganized(False)
    assert len(f.filter()) == 45
    r = pcl_amd.RadiusOutlierRemoval(gpu)
    r.setInputCloud(rec)
    r.setRadiusSearch(0.02)
    r.setMinNeighborsInRadius(14)
    assert len(r.filter()) == 307


def test_torch_device_buffers(gpu, cloud20):
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(cloud20).cuda()
    f, kept = sor(gpu, t, 50, 1.0)
    assert kept.is_cuda and f.lastMeanDistances().is_cuda
    fh, kh = sor(gpu, cloud20, 50, 1.0)
    assert np.array_equal(kept.cpu().numpy(), kh)
    assert np.array_equal(bits(f.lastMeanDistances().cpu().numpy()), bits(fh.lastMeanDistances()))
    assert np.array_equal(f.getRemovedIndices().cpu().numpy(), fh.getRemovedIndices())
    out = f.filter()
    assert out.is_cuda and out.shape == (len(kh), 3)
    r, rk = ror(gpu, t, 0.004, 6)
    rh, rkh = ror(gpu, cloud20, 0.004, 6)
    assert rk.is_cuda and np.array_equal(rk.cpu().numpy(), rkh)


def test_sor_10m_parity_and_repeatable(gpu):
    from pcl_amd import synth
    from oracle import pcl_oracle
    c = noisy_cloud(10_000_000, seed=11)
    tree = pcl_oracle.KdTree(c)
    f, kept = sor(gpu, c, 50, 1.0)
    check_sor(f, kept, rs.statistical_outlier_removal(c, 50, 1.0, tree=tree), "10M")
    d1, s1 = np.asarray(f.lastMeanDistances()).copy(), dict(f.lastStatistics())
    f2, kept2 = sor(gpu, c, 50, 1.0)
    assert np.array_equal(bits(f2.lastMeanDistances()), bits(d1)) and f2.lastStatistics() == s1
    assert np.array_equal(np.asarray(kept2), np.asarray(kept))
    r, rk = ror(gpu, c, 0.0015, 4)
    ref = rs.radius_outlier_removal(c, 0.0015, 4, tree=tree, dense=False)
    assert np.array_equal(np.asarray(rk), ref["kept"])
