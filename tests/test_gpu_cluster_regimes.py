"""EuclideanClusterExtraction off the easy path (the conventions of tests/test_gpu_cluster.py: lists, labels and counts
exactly equal to the reference, every case twice, the two runs the same bytes): cluster and record counts at the 8- and
16-bit key boundaries of the radix sorts, one lattice large enough that every block of the hook kernel takes a second query
group and one component is contended from every CU, and more coincident copies of a point than a leaf holds.

Where the clusters are known in closed form the reference is cluster_restatement.clusters_of_groups over the group the
coordinates give (no flood); tests/test_cluster_restatement.py verifies that closed form against the flood at small sizes.

Not here: index lists that name a record more than once.  The library still counts such a record once per copy (DESIGN.md
row f-10, known deviation); tests/test_cluster_restatement.py pins what the result has to be."""
import numpy as np
import pytest

import cluster_restatement as cr
from test_gpu_cluster import check, extractor

pytestmark = pytest.mark.gpu
JUST_ABOVE_TWO = float(np.nextafter(np.float32(2), np.float32(3)))


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


def check_csr(gpu, cloud, tol, offsets, indices, labels, mn=1, mx=0xFFFFFFFF):
    """two runs, byte-identical; offsets, indices and labels equal to the given ones (no per-cluster python lists)"""
    e = extractor(gpu, cloud, tol, mn, mx)
    off, idx, lab = e.extractCSR()
    off2, idx2, lab2 = e.extractCSR()
    assert off.tobytes() == off2.tobytes() and idx.tobytes() == idx2.tobytes() and lab.tobytes() == lab2.tobytes()
    assert off.dtype == np.uint64 and idx.dtype == np.int32 and lab.dtype == np.int32
    assert np.array_equal(off.astype(np.int64), np.asarray(offsets, np.int64))
    assert np.array_equal(idx, indices) and np.array_equal(lab, labels)
    return off, idx, lab


# ---- 2., 3. the sorts' key widths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537])
def test_singletons_at_key_boundaries(gpu, n):
    """n clusters of one record: the dense ids, the ranks and the keys of the last sort all reach n - 1 (and n for no
    record here); offsets, indices and labels are 0, 1, 2, ..."""
    chain = cr.integer_chain(n)
    check_csr(gpu, chain, 0.5, np.arange(n + 1), np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32))


@pytest.mark.parametrize("k", [255, 256, 257, 65535, 65536, 65537])
def test_pairs_and_rejected_records_at_key_boundaries(gpu, k):
    """k clusters of two and 300 records below min_size: the key of an unlabelled record in the last sort is k"""
    cloud, pair = cr.pairs_cloud(k)
    rc, rl, rn = cr.clusters_of_groups(pair, 2)
    assert len(rc) == k and rn == 2 * k and (rl[pair < 0] == -1).all() and (rl[pair >= 0] >= 0).all()
    firsts = np.array([c[0] for c in rc])
    assert (np.diff(firsts) > 0).all()  # all of one size: ordered by smallest original index
    if k <= 257:
        check(gpu, cloud, 0.75, 2, ref=(rc, rl, rn))
    else:
        check_csr(gpu, cloud, 0.75, 2 * np.arange(k + 1), np.concatenate(rc), rl, mn=2)


# ---- 4. every block takes a second query group -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    """A 256-thread block serves 256 points per query group, and a CU holds at most 8 blocks of 256 threads (2,048 lanes
    per CU), so whatever occupancy the runtime reports for the hook kernel, 8 * 256 * CUs points fill every block the
    launch can have; 1,024 more give a second group to some of them.  Not larger than that."""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    points = 8 * 256 * cus + 1024
    bands = cr.lattice_bands_for(points)
    cloud, band = cr.striped_lattice(bands)
    assert points <= len(cloud) < points + 3 * 1024
    print("fullgrid lattice: %d CUs -> %d points in %d bands" % (cus, len(cloud), bands))
    return cloud, band, bands


@pytest.mark.parametrize("tol", [cr.JUST_ABOVE_ONE, 2.0])
def test_fullgrid_lattice_bands(gpu, lattice, tol):
    """rows of a band are 1 apart, bands 2 apart (d2 = 4 is not < 4): the components are the bands, five sizes, ties by
    smallest original index"""
    cloud, band, bands = lattice
    ref = cr.clusters_of_groups(band)
    clusters, _ = check(gpu, cloud, tol, ref=ref)
    assert len(clusters) == bands and len(set(len(c) for c in clusters)) == 5


def test_fullgrid_lattice_one_component(gpu, lattice):
    """just above 2 the bands join: one tree, hooked from every CU"""
    cloud, band, bands = lattice
    n = len(cloud)
    check_csr(gpu, cloud, JUST_ABOVE_TWO, [0, n], np.arange(n, dtype=np.int32), np.zeros(n, np.int32))


# ---- 5. coincidence beyond a leaf -------------------------------------------------------------------------------------------
def test_three_points_5000_copies_each(gpu):
    cloud, which = cr.triple_cloud(5000)
    clusters, lab = check(gpu, cloud, 0.5, ref=cr.clusters_of_groups(which))
    assert [len(c) for c in clusters] == [5000] * 3 and clusters[0][0] == 0 and clusters[0][0] < clusters[1][0] < clusters[2][0]
    clusters, _ = check(gpu, cloud, cr.JUST_ABOVE_ONE, ref=cr.clusters_of_groups(np.zeros(len(cloud), np.int64)))
    assert [len(c) for c in clusters] == [15000]
