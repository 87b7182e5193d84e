"""The numpy restatement of EuclideanClusterExtraction (tests/cluster_restatement.py) pinned on the reference's own data --
the 3,283 golden radiusSearch(0.02) lists of sac_plane_test.pcd -- on brute force for bun0, and on clouds whose clusters
are known in closed form.  CPU only."""
import os

import numpy as np

import cluster_restatement as cr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sizes(clusters):
    return [len(c) for c in clusters]


def components_of_lists(offsets, indices):
    """components of the graph of CSR neighbour lists, ordered by the tie rule"""
    m = len(offsets) - 1
    lab = np.arange(m)
    src = np.repeat(np.arange(m), np.diff(offsets))
    while True:
        new = lab.copy()
        np.minimum.at(new, src, lab[indices])
        if np.array_equal(new, lab):
            break
        lab = new
    out = [np.nonzero(lab == v)[0].astype(np.int32) for v in np.unique(lab)]
    out.sort(key=lambda c: (-len(c), int(c[0])))
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_restatement_on_the_golden_radius_lists():
    z = np.load(os.path.join(GOLD, "sac_plane_radius.npz"))
    off, idx = z["offsets"].astype(np.int64), z["indices"].astype(np.int64)
    m = len(off) - 1
    assert m == 3283 and float(z["radius"]) == 0.02
    src = np.repeat(np.arange(m), np.diff(off))
    pairs = set(zip(src.tolist(), idx.tolist()))
    assert all((j, i) in pairs for i, j in pairs), "the golden lists are symmetric"
    assert all((i, i) in pairs for i in range(m)), "every point lists itself"
    comp = components_of_lists(off, idx)
    assert sizes(comp) == [3217, 44, 21, 1]
    clusters, labels, nc = cr.euclidean_clusters(z["cloud"], 0.02)
    assert same(clusters, comp) and nc == m
    assert all((labels[c] == r).all() for r, c in enumerate(clusters))
    # the restatement's own lists are the golden ones, as sets
    o2, i2 = cr.neighbour_lists(np.ascontiguousarray(z["cloud"][:, :3], np.float32), 0.02)
    assert np.array_equal(o2, off)
    assert set(zip(np.repeat(np.arange(m), np.diff(o2)).tolist(), i2.tolist())) == pairs


def test_restatement_on_bun0_bruteforce():
    b = np.load(os.path.join(GOLD, "bunny.npz"))["bun0"][:, :3]
    clusters, labels, nc = cr.euclidean_clusters(b, 0.01)
    assert sizes(clusters) == [357, 23, 12, 3, 1, 1]
    assert same(clusters, cr.components_bruteforce(b, 0.01))
    assert clusters[4][0] < clusters[5][0], "the two singletons: the smaller index first"
    assert nc == len(b) and (labels >= 0).all()
    c4 = cr.euclidean_clusters(b, 0.004)[0]
    assert len(c4) == 364 and same(c4, cr.components_bruteforce(b, 0.004))


def test_restatement_on_closed_forms():
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 257):
        c, lab, nc = cr.euclidean_clusters(cr.line_cloud(n), 1.5)
        assert sizes(c) == [n] and np.array_equal(c[0], np.arange(n)) and nc == n
    chain = cr.integer_chain(2000)
    c, lab, nc = cr.euclidean_clusters(chain, 1.0)  # d2 = 1 = t: the bound is strict
    assert sizes(c) == [1] * 2000 and [int(x[0]) for x in c] == list(range(2000))
    c, lab, nc = cr.euclidean_clusters(chain, cr.JUST_ABOVE_ONE)
    assert sizes(c) == [2000]
    cloud, row = cr.two_rows(512)
    c, lab, nc = cr.euclidean_clusters(cloud, cr.JUST_ABOVE_ONE)
    assert sizes(c) == [512, 512] and c[0][0] < c[1][0] and c[0][0] == 0
    assert all(len(set(row[x].tolist())) == 1 for x in c)
    assert sizes(cr.euclidean_clusters(cloud, 1.6)[0]) == [1024]
    cloud, which = cr.contention_cloud(300)
    c, lab, nc = cr.euclidean_clusters(cloud, 0.5)
    assert sizes(c) == [300, 300] and all(len(set(which[x].tolist())) == 1 for x in c)
    assert sizes(cr.euclidean_clusters(cloud, 1.5)[0]) == [600]
    cloud, ks = cr.blob_cloud()
    c, lab, nc = cr.euclidean_clusters(cloud, 0.011, 5, 30)
    assert sizes(c) == sorted([k for k in range(5, 31) for _ in range(2)], reverse=True) and len(c) == 52
    assert np.array_equal(lab >= 0, (ks >= 5) & (ks <= 30)) and nc == int(((ks >= 5) & (ks <= 30)).sum())
    assert all(len(set(ks[x].tolist())) == 1 and ks[x[0]] == len(x) for x in c)
    assert cr.euclidean_clusters(cloud, 0.011, 6, 5)[0] == []
    # edges of the tolerance: no neighbour at all, not even the point itself
    for tol in (0.0, 1e-30):
        c, lab, nc = cr.euclidean_clusters(cr.line_cloud(5), tol)
        assert sizes(c) == [1] * 5 and np.array_equal(lab, np.arange(5))
    # non-finite records, an index subset, a flattening scale
    cloud = cr.line_cloud(10)
    cloud[3, 1] = np.nan
    c, lab, nc = cr.euclidean_clusters(cloud, 1.5)
    assert [x.tolist() for x in c] == [[4, 5, 6, 7, 8, 9], [0, 1, 2]] and lab[3] == -1 and nc == 9
    c, lab, nc = cr.euclidean_clusters(cr.line_cloud(10), 1.5, indices=np.arange(0, 10, 3))
    assert [x.tolist() for x in c] == [[0], [3], [6], [9]]
    cloud, row = cr.two_rows(64, gap_axis=2)
    assert sizes(cr.euclidean_clusters(cloud, cr.JUST_ABOVE_ONE)[0]) == [64, 64]
    assert sizes(cr.euclidean_clusters(cloud, cr.JUST_ABOVE_ONE, scale=(1, 1, 0))[0]) == [128]


def test_restatement_on_repeated_indices():
    """a record named more than once is in its cluster once: against brute force over the distinct records of bun0"""
    b = np.ascontiguousarray(np.load(os.path.join(GOLD, "bunny.npz"))["bun0"][:, :3], np.float32)
    base, lists = cr.repeated_index_lists(len(b))
    assert len(base) == 199 and len(lists["head_again"]) == 209 and len(lists["each_twice"]) == 398
    assert len(np.unique(lists["permuted"])) == 199 and len(lists["permuted"]) > 199
    assert not np.array_equal(lists["permuted"], np.sort(lists["permuted"]))
    brute = [base[c] for c in cr.components_bruteforce(b[base], 0.01)]
    assert sizes(brute)[:3] == [21, 18, 12]
    plain = cr.euclidean_clusters(b, 0.01, indices=base)
    assert same(plain[0], brute) and plain[2] == 199
    for name, ind in lists.items():
        c, lab, nc = cr.euclidean_clusters(b, 0.01, indices=ind)
        assert same(c, brute), name
        assert nc == 199 and np.array_equal(lab, plain[1]), name
        cat = np.concatenate(c)
        assert len(np.unique(cat)) == len(cat) == 199 and np.isin(cat, base).all(), name
        # the size range counts distinct records
        c, lab, nc = cr.euclidean_clusters(b, 0.01, 13, 20, indices=ind)
        assert sizes(c) == [s for s in sizes(brute) if 13 <= s <= 20] and same(c, [x for x in brute if 13 <= len(x) <= 20])


def test_closed_forms_of_the_regime_clouds():
    """the clouds of tests/test_gpu_cluster_regimes.py at small sizes: the closed form (clusters_of_groups over the group
    the coordinates give) is what the flood gives"""
    def agree(ref, got):
        assert same(ref[0], got[0]) and np.array_equal(ref[1], got[1]) and ref[2] == got[2]

    chain = cr.integer_chain(300)
    agree(cr.clusters_of_groups(np.full(300, -1)), cr.euclidean_clusters(chain, 0.5))
    assert np.array_equal(cr.clusters_of_groups(np.full(300, -1))[1], np.arange(300))
    for k in (1, 7, 40):
        cloud, pair = cr.pairs_cloud(k, lone=9)
        ref = cr.clusters_of_groups(pair, 2)
        agree(ref, cr.euclidean_clusters(cloud, 0.75, 2))
        assert sizes(ref[0]) == [2] * k and (ref[1][pair < 0] == -1).all() and ref[2] == 2 * k
        firsts = [int(c[0]) for c in ref[0]]
        assert firsts == sorted(firsts)
    bands = cr.lattice_bands_for(1500, width=40)
    cloud, band = cr.striped_lattice(bands, width=40)
    assert len(cloud) >= 1500 and len(cr.striped_lattice(bands - 1, width=40)[0]) < 1500 and bands > 10
    for tol in (cr.JUST_ABOVE_ONE, 2.0):
        ref = cr.clusters_of_groups(band)
        agree(ref, cr.euclidean_clusters(cloud, tol))
        assert len(set(sizes(ref[0]))) == 5 and len(ref[0]) == bands
    one = cr.euclidean_clusters(cloud, float(np.nextafter(np.float32(2), np.float32(3))))
    agree(cr.clusters_of_groups(np.zeros(len(cloud), np.int64)), one)
    assert sizes(one[0]) == [len(cloud)]
    cloud, which = cr.triple_cloud(40)
    agree(cr.clusters_of_groups(which), cr.euclidean_clusters(cloud, 0.5))
    agree(cr.clusters_of_groups(np.zeros(120, np.int64)), cr.euclidean_clusters(cloud, cr.JUST_ABOVE_ONE))
