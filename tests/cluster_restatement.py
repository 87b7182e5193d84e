"""pcl::extractEuclideanClusters (segmentation/include/pcl/segmentation/impl/extract_clusters.hpp:124-217) and the ordering
of EuclideanClusterExtraction::extract (:244-250) written out in numpy: the breadth-first flood in the reference's order
over radiusSearch lists with the library's float32 d2 = (dx*dx + dy*dy) + dz*dz < float(r*r), r = double(float(tolerance)).
The lists come from a uniform grid of cells no smaller than r (every neighbour lies in the 27 cells around a point), so
50,000 points take seconds.  The reference leaves the order of clusters of equal size to an unstable std::sort; this
project's rule is applied instead: size descending, ties by ascending smallest index.  Deviation restated as well: a
non-finite record belongs to no cluster.  A record that `indices` names more than once is in its cluster once, as the
reference's processed[] has it."""
import numpy as np

UINT32_MAX = 2 ** 32 - 1


def bound(tolerance):
    """float(r * r) with r = double(float(tolerance)): kdtree_flann.hpp:398"""
    r = float(np.float32(tolerance))
    with np.errstate(over="ignore"):
        return np.float32(r * r)


def d2_f32(a, b):
    """float32 (dx*dx + dy*dy) + dz*dz, no contraction; a, b (m, 3) float32"""
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def neighbour_lists(pts, tolerance, chunk=1 << 22):
    """CSR (offsets, indices) of the radiusSearch lists of every point of pts (m, 3) float32 against pts, ascending
    (d2, index) as a sorted tree returns them."""
    m = len(pts)
    t = bound(tolerance)
    if m == 0 or not t > 0:
        return np.zeros(m + 1, np.int64), np.empty(0, np.int64)
    r = float(np.float32(tolerance))
    p64 = pts.astype(np.float64)
    lo = p64.min(axis=0)
    ext = float((p64.max(axis=0) - lo).max())
    cell = max(r * 1.001, ext / float(1 << 19), 1e-300)
    c = np.floor((p64 - lo) / cell).astype(np.int64) + 1  # 1 .. 2^19 + 1: the 27 cells around never leave the key range
    dim = np.int64((1 << 19) + 3)
    key = (c[:, 0] * dim + c[:, 1]) * dim + c[:, 2]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    qs, js, ds = [], [], []
    offs = [(dx * dim + dy) * dim + dz for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
    for off in offs:
        nk = key + off
        a = np.searchsorted(skey, nk, side="left")
        b = np.searchsorted(skey, nk, side="right")
        cnt = b - a
        nz = np.nonzero(cnt)[0]
        if len(nz) == 0:
            continue
        # candidates in chunks of bounded size
        csum = np.cumsum(cnt[nz])
        start = 0
        while start < len(nz):
            base = csum[start - 1] if start else 0
            end = int(np.searchsorted(csum, base + chunk, side="right"))
            end = max(end, start + 1)
            q = nz[start:end]
            n_q = cnt[q]
            tot = int(n_q.sum())
            qq = np.repeat(q, n_q)
            first = np.repeat(a[q], n_q)
            within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(n_q) - n_q, n_q)
            jj = order[first + within]
            d = d2_f32(pts[qq], pts[jj])
            hit = d < t
            qs.append(qq[hit])
            js.append(jj[hit])
            ds.append(d[hit])
            start = end
    if not qs:
        return np.zeros(m + 1, np.int64), np.empty(0, np.int64)
    q = np.concatenate(qs)
    j = np.concatenate(js)
    d = np.concatenate(ds)
    o = np.lexsort((j, d, q))
    q, j = q[o], j[o]
    offsets = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(q, minlength=m), out=offsets[1:])
    return offsets, j


def flood(m, offsets, nbr, sorted_results=True):
    """extract_clusters.hpp:149-194 over local ids 0..m-1 -> list of seed queues in the reference's order"""
    nn_start = 1 if sorted_results else 0
    processed = np.zeros(m, bool)
    off = offsets.tolist()
    nb = nbr.tolist()
    queues = []
    for index in range(m):
        if processed[index]:
            continue
        seed = [index]
        processed[index] = True
        sq = 0
        while sq < len(seed):
            a, b = off[seed[sq]], off[seed[sq] + 1]
            if b == a:  # !ret
                sq += 1
                continue
            for k in range(a + nn_start, b):
                jn = nb[k]
                if processed[jn]:
                    continue
                seed.append(jn)
                processed[jn] = True
            sq += 1
        queues.append(seed)
    return queues


def euclidean_clusters(cloud, tolerance, min_size=1, max_size=UINT32_MAX, indices=None, scale=None):
    """-> (clusters: list of ascending int32 arrays of original ids, labels (n,) int32, n_clustered)"""
    cloud = np.asarray(cloud, np.float32)[:, :3]
    n = len(cloud)
    ids = np.arange(n, dtype=np.int64) if indices is None else np.asarray(indices, np.int64).reshape(-1)
    # the flood marks records (processed[], :157-191): a record the list names again is in its cluster once and counts
    # once.  The first mention stands for it; the later ones find it processed.
    if len(ids):
        ids = ids[np.sort(np.unique(ids, return_index=True)[1])]
    p = cloud[ids]
    if scale is not None:
        p = p * np.asarray(scale, np.float32)[None, :]
    fin = np.isfinite(p).all(axis=1)
    ids, p = ids[fin], np.ascontiguousarray(p[fin])
    # Records at the same coordinates have the same list, and with ties listed in (d2, index) order the entry the flood
    # skips (nn_start_idx = 1) is always the lowest record of the query's own coordinates, which it has processed by then:
    # the flood over the distinct coordinates (in order of their first record), every coordinate standing for all of its
    # records, visits the same sets.  4,096 copies of a point cost one list, not 4,096 lists of 4,096.
    if len(p):
        uniq, first, inv = np.unique(p, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        by_first = np.argsort(first, kind="stable")
        uniq, pos_of = np.ascontiguousarray(uniq[by_first]), np.argsort(by_first)
        inv = pos_of[inv]
    else:
        uniq, inv = p, np.empty(0, np.int64)
    members_order = np.argsort(inv, kind="stable")
    members_off = np.zeros(len(uniq) + 1, np.int64)
    np.cumsum(np.bincount(inv, minlength=len(uniq)), out=members_off[1:])
    offsets, nbr = neighbour_lists(uniq, tolerance)
    clusters = []
    for useed in flood(len(uniq), offsets, nbr):
        if bound(tolerance) > 0:
            seed = np.concatenate([members_order[members_off[u]:members_off[u + 1]] for u in useed])
        else:  # no list holds anything, not even the query: every record is alone (:177-181)
            seed = None
        for s in ([seed] if seed is not None else [members_order[k:k + 1] for u in useed
                                                   for k in range(members_off[u], members_off[u + 1])]):
            if min_size <= len(s) <= max_size:  # :197
                clusters.append(np.sort(ids[s]).astype(np.int32))  # :206
    clusters.sort(key=lambda c: (-len(c), int(c[0])))  # :250 + the tie rule
    labels = np.full(n, -1, np.int32)
    for r, c in enumerate(clusters):
        labels[c] = r
    return clusters, labels, int(sum(len(c) for c in clusters))


def components_bruteforce(pts, tolerance):
    """connected components of d2 < t by all pairs (small clouds) -> list of ascending id arrays, ordered by the tie rule"""
    pts = np.asarray(pts, np.float32)[:, :3]
    m = len(pts)
    t = bound(tolerance)
    d = pts[:, None, :] - pts[None, :, :]
    adj = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < t
    lab = np.arange(m)
    while True:  # min-label propagation
        new = np.where(adj, lab[None, :], m).min(axis=1)
        new = np.minimum(new, lab)
        if np.array_equal(new, lab):
            break
        lab = new
    out = [np.nonzero(lab == v)[0].astype(np.int32) for v in np.unique(lab)]
    out.sort(key=lambda c: (-len(c), int(c[0])))
    return out


# ---- closed-form clouds shared by the CPU and the GPU tests -------------------------------------------------------------
JUST_ABOVE_ONE = float(np.nextafter(np.float32(1), np.float32(2)))


def line_cloud(n):
    """n collinear points at spacing 1: one cluster at any tolerance above 1"""
    c = np.zeros((n, 3), np.float32)
    c[:, 0] = np.arange(n, dtype=np.float32)
    return c


def integer_chain(n=20000, seed=5):
    """integer x, shuffled: d2 of neighbours is exactly 1"""
    c = line_cloud(n)
    return c[np.random.default_rng(seed).permutation(n)]


def two_rows(n=4096, gap_axis=1, seed=6):
    """integer x on two rows 1.5 apart along gap_axis, shuffled together -> (cloud, row of every record)"""
    c = np.zeros((2 * n, 3), np.float32)
    c[:n, 0] = np.arange(n, dtype=np.float32)
    c[n:, 0] = np.arange(n, dtype=np.float32)
    c[n:, gap_axis] = 1.5
    row = np.repeat(np.arange(2), n)
    p = np.random.default_rng(seed).permutation(2 * n)
    return c[p], row[p]


def contention_cloud(n=4096, seed=7):
    """n copies of the origin and n copies of (1, 0, 0), shuffled -> (cloud, which point)"""
    c = np.zeros((2 * n, 3), np.float32)
    c[n:, 0] = 1.0
    which = np.repeat(np.arange(2), n)
    p = np.random.default_rng(seed).permutation(2 * n)
    return c[p], which[p]


def blob_cloud(kmax=40, seed=8):
    """two blobs of k points at spacing 0.01 for every k = 1..kmax, centres 10 apart, shuffled -> (cloud, blob size of every
    record)"""
    pts, ks = [], []
    b = 0
    for k in range(1, kmax + 1):
        for _ in range(2):
            q = np.zeros((k, 3), np.float32)
            q[:, 0] = np.float32(10.0 * b)
            q[:, 1] = (np.arange(k) * 0.01).astype(np.float32)
            pts.append(q)
            ks.append(np.full(k, k))
            b += 1
    c, ks = np.concatenate(pts), np.concatenate(ks)
    p = np.random.default_rng(seed).permutation(len(c))
    return c[p], ks[p]


def random_volume(n=50000, seed=9):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def repeated_index_lists(n=397, seed=10):
    """index lists over n records that name records again -> (base without repeats, {name: list}): the base followed by
    its first ten entries, every entry twice in a row, and a shuffle of the base with every third entry once more"""
    base = np.arange(0, n, 2, dtype=np.int32)
    rng = np.random.default_rng(seed)
    mixed = np.concatenate([base, base[::3]])
    return base, {"head_again": np.concatenate([base, base[:10]]), "each_twice": np.repeat(base, 2),
                  "permuted": mixed[rng.permutation(len(mixed))].astype(np.int32)}


def pairs_cloud(k, lone=300, seed=11):
    """k pairs at x = 10 i and 10 i + 0.5 and `lone` single points (x = 10 (k + j), y = 5), shuffled -> (cloud, pair of
    every record or -1).  At tolerance 0.75 the components are the pairs and the lone points."""
    c = np.zeros((2 * k + lone, 3), np.float32)
    c[0:2 * k:2, 0] = 10.0 * np.arange(k)
    c[1:2 * k:2, 0] = 10.0 * np.arange(k) + 0.5
    c[2 * k:, 0] = 10.0 * (k + np.arange(lone))
    c[2 * k:, 1] = 5.0
    pair = np.concatenate([np.repeat(np.arange(k), 2), np.full(lone, -1)])
    assert 10.0 * (k + lone) < 2.0 ** 22  # every x is exact in float32
    p = np.random.default_rng(seed).permutation(len(c))
    return c[p], pair[p]


def striped_lattice(bands, width=1024, seed=12):
    """integer (x, y, 0): band b is the rows y = 4 b, 4 b + 1, 4 b + 2 (row 4 b + 3 is absent) over the columns
    0 .. width - 1 - 7 (b mod 5), shuffled -> (cloud, band of every record).  Rows of a band are 1 apart, bands 2 apart."""
    xs, ys = [], []
    for b in range(bands):
        w = width - 7 * (b % 5)
        for row in range(3):
            xs.append(np.arange(w, dtype=np.float32))
            ys.append(np.full(w, 4 * b + row, np.float32))
    c = np.zeros((sum(len(x) for x in xs), 3), np.float32)
    c[:, 0], c[:, 1] = np.concatenate(xs), np.concatenate(ys)
    c = c[np.random.default_rng(seed).permutation(len(c))]
    return c, (c[:, 1].astype(np.int64) // 4)


def lattice_bands_for(points, width=1024):
    """the smallest number of bands of striped_lattice(width=width) that holds at least `points` records"""
    per5 = 3 * sum(width - 7 * r for r in range(5))
    bands = 5 * (points // per5)
    have = (bands // 5) * per5
    while have < points:
        have += 3 * (width - 7 * (bands % 5))
        bands += 1
    return bands


def triple_cloud(n=5000, seed=13):
    """n copies of each of (0,0,0), (1,0,0), (2,0,0), shuffled -> (cloud, which point)"""
    c = np.zeros((3 * n, 3), np.float32)
    which = np.repeat(np.arange(3), n)
    c[:, 0] = which
    p = np.random.default_rng(seed).permutation(3 * n)
    return c[p], which[p]


def clusters_of_groups(group, min_size=1, max_size=UINT32_MAX):
    """the closed form: records with the same group >= 0 are one component (group < 0: a component of its own) ->
    (clusters, labels, n_clustered) as euclidean_clusters returns them, from sorting alone"""
    group = np.asarray(group, np.int64)
    n = len(group)
    g = group.copy()
    alone = np.nonzero(g < 0)[0]
    g[alone] = (g.max() + 1 if n else 0) + np.arange(len(alone))
    order = np.argsort(g, kind="stable")  # ascending ids inside every group
    starts = np.nonzero(np.r_[True, g[order][1:] != g[order][:-1]])[0] if n else np.empty(0, np.int64)
    ends = np.r_[starts[1:], n]
    size = ends - starts
    keep = (size >= min_size) & (size <= max_size)
    starts, ends, size = starts[keep], ends[keep], size[keep]
    first = order[starts]
    rank = np.lexsort((first, -size))
    clusters = [order[starts[r]:ends[r]].astype(np.int32) for r in rank]
    labels = np.full(n, -1, np.int32)
    for r, c in enumerate(clusters):
        labels[c] = r
    return clusters, labels, int(size.sum())
