"""RegionGrowing restated twice in numpy / plain Python, for tests/test_region_growing_restatement.py (CPU) and the
`-m gpu` modules tests/test_gpu_region_growing*.py.

  literal()    a transcription of pcl::RegionGrowing's loop (segmentation/include/pcl/segmentation/impl/region_growing.hpp
               :358-461: the curvature order, the seeding, growRegion with its queue, validatePoint in smooth mode without
               the residual test) plus assembleRegions and the size filter of extract (:258-271)
  two_phase()  the order-free formulation the kernels of pcl_amd/csrc/region_growing.hpp implement: phase 1 = the fixed
               point g(v) = min(own rank if expander, min over edges u->v out of expanders of g(u)); phase 2 = the
               lexicographically first selection among the leftover points; numbering by the seeds' ranks

Shared conventions (the library's deviations, include/pclhip.h): the k-NN lists are exact with ties to the lower index and
FLANN's float distance ((dx dx + dy dy) + dz dz); curvature ties go to the lower original index; a non-finite point is in
no segment; the dot of two normals is the float sum (x x' + y y') + z z'; c = cos(float32(theta)) in float32.
near_threshold() counts the |dot| values within 2 ulp of c: every test asserts that it is 0 before it compares anything,
so that nothing hangs on the last place of a cosine."""
from collections import deque

import numpy as np

DEFAULT_THETA = float(np.float32(30.0) / np.float32(180.0) * np.float32(np.pi))
DEFAULT_CURVATURE = 0.05
INF = 1 << 62


def selected(points, indices=None):
    """ascending original ids of the finite (and selected) records"""
    pts = np.asarray(points, np.float32)[:, :3]
    ok = np.isfinite(pts).all(axis=1)
    if indices is not None:
        pick = np.zeros(len(pts), bool)
        pick[np.asarray(indices, np.int64)] = True
        ok &= pick
    return np.flatnonzero(ok)


def knn_lists(points, k, sel=None):
    """(n, k) int32: row i = the k nearest of the selected points to point i (itself included), ascending by (float d2,
    index); -1 where there are fewer, and in the rows of records that are not selected"""
    pts = np.asarray(points, np.float32)[:, :3]
    n = len(pts)
    if sel is None:
        sel = selected(pts)
    out = np.full((n, k), -1, np.int32)
    if len(sel) == 0 or k == 0:
        return out
    p = pts[sel]
    kk = min(k, len(sel))
    for b in range(0, len(sel), 512):
        q = p[b:b + 512]
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz  # float32 throughout
        order = np.argsort(d2, axis=1, kind="stable")[:, :kk]  # ties: the lower position = the lower original id
        out[sel[b:b + 512], :kk] = sel[order]
    return out


def cos_threshold(theta):
    return np.cos(np.float32(theta), dtype=np.float32)


def dots(normals, lists):
    """(n, k) float32: |n_i . n_lists[i][j]| as the float sum (x x' + y y') + z z' (garbage where lists < 0)"""
    nr = np.asarray(normals, np.float32)
    a = nr[:, None, :3]
    b = nr[np.maximum(lists, 0), :3]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def near_threshold(normals, lists, theta):
    """how many |dot| values of listed pairs lie within 2 ulp of c"""
    c = cos_threshold(theta)
    d = dots(normals, lists)
    with np.errstate(invalid="ignore"):
        close = np.abs(d - c) <= 2 * np.spacing(np.abs(c))
    return int((close & (lists >= 0)).sum())


def clear_theta(points, normals, k, theta, indices=None, lists=None):
    """the first of theta * (1 + j / 1000), j = 0, 1, ..., that leaves no |dot| within 2 ulp of its cosine: how a test picks
    a threshold near the one it wants without hanging on the last place of a cosine (decided by the restatement alone)"""
    if lists is None:
        lists = knn_lists(points, k, selected(points, indices))
    for j in range(1000):
        t = float(theta) * (1.0 + j / 1000.0)
        if near_threshold(normals, lists, t) == 0:
            return t
    raise AssertionError("no clear threshold near %r" % theta)


def _prepare(points, normals, k, theta, indices, lists):
    pts = np.asarray(points, np.float32)
    sel = selected(pts, indices)
    if lists is None:
        lists = knn_lists(pts, k, sel)
    nr = np.asarray(normals, np.float32)
    assert not np.isnan(nr[sel, 3]).any(), "a NaN curvature has no place in the order"
    with np.errstate(invalid="ignore"):
        ok = ~(dots(nr, lists) < cos_threshold(theta)) & (lists >= 0)  # NaN < c is false: a NaN normal passes
    curv = nr[:, 3].astype(np.float32)
    order = sorted(sel.tolist(), key=lambda i: (curv[i], i))  # (-0.0 == 0.0: a tie)
    return sel, lists, ok, curv, order


def _assemble(n, raw, nseg, mn, mx):
    """assembleRegions + the size filter -> (list of int32 arrays, labels int32 [n], n_clustered)"""
    sizes = np.bincount(raw[raw >= 0], minlength=nseg)
    keep = (sizes >= mn) & (sizes <= mx)
    new = np.where(keep, np.cumsum(keep) - 1, -1)
    labels = np.where(raw >= 0, new[np.maximum(raw, 0)], -1).astype(np.int32)
    idx = np.argsort(labels, kind="stable")
    idx = idx[labels[idx] >= 0]
    counts = sizes[keep]
    clusters = [a.astype(np.int32) for a in np.split(idx, np.cumsum(counts)[:-1])] if len(counts) else []
    return clusters, labels, int(counts.sum())


def literal(points, normals, k=30, theta=DEFAULT_THETA, curvature=DEFAULT_CURVATURE, mn=1, mx=0xFFFFFFFF, indices=None,
            curvature_test=True, lists=None):
    n = len(points)
    if n == 0 or normals is None or len(normals) != n or k == 0:  # prepareForSegmentation: no segment
        return [], np.full(n, -1, np.int32), 0
    sel, lists, ok, curv, order = _prepare(points, normals, k, theta, indices, lists)
    thr = np.float32(curvature)
    is_seed = ~(curv > thr) if curvature_test else np.ones(n, bool)
    labels = [-1] * n
    ll, oo, ss = lists.tolist(), ok.tolist(), is_seed.tolist()
    nseg = 0
    for seed in order:  # applySmoothRegionGrowingAlgorithm: the next point in the order that has no label
        if labels[seed] != -1:
            continue
        queue = deque([seed])  # growRegion
        labels[seed] = nseg
        while queue:
            u = queue.popleft()
            lu, ou = ll[u], oo[u]
            for j in range(k):
                v = lu[j]
                if v < 0 or labels[v] != -1 or not ou[j]:
                    continue
                labels[v] = nseg
                if ss[v]:
                    queue.append(v)
        nseg += 1
    return _assemble(n, np.asarray(labels, np.int64), nseg, mn, mx)


def two_phase(points, normals, k=30, theta=DEFAULT_THETA, curvature=DEFAULT_CURVATURE, mn=1, mx=0xFFFFFFFF, indices=None,
              curvature_test=True, lists=None, stats=None):
    n = len(points)
    if n == 0 or normals is None or len(normals) != n or k == 0:
        return [], np.full(n, -1, np.int32), 0
    sel, lists, ok, curv, order = _prepare(points, normals, k, theta, indices, lists)
    m = len(order)
    rank = {i: r for r, i in enumerate(order)}
    thr = np.float32(curvature)
    exp = [bool(not (curv[i] > thr)) or not curvature_test for i in order]
    out = [[rank[v] for v, e in zip(lists[i].tolist(), ok[i].tolist()) if e and v != i] for i in order]
    # phase 1: any relaxation order reaches the fixed point
    g = [r if exp[r] else INF for r in range(m)]
    sweeps = 0
    changed = True
    while changed:
        changed = False
        sweeps += 1
        for u in range(m):
            if exp[u]:
                gu = g[u]
                for v in out[u]:
                    if gu < g[v]:
                        g[v] = gu
                        changed = True
    # phase 2: the leftover points in rank order
    inn = [[] for _ in range(m)]
    for u in range(m):
        for v in out[u]:
            inn[v].append(u)
    lab = list(g)
    chosen = [False] * m
    left = 0
    for t in range(m):
        if g[t] != INF:
            continue
        left += 1
        claim = [u for u in inn[t] if u < t and chosen[u]]
        if claim:
            lab[t] = min(claim)
        else:
            chosen[t] = True
            lab[t] = t
    seeds = [r for r in range(m) if lab[r] == r]
    number = {s: c for c, s in enumerate(seeds)}
    raw = np.full(n, -1, np.int64)
    raw[np.asarray(order, np.int64)] = [number[lab[r]] for r in range(m)]
    if stats is not None:
        stats.update(leftover=left, sweeps=sweeps, seeds=len(seeds))
    return _assemble(n, raw, len(seeds), mn, mx)


# ---- clouds -------------------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def records(nrm, curv):
    return np.ascontiguousarray(np.concatenate([np.asarray(nrm, np.float32), np.asarray(curv, np.float32)[:, None]], axis=1))


def random_case(seed):
    """one of the 600 small clouds of the CPU tier -> dict(points, normals, k, theta, curvature)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 121))
    k = int(rng.integers(2, 9))
    kind = seed % 6
    pts = rng.random((n, 3))
    if kind == 1:  # a density gradient: the k-NN relation is far from symmetric
        pts[:, 0] = pts[:, 0] ** 4
        pts[:, 1] *= 0.2
        pts[:, 2] *= 0.05
    pts = pts.astype(np.float32)
    dirs = unit(rng.normal(size=(3, 3)))  # a few directions plus noise: the smoothness test passes and fails
    nrm = unit(dirs[rng.integers(0, 3, n)] + rng.normal(scale=0.25, size=(n, 3)))
    curv = (rng.random(n) * 0.1).astype(np.float32)
    curvature = 0.05
    if kind == 2:  # curvatures quantised into ties
        curv = (rng.integers(0, 4, n) * 0.03).astype(np.float32)
    if kind == 3:  # every point a seed
        curvature = 1.0
    if kind == 4:  # no point a seed
        curvature = -1.0
    if kind == 5:  # a gradient and ties at once, most points above the threshold
        pts[:, 0] = (pts[:, 0].astype(np.float64) ** 3).astype(np.float32)
        curv = (rng.integers(0, 3, n) * 0.04).astype(np.float32)
    theta = float(rng.uniform(0.15, 0.9))
    return dict(points=pts, normals=records(nrm, curv), k=k, theta=theta, curvature=curvature)


def roof(side=12, tilt0=25.0, bend=10.0, seed=3):
    """two sheets meeting at a ridge along y: the normals tilt by +-(tilt0 + bend |x|) degrees about y, the ridge points
    (x = 0) have a vertical normal and a curvature above the default threshold -> (points, normals, which) with which = -1 on
    the ridge, 0 / 1 on the sheets"""
    rng = np.random.default_rng(seed)
    xs = np.arange(-side, side + 1) / float(side)
    ys = np.arange(0, side + 1) / float(side)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    x, y = X.ravel(), Y.ravel()
    a = np.deg2rad(tilt0 + bend * np.abs(x)) * np.sign(x)
    z = -np.abs(x) * np.tan(np.deg2rad(tilt0))
    pts = np.stack([x, y, z], axis=1).astype(np.float32)
    nrm = unit(np.stack([np.sin(a), np.zeros_like(a), np.cos(a)], axis=1))
    curv = (0.001 + 0.03 * rng.random(len(x))).astype(np.float32)
    ridge = x == 0
    curv[ridge] = 0.2
    which = np.where(ridge, -1, (x > 0).astype(np.int64))
    return pts, records(nrm, curv), which


def growing_line(n=200, ratio=1.05, lowest="dense", level=0.01):
    """n points on a line whose gaps grow geometrically (with k = 2 the list of point i is (i, i - 1): nearly every edge
    points to the dense end), equal normals; the curvatures ascend from the dense or from the sparse end around `level`"""
    x = np.cumsum(ratio ** np.arange(n)) - 1.0
    pts = np.stack([x, np.zeros(n), np.zeros(n)], axis=1).astype(np.float32)
    step = np.arange(n) if lowest == "dense" else np.arange(n)[::-1]
    curv = (level * (1.0 + step / (4.0 * n))).astype(np.float32)
    nrm = np.tile(np.asarray([[0.0, 0.0, 1.0]], np.float32), (n, 1))
    return pts, records(nrm, curv)


def wavy_sheet(n, seed=0):
    """n random points on z = 0.1 sin(12 x) cos(8 y) over a rectangle that grows with n (constant density: 4096 points per
    unit area, so that the normals of neighbours differ by up to tenths of a radian and their dots spread over hundreds of
    thousands of floats), analytic normals, curvatures quantised to eight values with a quarter of them above the default
    threshold"""
    rng = np.random.default_rng(seed)
    w = np.sqrt(n / 4096.0)
    x, y = rng.random(n) * w, rng.random(n) * w
    z = 0.1 * np.sin(12 * x) * np.cos(8 * y)
    dzdx = 1.2 * np.cos(12 * x) * np.cos(8 * y)
    dzdy = -0.8 * np.sin(12 * x) * np.sin(8 * y)
    nrm = unit(np.stack([-dzdx, -dzdy, np.ones(n)], axis=1))
    curv = (rng.integers(0, 8, n) * 0.0085).astype(np.float32)
    return np.stack([x, y, z], axis=1).astype(np.float32), records(nrm, curv)


def faceted_sheet(n, seed=0, cell=0.25):
    """the points of wavy_sheet with the normal constant on every cell x cell facet, one of twelve directions that are at
    least 0.3 rad apart: the dots take a handful of values, far from the cosine of any threshold between 0.05 and 0.25 --
    the cloud for sizes at which a continuum of dots would meet every float near the threshold"""
    pts, rec = wavy_sheet(n, seed)
    az = np.arange(6) * (np.pi / 3)
    dirs = unit(np.concatenate([np.stack([s * np.cos(az + s), s * np.sin(az + s), np.ones(6)], axis=1) for s in (0.45, 1.1)]))
    gram = np.abs(dirs.astype(np.float64) @ dirs.astype(np.float64).T) - 2 * np.eye(12)
    assert gram.max() < np.cos(0.3)
    ix, iy = np.floor(pts[:, 0] / cell).astype(np.int64), np.floor(pts[:, 1] / cell).astype(np.int64)
    facet = (ix * 7 + iy * 13 + (ix * iy) % 5) % 12
    return pts, records(dirs[facet], rec[:, 3]), facet
