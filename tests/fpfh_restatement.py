"""numpy restatement of pcl::FPFHEstimation with setRadiusSearch: pcl::computePairFeatures (features/src/pfh.cpp:45-103),
computePointSPFHSignature and weightPointSPFHSignature (features/include/pcl/features/impl/fpfh.hpp:63-178), float32 in
the reference's operation order, neighbours in ascending d2 with ties broken by index (search::KdTree sorts).

Dot products and norms are ((x*x) + (y*y)) + (z*z), the cross product a1*b2 - a2*b1 per component, every operation
rounded to float32 (numpy evaluates one ufunc at a time: nothing is fused).  pcl_amd/csrc/fpfh.hpp uses the same order.

Besides the float32 result, restate() returns
  counts    the integer bin counts of every point (the SPFH value of a bin is hist_incr added `count` times in float32,
            which does not depend on the order of the neighbours)
  unstable  per point, the number of its pairs that a different acos / atan2 / rounding may bin differently.  A pair is
            unstable when, in a float64 evaluation of the same float32 inputs,
              - one of its three bin coordinates lies within EDGE_EPS of an integer, or
              - | |angle1| - |angle2| | lies within TIE_EPS of 0 without being 0 (the roles of the two points may swap), or
              - the pair is degenerate (distance 0 or d parallel to u: all features 0) in one precision and not in the
                other, or |d x u| <= DEGENERATE_EPS * |d| in float64.
            EDGE_EPS = 1e-5 and TIE_EPS = 1e-6: with them float32 and float64 binning agree on every pair of bun0 outside
            the unstable set at r = 0.01, 0.02 and 1.0 (tests/test_fpfh_restatement.py asserts it for 0.02 and 1.0).
  fpfh64    the FPFH in float64: the exact (math.fsum) sum of double(spfh) * double(1.0f / d2), normalised to 100 per
            histogram, not rounded
Deviation restated as pclhip_fpfh documents it: a point whose own normal is not finite gets NaN rows; a neighbour whose
normal is not finite is skipped in both passes but counts towards hist_incr.  Non-finite points are no one's neighbours
and get NaN rows.

A radius whose float32 square is 0 finds no neighbour at all, not even the point itself (d2 < 0 never holds): the SPFH
row stays at zero (fpfh.hpp:224-225) and weightPointSPFHSignature divides by the sum of no weights: the FPFH row is NaN
(fpfh.hpp:255-261).  restate() and weigh() give both."""
import math
import os

import numpy as np

EDGE_EPS = 1e-5
TIE_EPS = 1e-6
DEGENERATE_EPS = 1e-6
BINS = 11
F32 = np.float32
D_PI = F32(1.0) / (F32(2.0) * F32(math.pi))  # fpfh.h:98

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bun0():
    """(points [397,3], normals [397,3]) float32 of tests/golden/pcd/bun0.pcd (ascii, x y z normal_x normal_y normal_z curvature)."""
    a = np.loadtxt(os.path.join(ROOT, "tests", "golden", "pcd", "bun0.pcd"), skiprows=11, dtype=np.float32)
    assert a.shape == (397, 7)
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3:6])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(p1, n1, p2, n2, dtype=np.float32):
    """computePairFeatures of point (p1, n1) against the k points (p2, n2), every operation in `dtype`.
    -> f1, f2, f3 [k], angle1, angle2 [k], degenerate [k] (bool), vnorm / f4 [k]"""
    p1, n1, p2, n2 = (np.asarray(v, dtype) for v in (p1, n1, p2, n2))
    k = p2.shape[0]
    with np.errstate(all="ignore"):
        d = p2 - p1[None, :]
        f4 = np.sqrt(_dot(d, d))
        n1b = np.broadcast_to(n1, (k, 3))
        angle1 = _dot(n1b, d) / f4
        angle2 = _dot(n2, d) / f4
        swap = np.arccos(np.abs(angle1)) > np.arccos(np.abs(angle2))
        u = np.where(swap[:, None], n2, n1b)
        t = np.where(swap[:, None], n1b, n2)
        d = np.where(swap[:, None], -d, d)
        f3 = np.where(swap, -angle2, angle1)
        v = _cross(d, u)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = _cross(u, v)
        f2 = _dot(v, t)
        f1 = np.arctan2(_dot(w, t), _dot(u, t))
        deg = (f4 == 0) | (vn == 0)
        zero = np.zeros(k, dtype)
        rel = np.where(f4 == 0, zero, vn / f4)
    return (np.where(deg, zero, f1), np.where(deg, zero, f2), np.where(deg, zero, f3), angle1, angle2, deg, rel)


def bin_coords(f1, f2, f3):
    """the three bin coordinates in double from the features (fpfh.hpp:91-103): the bin is floor(), clamped to 0..10"""
    f1, f2, f3 = (np.asarray(v).astype(np.float64) for v in (f1, f2, f3))
    return np.stack([BINS * ((f1 + math.pi) * float(D_PI)), BINS * ((f2 + 1.0) * 0.5), BINS * ((f3 + 1.0) * 0.5)], axis=-1)


def bins_of(coords):
    with np.errstate(invalid="ignore"):
        b = np.floor(coords)
    b = np.where(np.isnan(b), 0.0, b)
    return np.clip(b, 0, BINS - 1).astype(np.int64)


def neighbourhoods(points, radius):
    """per finite point: (indices, d2) of every finite point with float32 d2 < float32(r * r), ascending (d2, index)"""
    pts = np.asarray(points, np.float32)
    fin = np.isfinite(pts).all(axis=1)
    ids = np.nonzero(fin)[0]
    p = pts[ids]
    t = F32(float(radius) * float(radius))
    out = {}
    for a, i in enumerate(ids):
        dx, dy, dz = p[a, 0] - p[:, 0], p[a, 1] - p[:, 1], p[a, 2] - p[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        sel = np.nonzero(d2 < t)[0]
        order = np.lexsort((ids[sel], d2[sel]))
        out[int(i)] = (ids[sel][order], d2[sel][order])
    return out


def spfh_values(counts, m):
    """counts [33] of a point with m neighbours (itself included) -> the float32 SPFH row: hist_incr added count times"""
    with np.errstate(divide="ignore"):
        incr = F32(100.0) / F32(m - 1)
    cmax = int(counts.max())
    tab = np.zeros(cmax + 1, np.float32)
    if cmax > 0:
        tab[1:] = np.cumsum(np.full(cmax, incr, np.float32), dtype=np.float32)  # sequential float32 additions
    return tab[counts]


def weight_float32(spfh, nb, d2):
    """weightPointSPFHSignature in the reference's order and precisions -> [33] float32"""
    keep = d2 != 0
    keep &= ~np.isnan(spfh[nb, 0])
    w = (F32(1.0) / d2[keep]).astype(np.float32)
    vals = (spfh[nb[keep]] * w[:, None]).astype(np.float32)
    out = np.zeros(3 * BINS, np.float32)
    if vals.shape[0] == 0:
        return out
    hist = np.cumsum(vals, axis=0, dtype=np.float32)[-1]
    for h in range(3):
        s = np.cumsum(vals[:, h * BINS:(h + 1) * BINS].astype(np.float64).ravel())[-1]
        f = 100.0 / s if s != 0 else 0.0
        out[h * BINS:(h + 1) * BINS] = (hist[h * BINS:(h + 1) * BINS].astype(np.float64) * f).astype(np.float32)
    return out


def weight_float64(spfh, nb, d2):
    """the exact weighted sum with the reference's float32 weights, normalised to 100 per histogram -> [33] float64"""
    keep = d2 != 0
    keep &= ~np.isnan(spfh[nb, 0])
    w = (F32(1.0) / d2[keep]).astype(np.float64)
    prod = spfh[nb[keep]].astype(np.float64) * w[:, None]  # exact: 24 x 24 bits
    acc = np.array([math.fsum(prod[:, b]) for b in range(3 * BINS)])
    out = np.zeros(3 * BINS)
    for h in range(3):
        s = math.fsum(acc[h * BINS:(h + 1) * BINS])
        if s != 0:
            out[h * BINS:(h + 1) * BINS] = acc[h * BINS:(h + 1) * BINS] * (100.0 / s)
    return out


def weigh(spfh, points, radius, hoods=None):
    """both weightings of given SPFH rows (one per record of `points`) -> fpfh32 [n,33], fpfh64 [n,33], m [n]"""
    pts = np.asarray(points, np.float32)
    hoods = hoods if hoods is not None else neighbourhoods(pts, radius)
    n = pts.shape[0]
    f32 = np.full((n, 3 * BINS), np.nan, np.float32)
    f64 = np.full((n, 3 * BINS), np.nan)
    m = np.zeros(n, np.int64)
    for i, (nb, d2) in hoods.items():
        m[i] = len(nb)
        if np.isnan(spfh[i, 0]) or len(nb) == 0:  # no neighbour, not even itself (float32(r * r) == 0): NaN
            continue
        f32[i] = weight_float32(spfh, nb, d2)
        f64[i] = weight_float64(spfh, nb, d2)
    return f32, f64, m


def neighbourhoods_of(points, radius, rows):
    """neighbourhoods() of the finite records `rows` alone, each by one pass over the cloud"""
    pts = np.asarray(points, np.float32)
    ids = np.nonzero(np.isfinite(pts).all(axis=1))[0]
    p = pts[ids]
    t = F32(float(radius) * float(radius))
    out = {}
    for i in rows:
        dx, dy, dz = pts[i, 0] - p[:, 0], pts[i, 1] - p[:, 1], pts[i, 2] - p[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        sel = np.nonzero(d2 < t)[0]
        order = np.lexsort((ids[sel], d2[sel]))
        out[int(i)] = (ids[sel][order], d2[sel][order])
    return out


def restate(points, normals, radius, hoods=None):
    """hoods (optional): the neighbourhoods of the points to restate (neighbourhoods_of).  The SPFH part of the result is
    then that of these points alone, and fpfh32 / fpfh64 mean nothing (they weigh rows that were not restated)."""
    pts = np.asarray(points, np.float32)
    nrm = np.asarray(normals, np.float32)[:, :3]
    n = pts.shape[0]
    hoods = hoods if hoods is not None else neighbourhoods(pts, radius)
    nfin = np.isfinite(nrm).all(axis=1)
    counts = np.zeros((n, 3 * BINS), np.int64)
    counts64 = np.zeros((n, 3 * BINS), np.int64)
    unstable = np.zeros(n, np.int64)
    disagree = np.zeros(n, np.int64)  # pairs outside the unstable set that float32 and float64 bin differently
    pairs = 0
    spfh = np.full((n, 3 * BINS), np.nan, np.float32)
    for i, (nb, _d2) in hoods.items():
        if not nfin[i]:
            continue
        others = nb[(nb != i) & nfin[nb]]
        if len(others):
            f1, f2, f3, _a1, _a2, deg32, _r = pair_features(pts[i], nrm[i], pts[others], nrm[others], np.float32)
            g1, g2, g3, a1, a2, deg64, rel = pair_features(pts[i], nrm[i], pts[others], nrm[others], np.float64)
            b32 = bins_of(bin_coords(f1, f2, f3))
            c64 = bin_coords(g1, g2, g3)
            b64 = bins_of(c64)
            with np.errstate(invalid="ignore"):
                edge = (np.abs(c64 - np.round(c64)) < EDGE_EPS).any(axis=1)
                tie = np.abs(np.abs(a1) - np.abs(a2))
                tie = (tie < TIE_EPS) & (tie != 0)
                degen = (deg32 != deg64) | (~deg64 & (rel <= DEGENERATE_EPS))
            u = edge | tie | degen
            unstable[i] = int(u.sum())
            disagree[i] = int(((b32 != b64).any(axis=1) & ~u).sum())
            pairs += len(others)
            for h in range(3):
                counts[i, h * BINS:(h + 1) * BINS] = np.bincount(b32[:, h], minlength=BINS)
                counts64[i, h * BINS:(h + 1) * BINS] = np.bincount(b64[:, h], minlength=BINS)
        spfh[i] = spfh_values(counts[i], len(nb)) if len(nb) else 0.0  # (no neighbour at all: nothing was added)
    fpfh32, fpfh64, m = weigh(spfh, pts, radius, hoods)
    return dict(spfh=spfh, counts=counts, counts64=counts64, unstable=unstable, disagree=disagree, pairs=pairs,
                fpfh32=fpfh32, fpfh64=fpfh64, m=m, hoods=hoods)


def counts_from_rows(rows, m):
    """the integer counts behind device SPFH rows: the c with (hist_incr added c times) == value, bit for bit; -1 where no
    count gives the value"""
    rows = np.asarray(rows, np.float32)
    out = np.full(rows.shape, -1, np.int64)
    for i in range(rows.shape[0]):
        if np.isnan(rows[i, 0]):
            continue
        k = max(int(m[i]) - 1, 0)  # (m == 0: float32(r * r) == 0, not even the point itself)
        tab = spfh_values(np.arange(k + 1), int(m[i])) if k > 0 else np.zeros(1, np.float32)
        for b in range(rows.shape[1]):
            hit = np.nonzero(tab == rows[i, b])[0]
            if len(hit):
                out[i, b] = hit[0]
    return out
