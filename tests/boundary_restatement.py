"""A numpy restatement of pcl::BoundaryEstimation (features/include/pcl/features/impl/boundary.hpp:87-137 isBoundaryPoint,
:141-209 computeFeature; boundary.h:161-168 getCoordinateSystemOnPlane), the yardstick of tests/test_gpu_boundary*.py.  Not
product code.

  neighbourhood   every finite point with float32 d2 < float32(r * r), the point itself included -- by brute force
                  (iss_restatement.hits) -- or lists handed in (k mode: the device's own pclhip_knn lists); fewer than
                  max(3, min_neighbors) entries: flag 0
  basis           v = (nx, ny, nz, 0).unitOrthogonal() by Eigen's rule for 4-vectors: maxi the first index of the largest
                  |component|, sndi = 1 if maxi == 0 else 0, inv = 1 / sqrt(n[sndi]^2 + n[maxi]^2), v[maxi] = -n[sndi] * inv,
                  v[sndi] = n[maxi] * inv, the rest 0; u = n x v; all in float32
  angles          delta = p - q in float32, an all-zero delta is skipped; atan2(v . delta, u . delta), the dots as
                  ((a0 b0) + (a1 b1)) + (a2 b2) in float32; no angle: flag 0
  largest gap     the angles sorted; consecutive float32 differences and the wrap-around (2 * float32(pi) - last) + first
  flag            max gap > float32(threshold)
  invalid         a non-finite record, a non-finite or zero normal, no neighbour at all: flag 0, counted (include/pclhip.h)

Two formulations.  The float32 path above follows the reference operation by operation.  The float64 path takes the same
float32 deltas and the same float32 basis and evaluates dots, atan2 and the differences in float64 (2 * float32(pi) widened):
the reference's formula without its rounding.

The unstable band.  A gap g between the angles a and b is an UNSTABLE comparison when |g - thr| <= E,
    E = 2^-24 * (c * (kappa_a + kappa_b) + c0),   kappa = |delta| / hypot(u . delta, v . delta),   c = 10, c0 = 32.
Units of 2^-24 (one float32 rounding of a value near 1):
  * a three-term float32 dot rounds three products and two sums: |dx|, |dy| <= 3 * sum |a_i delta_i| <= 3 |delta| (|a| = 1),
    and atan2 turns a displacement (dx, dy) of (x, y) into at most hypot(dx, dy) / hypot(x, y) <= 3 sqrt(2) kappa of angle
  * the basis' own rounding: inv takes a square root, a division and a product, the cross product two products and a
    difference per component -- u and v are each within 4 of unit orthogonal vectors, which moves (x, y) by at most
    4 |delta| each: another 4 sqrt(2) kappa per angle.  c = 7 sqrt(2) = 9.9 -> 10
  * atan2f is good to 2 ulp; an ulp at 2 <= |angle| <= pi is 4: 8 per angle, 16 per gap
  * the final subtraction: half an ulp of a gap below 8 is 4; the wrap-around first forms 2 pi - last < 16: another 8.
    c0 = 16 + 12 = 28 -> 32
Only points that own such a gap may get different flags from two correct implementations.  restate() reports them (`own`),
and the largest |g32 - g64| / E over all gaps (`ratio`): the float32 path held against the float64 path, never against a
device."""
import os

import numpy as np

import iss_restatement as ir

ROOT = ir.ROOT
F32 = np.float32
U24 = 2.0 ** -24
C_KAPPA = 10.0
C_ZERO = 32.0
PI_F = F32(np.pi)
TWO_PI_F = F32(2.0) * PI_F
BUN0_RESOLUTION = ir.BUN0_RESOLUTION


def load_bun0():
    """points [397, 3], normals [397, 3] float32 of tests/golden/pcd/bun0.pcd"""
    a = np.loadtxt(os.path.join(ROOT, "tests", "golden", "pcd", "bun0.pcd"), skiprows=11, dtype=np.float32)
    assert a.shape == (397, 7)
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3:6])


def global_normal(points):
    """the normal NormalEstimation gives every point when k = n (the reference's test): the eigenvector of the smallest
    eigenvalue of the cloud's covariance, float32, its largest component positive (the flags do not depend on the sign)"""
    p = np.asarray(points, np.float64)
    c = np.cov((p - p.mean(axis=0)).T)
    w, v = np.linalg.eigh(c)
    nrm = v[:, 0]
    nrm = nrm * np.sign(nrm[np.argmax(np.abs(nrm))])
    return nrm.astype(F32)


def basis(normal):
    """-> u, v float32 [3] of one float32 normal (getCoordinateSystemOnPlane)"""
    n = np.asarray(normal, F32)
    n4 = np.array([n[0], n[1], n[2], 0], F32)
    maxi = int(np.argmax(np.abs(n4)))  # the first index of the largest
    sndi = 1 if maxi == 0 else 0
    inv = F32(1) / np.sqrt(n4[sndi] * n4[sndi] + n4[maxi] * n4[maxi], dtype=F32)
    v = np.zeros(4, F32)
    v[maxi] = -n4[sndi] * inv
    v[sndi] = n4[maxi] * inv
    u = np.array([n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0]], F32)
    return u, v[:3].copy()


def gaps_of(q, nbrs, u, v):
    """the gaps around q of the neighbours nbrs [m, 3] -> None without an angle, else dict: g32, g64 [a] (the sorted order
    of the float32 angles, the wrap-around last), E [a], kappa [a] (of the angle each gap starts at)"""
    d = (np.asarray(nbrs, F32) - np.asarray(q, F32)[None, :]).astype(F32)
    d = d[(d != 0).any(axis=1)]
    if len(d) == 0:
        return None
    x32 = (u[0] * d[:, 0] + u[1] * d[:, 1]) + u[2] * d[:, 2]
    y32 = (v[0] * d[:, 0] + v[1] * d[:, 1]) + v[2] * d[:, 2]
    assert x32.dtype == F32 and y32.dtype == F32
    a32 = np.arctan2(y32, x32)
    assert a32.dtype == F32
    d64, u64, v64 = d.astype(np.float64), u.astype(np.float64), v.astype(np.float64)
    x64, y64 = d64 @ u64, d64 @ v64
    a64 = np.arctan2(y64, x64)
    with np.errstate(divide="ignore"):
        kappa = np.sqrt((d64 * d64).sum(axis=1)) / np.hypot(x64, y64)
    o = np.argsort(a32, kind="stable")
    a32, a64, kappa = a32[o], a64[o], kappa[o]
    g32 = np.append(np.diff(a32), (TWO_PI_F - a32[-1]) + a32[0]).astype(F32)
    g64 = np.append(np.diff(a64), (float(TWO_PI_F) - a64[-1]) + a64[0])
    E = U24 * (C_KAPPA * (kappa + np.roll(kappa, -1)) + C_ZERO)
    return dict(g32=g32, g64=g64, E=E, kappa=kappa)


def restate(points, normals, threshold=np.pi / 2, radius=None, lists=None, rows=None, min_neighbors=3, skip=None):
    """points [n, 3], normals [n, 3] (or one [3] for all).  Queries: `rows` (default every record), neighbourhoods by
    `radius` or `lists` (one sequence of record ids per query; ids < 0 and non-finite records are no entries).  `skip`
    [n] bool: records that are never neighbours.
    -> dict over the queries: flag uint8, invalid bool, own bool (an unstable comparison), m (entries), max32, max64 (largest
    gap, NaN without one), closest (smallest |g32 - thr|), and scalars: ratio (largest |g32 - g64| / E), spread (largest
    |g32 - g64|), kappa (largest), flips (queries whose float64 flag differs)"""
    pts = np.asarray(points, F32)
    n = len(pts)
    nrm = np.asarray(normals, F32)
    if nrm.ndim == 1:
        nrm = np.broadcast_to(nrm, (n, 3))
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    thr = F32(threshold)
    need = max(3, int(min_neighbors))
    fin = np.isfinite(pts).all(axis=1)
    usable = fin if skip is None else fin & ~np.asarray(skip, bool)
    k = len(rows)
    out = dict(flag=np.zeros(k, np.uint8), invalid=np.zeros(k, bool), own=np.zeros(k, bool), m=np.zeros(k, np.int64),
               max32=np.full(k, np.nan), max64=np.full(k, np.nan), closest=np.full(k, np.inf))
    ratio = spread = kmax = 0.0
    flips = 0
    chunk = max(8, min(512, (1 << 22) // max(n, 1)))
    h = None
    for a, r in enumerate(rows):
        if radius is not None and a % chunk == 0:
            sel = rows[a:a + chunk]
            h = ir.hits(pts, np.where(fin[sel], sel, 0), radius) & usable[None, :]
        nv = nrm[r]
        if not fin[r] or not np.isfinite(nv).all() or not nv.any():
            out["invalid"][a] = True
            continue
        if radius is not None:
            nb = np.nonzero(h[a % chunk])[0]
        else:
            nb = np.asarray(lists[a], np.int64)
            nb = nb[nb >= 0]
            nb = nb[usable[nb]]
        out["m"][a] = len(nb)
        if len(nb) == 0:
            out["invalid"][a] = True
            continue
        if len(nb) < need:
            continue
        u, v = basis(nv)
        g = gaps_of(pts[r], pts[nb], u, v)
        if g is None:
            continue
        out["max32"][a], out["max64"][a] = g["g32"].max(), g["g64"].max()
        out["flag"][a] = 1 if g["g32"].max() > thr else 0
        dist = np.abs(g["g32"].astype(np.float64) - float(thr))
        out["closest"][a] = dist.min()
        out["own"][a] = bool((dist <= g["E"]).any())
        flips += int((g["g64"].max() > float(thr)) != bool(out["flag"][a]))
        diff = np.abs(g["g32"].astype(np.float64) - g["g64"])
        ratio = max(ratio, float((diff / g["E"]).max()))
        spread = max(spread, float(diff.max()))
        kmax = max(kmax, float(g["kappa"].max()))
    out.update(ratio=ratio, spread=spread, kappa=kmax, flips=flips)
    return out


def unstable(ref):
    """how many queries own an unstable comparison"""
    return int(ref["own"].sum())


# ---- clouds with closed forms ----------------------------------------------------------------------------------------------
def planar_lattice(side=9, rotation=None):
    """side x side points (i, j, 0) and the normal z, both turned by `rotation` [3, 3] -> points, normal [3], ij"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)
    p = np.concatenate([g, np.zeros((len(g), 1))], axis=1).astype(np.float64)
    nrm = np.array([0.0, 0.0, 1.0])
    if rotation is not None:
        p, nrm = p @ np.asarray(rotation).T, np.asarray(rotation) @ nrm
    return np.ascontiguousarray(p.astype(F32)), nrm.astype(F32), g


def rotation(axis, angle):
    """Rodrigues"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def lattice_gap(ij, side):
    """the closed form at r = 1.5 spacings (the 8 surrounding points): interior pi / 4, edge pi, corner 3 pi / 2"""
    rim = ((ij == 0) | (ij == side - 1)).sum(axis=1)
    return np.where(rim == 0, np.pi / 4, np.where(rim == 1, np.pi, 1.5 * np.pi))


def ring(m, wedge, phase, radius=1.0):
    """a centre (record 0) and m points on a circle in the z = 0 plane around it: the gaps are equal but one of `wedge`,
    which starts at the reference's angle `phase` (so it spans the +-pi cut when phase < pi < phase + wedge).  With the
    normal z the basis is u = y, v = x: the point at angle a is (sin a, cos a, 0) -> points [m + 1, 3] float32"""
    step = (2 * np.pi - wedge) / (m - 1)
    a = phase + wedge + step * np.arange(m)
    p = np.stack([radius * np.sin(a), radius * np.cos(a), np.zeros(m)], axis=1)
    return np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), p]).astype(F32))
