"""A numpy restatement of pcl::ISSKeypoint3D without boundary estimation (keypoints/include/pcl/keypoints/impl/iss_3d.hpp
:164-208, 302-473), the yardstick of tests/test_gpu_iss*.py.  Not product code.

  neighbourhood   every finite point with float32 d2 < float32(r * r), d2 in FLANN's L2_Simple order
                  ((dx * dx) + dy * dy) + dz * dz, the point itself included -- by brute force
  scatter         C_i = sum (p_j - p_i)(p_j - p_i)^T, the coordinates widened to float64 before the subtraction, float64 sums
  eigenvalues     numpy.linalg.eigvalsh, e1 >= e2 >= e3
  saliency        s_i = e3 iff m_i >= min_neighbors, e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (a NaN ratio fails), else 0;
                  a point with e3 < 0 or a non-finite eigenvalue is not salient (include/pclhip.h: the deviation)
  non-max         s_i > 0, >= min_neighbors points within the non-max radius, no neighbour j with s_i < s_j (strict)
  output          the keypoints' indices, ascending

The bound the device's eigenvalues are held to: B_i = (m_i + 32) * 2^-53 * trace(C_i).  m_i * 2^-53 * trace bounds a
sequential float64 sum of m_i products in any order and reaches the eigenvalues by Weyl's inequality; the 32 is an
allowance for the two eigenvalue solvers.  A comparison whose two sides are closer than that bound allows is UNSTABLE:
  |e2 - gamma_21 * e1| <= 2 B,  |e3 - gamma_32 * e2| <= 2 B,  e3 <= B or e2 <= B,
  and in the non-max pass |s_i - s_j| <= B_i + B_j for unequal values.
restate() reports the points that own such a comparison (`own`) and those with such a point in their non-max
neighbourhood as well (`excluded`): only these may differ between two correct implementations."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -53
SOLVER_ALLOWANCE = 32

# the reference's own test (test/keypoints/test_iss_3d.cpp:50-101)
BUN0_RESOLUTION = 0.0058329
BUN0_KEYPOINTS = np.array([(-0.071112, 0.137670, 0.047518), (-0.041733, 0.127960, 0.016650), (-0.011943, 0.086771, 0.057009),
                           (0.031733, 0.099372, 0.038505), (-0.062116, 0.045145, 0.037802), (-0.048250, 0.167480, -0.000152)],
                          np.float32)
BUN0_RECORDS = [31, 98, 143, 178, 332, 371]


def load_bun0():
    """points [397, 3] float32 of tests/golden/pcd/bun0.pcd (ascii, x y z normal_x normal_y normal_z curvature)"""
    a = np.loadtxt(os.path.join(ROOT, "tests", "golden", "pcd", "bun0.pcd"), skiprows=11, dtype=np.float32)
    assert a.shape == (397, 7)
    return np.ascontiguousarray(a[:, :3])


def hits(points, rows, radius):
    """[len(rows), n] bool: float32 d2(points[rows[a]], points[b]) < float32(r * r); never true for a non-finite record"""
    pts = np.asarray(points, F32)
    with np.errstate(over="ignore"):
        t = F32(float(radius) * float(radius))
    q = pts[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[:, None, 0] - pts[None, :, 0]
        dy = q[:, None, 1] - pts[None, :, 1]
        dz = q[:, None, 2] - pts[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        return d2 < t  # (NaN compares false)


def scatter_of(points, radius, rows):
    """-> m [k] int64, C [k, 3, 3] float64 of the finite records `rows`"""
    pts = np.asarray(points, F32)
    chunk = max(8, min(256, (1 << 21) // max(len(pts), 1)))
    p64 = np.where(np.isfinite(pts), pts, 0).astype(np.float64)
    rows = np.asarray(rows, np.int64)
    m = np.zeros(len(rows), np.int64)
    c = np.zeros((len(rows), 3, 3), np.float64)
    for b in range(0, len(rows), chunk):
        r = rows[b:b + chunk]
        h = hits(pts, r, radius)
        m[b:b + chunk] = h.sum(axis=1)
        d = (p64[None, :, :] - p64[r][:, None, :]) * h[:, :, None]
        c[b:b + chunk] = np.einsum("abk,abl->akl", d, d)
    return m, c


def saliency_from(e, m, g21, g32, min_neighbors):
    """e [k, 3] descending -> s [k]"""
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (m >= min_neighbors) & np.isfinite(e).all(axis=1) & (e[:, 2] >= 0)
        ok &= (e[:, 1] / e[:, 0] < g21) & (e[:, 2] / e[:, 1] < g32)
    return np.where(ok, e[:, 2], 0.0)


def nms_of(points, radius, rows, sal, min_neighbors):
    """the non-max pass of the finite records `rows` over the saliencies `sal` [n] -> is_keypoint [k] bool, m [k]"""
    pts = np.asarray(points, F32)
    chunk = max(8, min(512, (1 << 22) // max(len(pts), 1)))
    rows = np.asarray(rows, np.int64)
    key = np.zeros(len(rows), bool)
    m = np.zeros(len(rows), np.int64)
    for b in range(0, len(rows), chunk):
        r = rows[b:b + chunk]
        h = hits(pts, r, radius)
        m[b:b + chunk] = h.sum(axis=1)
        top = np.where(h, sal[None, :], 0.0).max(axis=1)
        key[b:b + chunk] = (sal[r] > 0) & (m[b:b + chunk] >= min_neighbors) & ~(sal[r] < top)
    return key, m


def restate(points, salient_radius, non_max_radius, g21=0.975, g32=0.975, min_neighbors=5, widen=1.0):
    """-> dict: m, trace, eig [n, 3] (0 below min_neighbors, NaN for a non-finite record), sal [n], m_nms, keypoints (int32,
    ascending), B [n], own / excluded [n] bool (the module's docstring; `widen` multiplies B)"""
    pts = np.asarray(points, F32)
    n = len(pts)
    fin = np.isfinite(pts).all(axis=1)
    ids = np.nonzero(fin)[0]
    m = np.zeros(n, np.int64)
    trace = np.zeros(n)
    eig = np.full((n, 3), np.nan)
    mm, c = scatter_of(pts, salient_radius, ids)
    m[ids] = mm
    trace[ids] = np.trace(c, axis1=1, axis2=2)
    e = np.linalg.eigvalsh(c)[:, ::-1] if len(ids) else np.zeros((0, 3))
    eig[ids] = np.where((mm >= min_neighbors)[:, None], e, 0.0)
    sal = np.zeros(n)
    sal[ids] = saliency_from(e, mm, g21, g32, min_neighbors)
    key = np.zeros(n, bool)
    m_nms = np.zeros(n, np.int64)
    key[ids], m_nms[ids] = nms_of(pts, non_max_radius, ids, sal, min_neighbors)
    # the unstable comparisons
    B = widen * (m + SOLVER_ALLOWANCE) * U * trace
    own = np.zeros(n, bool)
    live = fin & (m >= min_neighbors)
    e1, e2, e3 = eig[:, 0], eig[:, 1], eig[:, 2]
    with np.errstate(invalid="ignore"):
        own |= live & ((np.abs(e2 - g21 * e1) <= 2 * B) | (np.abs(e3 - g32 * e2) <= 2 * B) | (e3 <= B) | (e2 <= B))
    excluded = own.copy()
    for b in range(0, len(ids), 512):
        r = ids[b:b + 512]
        h = hits(pts, r, non_max_radius)
        diff = np.abs(sal[r][:, None] - sal[None, :])
        close = h & (diff != 0) & (diff <= B[r][:, None] + B[None, :]) & (sal[r] > 0)[:, None]
        own[r] |= close.any(axis=1)
    for b in range(0, len(ids), 512):
        r = ids[b:b + 512]
        h = hits(pts, r, non_max_radius)
        excluded[r] = own[r] | (h & own[None, :]).any(axis=1)
    return dict(m=m, trace=trace, eig=eig, sal=sal, m_nms=m_nms, keypoints=np.nonzero(key)[0].astype(np.int32), B=B,
                own=own, excluded=excluded)


def unstable(ref):
    """how many points own an unstable comparison"""
    return int(ref["own"].sum())


def median_spacing(points):
    """the median over the finite points of the distance to the nearest other point (float32 d2, sqrt in float64)"""
    pts = np.asarray(points, F32)
    ids = np.nonzero(np.isfinite(pts).all(axis=1))[0]
    near = np.empty(len(ids))
    for b in range(0, len(ids), 512):
        r = ids[b:b + 512]
        dx = pts[r][:, None, 0] - pts[None, ids, 0]
        dy = pts[r][:, None, 1] - pts[None, ids, 1]
        dz = pts[r][:, None, 2] - pts[None, ids, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(len(r)), b + np.arange(len(r))] = np.inf
        near[b:b + 512] = d2.min(axis=1)
    return float(np.median(np.sqrt(near.astype(np.float64))))


# ---- lattices with closed forms --------------------------------------------------------------------------------------------
def lattice(shape, spacing=(1, 1, 1)):
    """the points (i * sx, j * sy, k * sz), 0 <= (i, j, k) < shape, float32 (small integers: every difference, square and sum
    of them is exact in float32 and float64) -> points [n, 3], ijk [n, 3] int64"""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray((g * np.asarray(spacing)).astype(F32)), g


def lattice_offsets(spacing, radius):
    """the offsets (integer multiples of the spacings) with |v|^2 < float32(r * r) (every |v|^2 here is an exact float32)"""
    t = float(F32(float(radius) * float(radius)))
    reach = [int(radius // s) + 1 for s in spacing]
    g = np.stack(np.meshgrid(*[np.arange(-k, k + 1) for k in reach], indexing="ij"), axis=-1).reshape(-1, 3)
    v = g * np.asarray(spacing)
    return g[(v * v).sum(axis=1) < t]


def lattice_closed_form(spacing, radius):
    """an interior point of such a lattice: m and the eigenvalues (descending) of C = diag(sum vx^2, sum vy^2, sum vz^2) --
    the mixed sums cancel, v and its mirror images are all offsets"""
    off = lattice_offsets(spacing, radius)
    v = off * np.asarray(spacing)
    return len(off), np.sort((v * v).sum(axis=0).astype(np.float64))[::-1]


def lattice_interior(ijk, shape, spacing, radii):
    """points further from every face of the lattice than the sum of `radii` (in lattice steps, each rounded up): with one
    radius, the ball lies inside the lattice; with (salient, non-max), every point of the non-max ball has its salient
    ball inside"""
    ok = np.ones(len(ijk), bool)
    for a in range(3):
        k = sum(int(r // spacing[a]) + 1 for r in radii)
        ok &= (ijk[:, a] >= k) & (ijk[:, a] < shape[a] - k)
    return ok
