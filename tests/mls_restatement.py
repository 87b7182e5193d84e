"""A numpy restatement of pcl::MovingLeastSquares::process without upsampling (surface/include/pcl/surface/mls.h,
impl/mls.hpp: performProcessing, computeMLSPointNormal, MLSResult::computeMLSSurface, ::projectQueryPoint) for polynomial
orders 0 .. 2 and the projection methods NONE and SIMPLE -- the yardstick of tests/test_gpu_mls*.py.  Not product code; written
from the semantics in include/pclhip.h, float64 throughout, the neighbours in ascending distance.

  neighbourhood   every finite point with float32 d2 < float32(r * r), d2 in FLANN's L2_Simple order, the point itself
                  included -- by brute force (iss_restatement.hits); m < 3: no output record
  plane           c = mean p_j, C = sum (p_j - c)(p_j - c)^T; numpy.linalg.eigh: l0 <= l1 <= l2, n the eigenvector of l0, its
                  component of largest magnitude positive (ties: the lowest axis); mean = q - ((q - c) . n) n;
                  curvature = |l0 / trace| (0 when the trace is 0); v = unitOrthogonal(n) (Eigen's rule), u = n x v
  fit             order 2 and m >= 6: d = p_j - mean, w = exp(-d.d / sqr_gauss_param), (u, v, f) = (d.u, d.v, d.n),
                  P = (1, v, v^2, u, uv, u^2); (P diag(w) P^T) coeff = P diag(w) f by Cholesky; a pivot that is not positive
                  or a coeff[0] that is not finite: the plane stays
  projection      fit and SIMPLE: point = mean + coeff[0] n, normal = normalize(n - coeff[3] u - coeff[1] v);
                  else point = mean, normal = n

Conditioning, per output record: gap = (l1 - l0) / trace (0 when the trace is 0), cond = the 2-norm condition number of the fit
matrix with u and v measured in units of r (row and column k divided by r^deg(k); 1 without a fit),
kappa = max(1, 1 / gap, cond).  The bound two correct float64 implementations are held to:
  |d point| <= (m + A) * 2^-53 * kappa * r,   |d normal| (up to sign), |d curvature| <= (m + A) * 2^-53 * kappa
m * 2^-53 bounds a sequential sum of m terms in any order, kappa carries it through the eigenvector (Davis-Kahan: 1 / gap) and
the solve (cond), and A allows for the two eigen solvers, the Cholesky and the exp.  A record whose point bound exceeds
1e-3 * r (kappa of about 1e10) is `excluded`: its answer is not determined by the data.

Far from the origin.  Those bounds scale with r and know nothing of |q|.  Normal and curvature are functions of coordinate
differences and keep their bound wherever the cloud lies -- provided the implementation keeps its intermediates relative to
the query (query_relative=True: e = p_j - q exactly, o = mean - q, d = e - o, q added once).  The default formulations here
follow the reference and subtract a mean that was rounded at |q|; at |q| = 8192 their normals leave the bound sixfold
(tests/test_far_clouds_restatement.py).  The point cannot avoid one rounding at |q|: far_point_term() = 2 * 2^-53 * max_i |q_i|
joins bound_point wherever a point is compared far out (one half-ulp of the final q + offset per implementation).

A = SOLVER_ALLOWANCE is set from this restatement ALONE (spread(): 8 random neighbour orders, two-pass against one-pass shifted
sums, matrix product against moments, the query-relative formulation in the second half of the orders), never from a run of the device code: it stays at iss_restatement's 32 while the
measured spread stays within a quarter of the bound.  Measured worst |d| / bound over the clouds of
tests/test_mls_restatement.py::test_order_spread_sets_the_allowance: see MEASURED_WORST_SPREAD below."""
import os

import numpy as np

import iss_restatement as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -53
SOLVER_ALLOWANCE = 32
SPREAD_CAP = 0.25              # A stays 32 while the restatement's own spread stays within this share of the bound
MEASURED_WORST_SPREAD = 0.1881  # (a point of bun0 at r = 0.0075; 0.1411 at r = 0.01, 0.0035 at r = 0.03) the worst |d| / bound that test_order_spread_sets_the_allowance printed for the formulations that subtract a mean
# With the query-relative formulation in spread()'s rotation the same test prints 0.2489: its POINT at bun0 r = 0.0075 against
# bound_point + far_point_term -- the point moved by 2.78e-17, one ulp of a double at |q| = 0.19; normals at most 0.0549,
# curvatures 0.0214.  Far from the origin (tests/test_far_clouds_restatement.py, the 2^-10 grid moved by (8192, -8192, 4096)
# against the unmoved restatement plus the shift), worst |d| / bound of the query-relative formulation:
MEASURED_FAR_QUERY_RELATIVE = {0.1: (0.0000, 0.0008, 0.0008), 0.06: (0.8101, 0.0074, 0.0016)}  # r -> (point with far_point_term, normal, curvature)
# and of the two that subtract a mean rounded at |q|: normal 5.878 at r = 0.1 and 6.361 at r = 0.06 (both), point 0.989 / 0.994
NONE, SIMPLE, ORTHOGONAL = 0, 1, 2

# the reference's own test (test/surface/test_moving_least_squares.cpp:95-118): record 0 of bun0 at r = 0.03, order 2
BUN0_POINT0 = (0.005417, 0.113463, 0.040715)
BUN0_ABS_NORMAL0 = (0.111894, 0.594906, 0.795969)
BUN0_CURVATURE0 = 0.012019

load_bun0 = ir.load_bun0


def sign_rule(n):
    """the component of largest magnitude positive, ties to the lowest axis"""
    k = int(np.argmax(np.abs(n)))  # (the first of equal maxima)
    return -n if n[k] < 0 else n


def unit_orthogonal(n):
    """Eigen's unitOrthogonal for 3-vectors (isMuchSmallerThan at 1e-12)"""
    x, y, z = n
    if not (abs(x) <= abs(z) * 1e-12) or not (abs(y) <= abs(z) * 1e-12):
        h = np.sqrt(x * x + y * y)
        return np.array([-y / h, x / h, 0.0])
    h = np.sqrt(y * y + z * z)
    return np.array([0.0, -z / h, y / h])


def cholesky_solve(a, b):
    """-> x with a x = b, or None when a pivot is not positive (NaN included)"""
    k = len(b)
    l = np.zeros((k, k))
    for j in range(k):
        d = a[j, j] - np.dot(l[j, :j], l[j, :j])
        if not d > 0.0:
            return None
        l[j, j] = np.sqrt(d)
        for i in range(j + 1, k):
            l[i, j] = (a[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    y = np.zeros(k)
    for i in range(k):
        y[i] = (b[i] - np.dot(l[i, :i], y[:i])) / l[i, i]
    x = np.zeros(k)
    for i in range(k - 1, -1, -1):
        x[i] = (y[i] - np.dot(l[i + 1:, i], x[i + 1:])) / l[i, i]
    return x


# exponents (a, b) of u^a v^b in P = (1, v, v^2, u, uv, u^2): the reference's order, ui outer and vi inner
TERMS = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)]
DEGREE = np.array([a + b for a, b in TERMS])


def fit_system(uj, vj, fj, w, moments):
    """-> (A [6, 6], rhs [6]) = (sum w P P^T, sum w P f), as the matrix product or assembled from the moments sum w u^a v^b"""
    if not moments:
        P = np.stack([uj ** a * vj ** b for a, b in TERMS])
        Pw = P * w[None, :]
        return Pw @ P.T, Pw @ fj
    mom = {(a, b): np.sum(w * uj ** a * vj ** b) for a in range(5) for b in range(5 - a)}
    fm = {(a, b): np.sum(w * fj * uj ** a * vj ** b) for a, b in TERMS}
    A = np.array([[mom[(ak + al, bk + bl)] for (al, bl) in TERMS] for (ak, bk) in TERMS])
    return A, np.array([fm[t] for t in TERMS])


def one_point(q, nb, radius, sqr_gauss_param, order, method, one_pass=False, moments=False, query_relative=False):
    """q [3] float64, nb [m, 3] float64 (m >= 3) in the order the sums are to run -> dict of the record.  query_relative: the
    formulation that never subtracts a value rounded at the point's coordinates (the module's docstring)"""
    m = len(nb)
    if query_relative:
        return one_point_query_relative(q, nb, radius, sqr_gauss_param, order, method, moments)
    if one_pass:  # shifted by the query: C = sum d d^T - (sum d)(sum d)^T / m
        d = nb - q
        s = d.sum(axis=0)
        C = d.T @ d - np.outer(s, s) / m
        c = q + s / m
    else:
        c = nb.sum(axis=0) / m
        d = nb - c
        C = d.T @ d
    C = (C + C.T) / 2
    w, V = np.linalg.eigh(C)
    trace = C[0, 0] + C[1, 1] + C[2, 2]
    n = sign_rule(V[:, 0] / np.linalg.norm(V[:, 0]))
    mean = q - np.dot(q - c, n) * n
    curvature = abs(w[0] / trace) if trace != 0 else 0.0
    gap = (w[1] - w[0]) / trace if trace > 0 else 0.0
    rec = dict(m=m, plane_point=mean, plane_normal=n, curvature=curvature, gap=gap, cond=1.0, fitted=False, point=mean,
               normal=n)
    if order == 2 and m >= 6:
        v = unit_orthogonal(n)
        u = np.cross(n, v)
        d = nb - mean
        wt = np.exp(-np.einsum("ij,ij->i", d, d) / sqr_gauss_param)
        uj, vj, fj = d @ u, d @ v, d @ n
        A, rhs = fit_system(uj, vj, fj, wt, moments)
        coeff = cholesky_solve(A, rhs)
        if coeff is not None and np.isfinite(coeff[0]):
            rec["fitted"] = True
            scale = float(radius) ** -DEGREE.astype(np.float64)
            As = A * scale[:, None] * scale[None, :]
            rec["cond"] = float(np.linalg.cond(As)) if np.isfinite(As).all() else np.inf
            if method == SIMPLE:
                rec["point"] = mean + coeff[0] * n
                o = n - coeff[3] * u - coeff[1] * v
                rec["normal"] = o / np.linalg.norm(o)
    return rec


def one_point_query_relative(q, nb, radius, sqr_gauss_param, order, method, moments=False):
    """one_point with every intermediate relative to the query: e = p_j - q (exact in float64 for float32 inputs within a
    factor 2^29 of each other), C = sum e e^T - (sum e)(sum e)^T / m, o = mean - q = ((sum e / m) . n) n, the fit's
    d = e - o, and q is added ONCE, to o or to o + coeff[0] n"""
    m = len(nb)
    e = nb - q
    s = e.sum(axis=0)
    C = e.T @ e - np.outer(s, s) / m
    C = (C + C.T) / 2
    w, V = np.linalg.eigh(C)
    trace = C[0, 0] + C[1, 1] + C[2, 2]
    n = sign_rule(V[:, 0] / np.linalg.norm(V[:, 0]))
    o = np.dot(s / m, n) * n  # q - c = -(sum e) / m
    curvature = abs(w[0] / trace) if trace != 0 else 0.0
    gap = (w[1] - w[0]) / trace if trace > 0 else 0.0
    rec = dict(m=m, plane_point=q + o, plane_normal=n, curvature=curvature, gap=gap, cond=1.0, fitted=False, point=q + o,
               normal=n)
    if order == 2 and m >= 6:
        v = unit_orthogonal(n)
        u = np.cross(n, v)
        d = e - o
        wt = np.exp(-np.einsum("ij,ij->i", d, d) / sqr_gauss_param)
        uj, vj, fj = d @ u, d @ v, d @ n
        A, rhs = fit_system(uj, vj, fj, wt, moments)
        coeff = cholesky_solve(A, rhs)
        if coeff is not None and np.isfinite(coeff[0]):
            rec["fitted"] = True
            scale = float(radius) ** -DEGREE.astype(np.float64)
            As = A * scale[:, None] * scale[None, :]
            rec["cond"] = float(np.linalg.cond(As)) if np.isfinite(As).all() else np.inf
            if method == SIMPLE:
                rec["point"] = q + (o + coeff[0] * n)
                t = n - coeff[3] * u - coeff[1] * v
                rec["normal"] = t / np.linalg.norm(t)
    return rec


def far_point_term(points, indices):
    """per output record: 2 * 2^-53 * max_i |q_i| -- each of two correct implementations rounds its final q + offset once, to
    half an ulp (at most 2^-53 |value|) of a value of the magnitude of q.  A derived rounding bound that joins bound_point
    where clouds lie far from the origin; it is no allowance, SPREAD_CAP does not govern it."""
    q = np.asarray(points, F32)[np.asarray(indices, np.int64), :3].astype(np.float64)
    return 2.0 * U * np.abs(q).max(axis=1) if len(q) else np.zeros(0)


def restate(points, radius, sqr_gauss_param=None, order=2, method=SIMPLE, rows=None, rng=None, one_pass=False,
            moments=False, query_relative=False):
    """-> dict over the k output records (those of `rows`, default every record, with m >= 3, ascending): indices int32, m,
    point / normal / plane_point / plane_normal [k, 3], curvature, fitted, gap, cond, kappa, bound_point, bound_unit,
    excluded; and m_all [len(rows)].  rng: the neighbours in a random order instead of ascending distance."""
    pts = np.asarray(points, F32)[:, :3]
    n = len(pts)
    if sqr_gauss_param is None:
        sqr_gauss_param = float(radius) * float(radius)  # setSearchRadius
    fin = np.isfinite(pts).all(axis=1)
    rows = np.nonzero(fin)[0] if rows is None else np.asarray(rows, np.int64)[fin[np.asarray(rows, np.int64)]]
    p64 = np.where(np.isfinite(pts), pts, 0).astype(np.float64)
    recs, ids, m_all = [], [], np.zeros(len(rows), np.int64)
    chunk = max(8, min(256, (1 << 21) // max(n, 1)))
    for b in range(0, len(rows), chunk):
        r = rows[b:b + chunk]
        h = ir.hits(pts, r, radius)
        for a, i in enumerate(r):
            nb = np.nonzero(h[a])[0]
            m_all[b + a] = len(nb)
            if len(nb) < 3:
                continue
            with np.errstate(over="ignore"):
                dd = pts[nb] - pts[i]
                d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
            nb = nb[np.argsort(d2, kind="stable")] if rng is None else nb[rng.permutation(len(nb))]
            recs.append(one_point(p64[i], p64[nb], radius, sqr_gauss_param, order, method, one_pass, moments, query_relative))
            ids.append(i)
    k = len(recs)
    vec = lambda key: np.array([x[key] for x in recs], np.float64).reshape(k, 3)  # noqa: E731
    sca = lambda key, t=np.float64: np.array([x[key] for x in recs], t).reshape(k)  # noqa: E731
    out = dict(indices=np.array(ids, np.int32), m=sca("m", np.int64), point=vec("point"), normal=vec("normal"),
               plane_point=vec("plane_point"), plane_normal=vec("plane_normal"), curvature=sca("curvature"),
               fitted=sca("fitted", bool), gap=sca("gap"), cond=sca("cond"), m_all=m_all)
    with np.errstate(divide="ignore"):
        out["kappa"] = np.maximum(1.0, np.maximum(1.0 / out["gap"], out["cond"]))
        out["bound_unit"] = (out["m"] + SOLVER_ALLOWANCE) * U * out["kappa"]
    out["bound_point"] = out["bound_unit"] * float(radius)
    out["excluded"] = ~(out["bound_unit"] <= 1e-3)  # bound_point > 1e-3 r (inf and NaN included)
    return out


def normal_delta(a, b):
    """per row: the distance of two unit vectors up to sign"""
    return np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)) if len(a) else np.zeros(0)


def spread(points, radius, sqr_gauss_param=None, orders=8, seed=0):
    """the restatement against itself: the neighbours in `orders` random orders, in both formulations of the plane sums and of
    the fit matrix -> the worst |d| / bound over the records that are not excluded (point, normal, curvature), the largest
    absolute moves (point, normal) and the base restatement.  The second half of the orders runs the query-relative
    formulation (with either fit matrix); its point -- q + offset, where the others form q - ... and mean + ... -- is held to
    bound_point + far_point_term: the last rounding at |q| is that term's, a derived bound, and no business of the allowance.
    Normal and curvature of every formulation, and the point of the others, are held to the bounds with A alone."""
    base = restate(points, radius, sqr_gauss_param)
    keep = ~base["excluded"]
    far = far_point_term(points, base["indices"])
    worst = np.zeros(3)
    moved = np.zeros(2)
    rng = np.random.default_rng(seed)
    for t in range(orders):
        other = restate(points, radius, sqr_gauss_param, rng=rng, one_pass=bool(t & 1), moments=bool(t & 2),
                        query_relative=bool(t & 4))
        assert np.array_equal(other["indices"], base["indices"]) and np.array_equal(other["m"], base["m"])
        assert np.array_equal(other["fitted"][keep], base["fitted"][keep])
        dp = np.abs(other["point"] - base["point"]).max(axis=1)[keep]
        dn = normal_delta(other["normal"], base["normal"])[keep]
        dc = np.abs(other["curvature"] - base["curvature"])[keep]
        if keep.any():
            bp = (base["bound_point"] + far if t & 4 else base["bound_point"])[keep]
            worst = np.maximum(worst, [(dp / bp).max(), (dn / base["bound_unit"][keep]).max(),
                                       (dc / base["bound_unit"][keep]).max()])
            moved = np.maximum(moved, [dp.max(), dn.max()])
    return worst, moved, base


# ---- clouds with closed forms ---------------------------------------------------------------------------------------------
def plane_lattice(nx=9, ny=8):
    """integer points (i, j, 0): every sum of the plane pass is exact"""
    return np.ascontiguousarray(ir.lattice((nx, ny, 1))[0])


def rotation(seed=4):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def axis_line(k=12):
    """integer points on the x axis: C = diag(s, 0, 0) exactly"""
    p = np.zeros((k, 3), F32)
    p[:, 0] = np.arange(k)
    return p


def almost_on_line():
    """the reference's cloud (test/surface/test_moving_least_squares.cpp:66-70), r = 4.65032"""
    return np.array([(13.1647, 9.62041, 0.0), (13.2399, 13.1738, 0.0), (13.2623, 14.2374, 0.0), (13.2799, 15.0696, 0.0)], F32)


ALMOST_ON_LINE_RADIUS = 4.65032


def edge_groups(seed=11):
    """isolated groups of 2, 3, 5 and 6 points in general position (each within 0.5 of its centre, the centres 10 apart)
    and one isolated point -> points [17, 3], group size per record"""
    rng = np.random.default_rng(seed)
    pts, size = [], []
    for g, k in enumerate((2, 3, 5, 6, 1)):
        pts.append((rng.random((k, 3)) * 0.5 + (10.0 * g, 0.0, 0.0)).astype(F32))
        size += [k] * k
    order = rng.permutation(len(size))
    return np.ascontiguousarray(np.concatenate(pts)[order]), np.array(size)[order]
