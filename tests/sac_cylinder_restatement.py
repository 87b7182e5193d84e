"""numpy restatement of pcl::SampleConsensusModelCylinder under pcl::RandomSampleConsensus (sample_consensus/.../impl/
sac_model_cylinder.hpp:49-140,182-265,268-309,453-489, sample_consensus/src/sac_model_cylinder.cpp:42-143, impl/ransac.hpp:
56-217, common/.../distances.h:75-80, common/impl/common.hpp:58-68) with the project's draws (tests/scp_restatement.py) and
the replay of tests/sac_restatement.py with the exponent 2.  The contract is stated in include/pclhip.h.

The float parts are elementwise float32 numpy (no contraction): the bits the device has to meet.  The double parts (acos,
sqrt, the blend) are numpy's and differ from the device's by ulps, so a flag is compared only where |distance - threshold|
> BAND * max(threshold, distance) and where wed is that far from the threshold; a gate likewise.  in_band / gate_band count
the pairs and hypotheses inside.  Every test asserts first that there are none.

A float sum of three products of an Eigen::Vector3f has three possible orders; `order` picks one:
  0  x x' + (y y' + z z')    the contract (dot3v: Eigen's unrolled scalar reduction of size 3)
  1  (x x' + y y') + z z'
  2  (x x' + z z') + y y'    (dot3, the Vector4f packet order)
order_sensitive() counts the flags on which they differ.

The refit is Levenberg-Marquardt in float64 on the reference's objective in the reference's parametrisation; gn_step() is
the Gauss-Newton step at given coefficients, the measure of how far they are from the minimum."""
import math
import struct

import numpy as np

import sac_models_restatement as sm
import sac_restatement as sac
import scp_restatement as sr

F = np.float32
BAND = sm.BAND
DBL_MAX = sac.DBL_MAX
FLT_EPS = F(np.finfo(np.float32).eps)


def dot3v(u, v, order=0):
    """float32 dot of (..., 3) arrays in a Vector3f's order"""
    with np.errstate(all="ignore"):
        a, b, c = u[..., 0] * v[..., 0], u[..., 1] * v[..., 1], u[..., 2] * v[..., 2]
        if order == 0:
            return a + (b + c)
        return (a + b) + c if order == 1 else (a + c) + b


def normalized3v(v, order=0):
    """Eigen's normalized() of (..., 3) float32 in a Vector3f's order"""
    v = np.asarray(v, F)
    q = dot3v(v, v, order)
    with np.errstate(all="ignore"):
        r = np.sqrt(q)
        return np.where((q > 0)[..., None], v / r[..., None], v).astype(F)


def cross(a, b):
    with np.errstate(all="ignore"):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def model_from_samples(p1, p2, n1, n2, radius_min=-DBL_MAX, radius_max=DBL_MAX):
    """computeModelCoefficients (:75-140) in the reference's Vector4f order -> (coefficients float32 [7], skipped)"""
    p1, p2, n1, n2 = (np.asarray(v, F)[:3] for v in (p1, p2, n1, n2))
    with np.errstate(all="ignore"):
        skipped = bool((np.abs(p1 - p2) <= FLT_EPS).all())  # isSampleGood (:59-68)
        w = (n1 + p1) - p2
        ld = cross(n1, n2)
        b, c, d, e = sm.dot3(n1, n2), sm.dot3(n2, n2), sm.dot3(n1, w), sm.dot3(n2, w)
        den = sm.dot3(ld, ld)
        sc = F(0) if np.float64(den) < 1e-8 else (b * e - c * d) / den
        lp = (p1 + n1) + sc * n1
        ld = sm.normalized(ld)
        l2 = sm.dot3(ld, ld)
        roots = []
        for p in (p1, p2):
            x = cross(ld, lp - p)
            roots.append(np.sqrt(np.float64(sm.dot3(x, x) / l2)))
        radius = F(0.5 * (roots[0] + roots[1]))
        if np.float64(radius) > radius_max or np.float64(radius) < radius_min:  # :133
            skipped = True
    return np.concatenate([lp, ld, [radius]]).astype(F), skipped


def e_out(ndw, threshold):
    """the least float32 e >= 0 with (1 - ndw) * double(e) > threshold, by bisection over the bits; NaN: none / no tier 1"""
    if not (0.0 <= ndw <= 1.0):
        return F(np.nan)
    om = 1.0 - float(ndw)

    def val(bits):
        return struct.unpack("<f", struct.pack("<I", bits))[0]

    def out(bits):
        with np.errstate(all="ignore"):
            return bool(np.float64(om) * np.float64(val(bits)) > threshold)
    lo, hi = 0, 0x7F800000
    if not out(hi):
        return F(np.nan)
    if out(lo):
        return F(0)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if out(mid):
            hi = mid
        else:
            lo = mid
    return F(val(hi))


class Model:
    def __init__(self, ndw=0.1, radius_min=-DBL_MAX, radius_max=DBL_MAX, axis=(0, 0, 0), eps_angle=0.0, order=0):
        self.ndw = float(ndw)
        self.radius_min, self.radius_max = float(radius_min), float(radius_max)
        self.axis = np.asarray(axis, F)
        self.eps_angle = float(eps_angle)
        self.order = order

    def gate(self, coeff):
        """isModelValid (:453-489) -> (valid, inside the band of a bound)"""
        c = np.asarray(coeff, F)
        valid, near = True, False
        with np.errstate(all="ignore"):
            if self.eps_angle > 0.0:
                ang = sm.folded_angle(dot3v(normalized3v(self.axis, self.order), normalized3v(c[3:6], self.order), self.order))
                near = near or bool(sm.near(ang, self.eps_angle))
                if ang > self.eps_angle:
                    valid = False
            if self.radius_min != -DBL_MAX and np.float64(c[6]) < self.radius_min:
                valid = False
            if self.radius_max != DBL_MAX and np.float64(c[6]) > self.radius_max:
                valid = False
        return valid, near

    def parts(self, pts, unit_normals, coeff):
        """-> (wed float64, d_normal float64) per point (:206-217)"""
        c = np.asarray(coeff, F)
        o = self.order
        with np.errstate(all="ignore"):
            ld = normalized3v(c[3:6], o)
            diff = pts - c[0:3]
            t = dot3v(diff, ld, o)
            dirv = (diff - t[:, None] * ld).astype(F)
            e = np.abs(np.sqrt(dot3v(dirv, dirv, o)) - c[6])
            wed = (np.float64(1.0) - np.float64(self.ndw)) * e.astype(np.float64)
            d_normal = sm.folded_angle(dot3v(unit_normals, normalized3v(dirv, o), o))
        return wed, d_normal

    def distances(self, pts, unit_normals, coeff):
        """getDistancesToModel (:143-179), whatever the gate says"""
        wed, dn = self.parts(pts, unit_normals, coeff)
        with np.errstate(all="ignore"):
            return np.abs(np.float64(self.ndw) * dn + wed)

    def within(self, pts, unit_normals, coeff, threshold):
        """the inlier test (:206-221) -> (bool mask, pairs inside a band)"""
        wed, dn = self.parts(pts, unit_normals, coeff)
        with np.errstate(all="ignore"):
            dist = np.abs(np.float64(self.ndw) * dn + wed)
            early = wed > threshold
            mask = ~early & (dist < threshold)
            band = sm.near(wed, threshold) | (~early & sm.near(dist, threshold))
        return mask, int(np.count_nonzero(band))


def point_set(cloud, normals, indices=None):
    """the (n, 3) points, the (n, 3) raw normals and the unit normals (the normal plane's staging: dot3's order) of the set,
    and the cloud index of every position"""
    pts, ids = sac.point_set(cloud, indices)
    raw = np.ascontiguousarray(np.asarray(normals, F)[ids][:, :3])
    return pts, raw, sm.normalized(raw), ids


def evaluate(model, cloud, normals, coeffs, threshold, indices=None):
    """-> (counts, valid, in_band, gate_band) of (H, 7) coefficient rows"""
    pts, raw, un, ids = point_set(cloud, normals, indices)
    counts, valid, in_band, gate_band = [], [], 0, 0
    for c in np.asarray(coeffs, F).reshape(-1, 7):
        ok, near = model.gate(c)
        gate_band += int(near)
        if ok and len(pts) > 0:
            mask, nb = model.within(pts, un, c, threshold)
            counts.append(int(mask.sum()))
            in_band += nb
        else:
            counts.append(0)
        valid.append(ok)
    return np.array(counts, np.uint32), np.array(valid, bool), in_band, gate_band


def order_sensitive(model_kw, cloud, normals, coeffs, threshold, indices=None):
    """how many flags differ between the three orders of the Vector3f sums"""
    pts, raw, un, ids = point_set(cloud, normals, indices)
    differ = 0
    for c in np.asarray(coeffs, F).reshape(-1, 7):
        masks = [Model(order=o, **model_kw).within(pts, un, c, threshold)[0] for o in (0, 1, 2)]
        differ += int(np.count_nonzero((masks[0] != masks[1]) | (masks[0] != masks[2])))
    return differ


class Replay(sac.Replay):
    """tests/sac_restatement.py's replay with the model's sample size as the exponent (ransac.hpp:165)"""

    def __init__(self, max_iterations, probability, n, sample_size=2):
        super().__init__(max_iterations, probability, n)
        self.sample_size = sample_size

    def feed(self, skipped, count):
        trial = self.trials
        self.trials += 1
        if skipped:
            self.skipped += 1
            if self.skipped < self.max_iterations * 10:
                return True
            self.done = True
            return False
        if count > self.best:
            self.best = int(count)
            self.best_trial = trial
            w = float(self.best) * self.one_over_n
            p = 1.0 - math.pow(w, float(self.sample_size))
            p = max(sac.DBL_EPS, p)
            p = min(1.0 - sac.DBL_EPS, p)
            self.k = self.log_probability / math.log(p)
        self.iterations += 1
        if self.iterations > self.k or self.iterations > self.max_iterations:
            self.done = True
            return False
        return True


def hypotheses(cloud, normals, count, seed=0, indices=None):
    """the coefficients of the first `count` trials' samples (skipped ones included), (count, 7) float32"""
    pts, raw, un, ids = point_set(cloud, normals, indices)
    out = []
    for t in range(count):
        s = sr.select_samples(int(seed), t, 2, len(pts))
        out.append(model_from_samples(pts[s[0]], pts[s[1]], raw[s[0]], raw[s[1]])[0])
    return np.array(out, F)


def compute_model(model, cloud, normals, threshold, max_iterations=10000, probability=0.99, seed=0, indices=None):
    """RandomSampleConsensus::computeModel -> dict(found, coefficients, inliers, outliers (cloud indices in the set's order),
    sample (positions), iterations, skipped, trials, best_trial, best_count, trace, in_band, gate_band)"""
    pts, raw, un, ids = point_set(cloud, normals, indices)
    n = len(pts)
    r = Replay(max_iterations, probability, max(n, 1))
    trace, best, best_s, in_band, gate_band = [], None, None, 0, 0
    while n >= 2 and not r.done:
        t = r.trials
        s = sr.select_samples(int(seed), t, 2, n)
        coeff, skipped = model_from_samples(pts[s[0]], pts[s[1]], raw[s[0]], raw[s[1]], model.radius_min, model.radius_max)
        valid, count = False, 0
        if not skipped:
            valid, near = model.gate(coeff)
            gate_band += int(near)
            if valid:
                mask, nb = model.within(pts, un, coeff, threshold)
                count, in_band = int(mask.sum()), in_band + nb
        trace.append(dict(samples=list(s), skipped=skipped, coefficients=coeff, count=count, valid=valid))
        before = r.best
        r.feed(skipped, count)
        if r.best != before:
            best, best_s = coeff, list(s)
    out = dict(found=best is not None, coefficients=best, sample=best_s, iterations=r.iterations, skipped=r.skipped,
               trials=r.trials, best_trial=r.best_trial, best_count=r.best, trace=trace, in_band=in_band, gate_band=gate_band)
    if best is None:
        out.update(inliers=np.zeros(0, np.int32), outliers=ids.copy())
        return out
    mask, _ = model.within(pts, un, best, threshold)
    out.update(inliers=ids[mask], outliers=ids[~mask])
    return out


def select(model, cloud, normals, coeff, threshold, indices=None):
    """selectWithinDistance with the gate -> (inliers, outliers (cloud indices), in_band, gate_band)"""
    pts, raw, un, ids = point_set(cloud, normals, indices)
    ok, near = model.gate(coeff)
    if not ok or len(pts) == 0:
        return ids[:0], ids.copy(), 0, int(near)
    mask, nb = model.within(pts, un, coeff, threshold)
    return ids[mask], ids[~mask], nb, int(near)


# ---- the refit, float64 ----

def frame(coeff, pts):
    """src/sac_model_cylinder.cpp:107-124 -> (ref_pt, ref_dir, u, v)"""
    c = np.asarray(coeff, np.float64)
    P = np.asarray(pts, np.float64)
    lp, ld = c[0:3].copy(), c[3:6].copy()
    q = float(ld @ ld)
    if q > 0:
        ld = ld / math.sqrt(q)
    lp = lp + ((P.mean(axis=0) - lp) @ ld) * ld
    ax, ay, az = np.abs(ld)
    pick = (0 if ax < az else 2) if ax < ay else 1
    u = np.zeros(3)
    u[pick] = 1.0
    u = u - ld[pick] * ld
    uq = float(u @ u)
    if uq > 0:
        u = u / math.sqrt(uq)
    return lp, ld, u, np.cross(ld, u)


def residuals(x, fr, pts, jac=True):
    """f (m,) and J (m, 5) of src/sac_model_cylinder.cpp:60-101 at the unknowns x"""
    ref_pt, ref_dir, u, v = fr
    P = np.asarray(pts, np.float64)
    lp = ref_pt + x[0] * u + x[1] * v
    ld = ref_dir + x[2] * u + x[3] * v
    sqr = float(ld @ ld)
    with np.errstate(all="ignore"):
        b = lp - P
        cr = np.cross(ld, b)
        dist = np.sqrt((cr * cr).sum(axis=1) / sqr)
        f = dist - abs(x[4])
        if not jac:
            return f, None
        dir_b = b @ ld
        d = b - dir_b[:, None] * ld / sqr
        du, dv = (d @ u) / dist, (d @ v) / dist
        J = np.column_stack([du, dv, -du * dir_b / sqr, -dv * dir_b / sqr, np.full(len(P), -1.0 if x[4] > 0 else 1.0)])
    return f, J


def coefficients_of(x, fr):
    """(line_pt, un-normalised direction, |r|) in float64"""
    ref_pt, ref_dir, u, v = fr
    return np.concatenate([ref_pt + x[0] * u + x[1] * v, ref_dir + x[2] * u + x[3] * v, [abs(x[4])]])


def rounded(c64, order=0):
    """the output of the refit: rounded to float32, the direction then normalised in float (:304-308)"""
    c = np.asarray(c64, np.float64).astype(F)
    c[3:6] = normalized3v(c[3:6], order)
    return c


def refit(pts, coeff, cap=100):
    """Levenberg-Marquardt in float64 from (0, 0, 0, 0, radius) -> (float64 coefficients with a unit direction or None,
    iterations).  None: a non-finite value, or no step that lowered the sum of squares."""
    P = np.asarray(pts, np.float64)
    fr = frame(coeff, P)
    x = np.array([0.0, 0.0, 0.0, 0.0, float(np.asarray(coeff, F)[6])])
    f, J = residuals(x, fr, P)
    if not (np.isfinite(f).all() and np.isfinite(J).all()):
        return None, 0
    cost, g, H = float(f @ f), J.T @ f, J.T @ J
    lam, nu, accepted, it = 1e-3, 2.0, 0, 0
    while it < cap and cost > 0.0 and lam <= 1e16:
        D = np.maximum(np.diag(H), 1e-300)
        if (np.abs(g) <= 1e-12 * np.sqrt(np.diag(H) * cost)).all():
            break
        try:
            d = -np.linalg.solve(H + lam * np.diag(D), g)
        except np.linalg.LinAlgError:
            lam, nu = lam * nu, nu * 2
            continue
        rs = abs(x[4])
        if (np.abs(d[[0, 1, 4]]) <= 1e-12 * rs).all() and (np.abs(d[[2, 3]]) <= 1e-12).all():
            break
        it += 1
        f2, J2 = residuals(x + d, fr, P)
        c2 = float(f2 @ f2)
        pred = 0.5 * float(d @ (lam * D * d - g))
        act = 0.5 * (cost - c2)
        if np.isfinite(c2) and np.isfinite(J2).all() and act > 0 and pred > 0:
            rho = act / pred
            x, cost, g, H = x + d, c2, J2.T @ f2, J2.T @ J2
            lam, nu, accepted = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0, accepted + 1
        else:
            lam, nu = lam * nu, nu * 2
    if accepted == 0:
        return None, it
    c = coefficients_of(x, fr)
    c[3:6] /= np.linalg.norm(c[3:6])
    return (c, it) if np.isfinite(c).all() else (None, it)


def gn_step(pts, coeff):
    """the Gauss-Newton step (J^T J)^-1 J^T f in the 5-parameter frame built AT `coeff`, float64: how far the coefficients
    are from the minimum of the refit's objective over `pts`"""
    P = np.asarray(pts, np.float64)
    c = np.asarray(coeff, np.float64)
    fr = frame(c, P)
    x = np.array([0.0, 0.0, 0.0, 0.0, c[6]])
    f, J = residuals(x, fr, P)
    return np.linalg.solve(J.T @ J, J.T @ f)
