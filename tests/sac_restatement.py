"""numpy restatement of pcl::SACSegmentation for SACMODEL_PLANE under SAC_RANSAC (segmentation/include/pcl/segmentation/
impl/sac_segmentation.hpp:79-133, sample_consensus/.../impl/ransac.hpp:56-217, impl/sac_model_plane.hpp:80-118,153-230,
311-360, sac_model_plane.h:299-320) with the project's draws (pcl_amd/csrc/scp_draw.hpp through tests/scp_restatement.py).

Everything per point is elementwise float32 numpy, which does not contract a multiply with an add: the bit pattern the
device has to meet.  The stopping rule is float64 with libm's log and pow, as in the reference.  The refit is the reference's
own float path (oracle.pcl_oracle.mean_and_covariance + solve_plane_parameters: computeMeanAndCovarianceMatrix and
pcl::eigen33 in their float order)."""
import math
import sys

import numpy as np

import scp_restatement as sr

F = np.float32
DBL_EPS = sys.float_info.epsilon
DBL_MAX = sys.float_info.max


def point_set(cloud, indices=None):
    """the (n, 3) float32 points of the set, in its order, and the cloud index of every position"""
    c = np.asarray(cloud, F)[:, :3]
    ids = np.arange(len(c), dtype=np.int32) if indices is None else np.asarray(indices, np.int32).reshape(-1)
    return np.ascontiguousarray(c[ids]), ids


def plane_from_samples(p0, p1, p2):
    """computeModelCoefficients (impl/sac_model_plane.hpp:93-113) -> (coefficients float32 [4], skipped)"""
    p0, p1, p2 = (np.asarray(p, F) for p in (p0, p1, p2))
    with np.errstate(all="ignore"):
        u, v = p1 - p0, p2 - p0
        cx = u[1] * v[2] - u[2] * v[1]
        cy = u[2] * v[0] - u[0] * v[2]
        cz = u[0] * v[1] - u[1] * v[0]
        norm = np.sqrt((cx * cx + cy * cy) + cz * cz)
        skipped = bool(norm < F(1e-5))  # Eigen's dummy_precision<float>; false for a NaN
        a, b, c = cx / norm, cy / norm, cz / norm
        d = -((a * p0[0] + b * p0[1]) + c * p0[2])
    return np.array([a, b, c, d], F), skipped


def within(pts, coeff, threshold):
    """the one inlier test: fabsf((a x + b y) + (c z + d)) < float(threshold), strict -> bool mask"""
    a, b, c, d = (F(v) for v in coeff)
    with np.errstate(all="ignore"):
        e = (a * pts[:, 0] + b * pts[:, 1]) + (c * pts[:, 2] + d)
        return np.abs(e) < F(threshold)


def count_within(pts, coeff, threshold):
    return int(np.count_nonzero(within(pts, coeff, threshold)))


class Replay:
    """ransac.hpp:66-202 on a sequence of (skipped, count): pcl_amd/csrc/sac_replay.hpp"""

    def __init__(self, max_iterations, probability, n):
        self.max_iterations = int(max_iterations)
        with np.errstate(all="ignore"):
            self.log_probability = float(np.log(np.float64(1.0) - np.float64(probability)))
        self.one_over_n = 1.0 / float(n)
        self.iterations = 0
        self.skipped = 0
        self.best = 0
        self.k = DBL_MAX
        self.best_trial = -1
        self.trials = 0
        self.done = False

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
            p = 1.0 - math.pow(w, 3.0)
            p = max(DBL_EPS, p)
            p = min(1.0 - DBL_EPS, p)
            self.k = self.log_probability / math.log(p)
        self.iterations += 1
        if self.iterations > self.k or self.iterations > self.max_iterations:
            self.done = True
            return False
        return True


def replay_counts(seq, max_iterations=50, probability=0.99, n=100):
    """the stopping rule on a hand-made sequence of (skipped, count) -> the Replay after the loop ended (or ran out)"""
    r = Replay(max_iterations, probability, n)
    for skipped, count in seq:
        if not r.feed(skipped, count):
            break
    return r


def refit(cloud, inlier_ids):
    """optimizeModelCoefficients (impl/sac_model_plane.hpp:331-359) in the reference's float path -> coefficients or None"""
    from oracle import pcl_oracle as orc
    cov, cen, cnt = orc.mean_and_covariance(np.asarray(cloud, F), np.asarray(inlier_ids, np.int32))
    if cnt == 0:
        return None
    nx, ny, nz, _ = orc.solve_plane_parameters(cov)
    n = np.array([nx, ny, nz], F)
    d = -((n[0] * cen[0] + n[1] * cen[1]) + n[2] * cen[2])
    out = np.array([n[0], n[1], n[2], d], F)
    return out if np.isfinite(out).all() else None


def segment(cloud, threshold, max_iterations=50, probability=0.99, optimize=True, seed=0, indices=None):
    """-> dict(found, coefficients (unrefined winner), refined (or None), inliers, outliers (cloud indices in the set's
    order, after the refined selection when there is one), first_inliers (the winner's own selection), iterations,
    skipped, trials, best_trial, best_count, trace [dict(samples, skipped, coefficients, count)])"""
    pts, ids = point_set(cloud, indices)
    n = len(pts)
    r = Replay(max_iterations, probability, max(n, 1))
    trace, best = [], None
    while n >= 3 and not r.done:
        t = r.trials
        s = sr.select_samples(int(seed), t, 3, n)
        coeff, skipped = plane_from_samples(pts[s[0]], pts[s[1]], pts[s[2]])
        count = 0 if skipped else count_within(pts, coeff, threshold)
        trace.append(dict(samples=s, skipped=skipped, coefficients=coeff, count=count))
        before = r.best
        r.feed(skipped, count)
        if r.best != before:
            best = coeff
    out = dict(found=best is not None, coefficients=best, refined=None, iterations=r.iterations, skipped=r.skipped,
               trials=r.trials, best_trial=r.best_trial, best_count=r.best, trace=trace)
    if best is None:
        out.update(inliers=np.zeros(0, np.int32), first_inliers=np.zeros(0, np.int32), outliers=ids.copy())
        return out
    mask = within(pts, best, threshold)
    out["first_inliers"] = ids[mask]
    if optimize and int(mask.sum()) > 3:
        ref = refit(np.asarray(cloud, F), ids[mask])
        if ref is not None:
            out["refined"] = ref
            mask = within(pts, ref, threshold)
    out["inliers"] = ids[mask]
    out["outliers"] = ids[~mask]
    return out


def unstable(pts, coeff, threshold):
    """a float64 evaluation puts some point within 4 * 2^-24 * (|a x| + |b y| + |c z| + |d|) of the threshold: the float
    result may then depend on the order of the operations"""
    p = np.asarray(pts, np.float64)
    a, b, c, d = (float(v) for v in coeff)
    if not np.isfinite([a, b, c, d]).all():
        return False
    ok = np.isfinite(p).all(axis=1)
    p = p[ok]
    e = np.abs(a * p[:, 0] + b * p[:, 1] + c * p[:, 2] + d)
    mag = np.abs(a * p[:, 0]) + np.abs(b * p[:, 1]) + np.abs(c * p[:, 2]) + abs(d)
    return bool((np.abs(e - float(F(threshold))) <= 4.0 * 2.0 ** -24 * mag).any())
