"""Numpy restatement of StatisticalOutlierRemoval / RadiusOutlierRemoval (TEST INFRASTRUCTURE).

The reference's applyFilterIndices (filters/include/pcl/filters/impl/statistical_outlier_removal.hpp:47-132,
.../radius_outlier_removal.hpp:48-172) written out in numpy over the oracle's exact k-NN (oracle.pcl_oracle.KdTree).
Every sum runs sequentially, in the reference's order (a column-by-column loop over k, np.add.accumulate over the
points): the GPU's fixed-order tree sums are checked against these, not against np.sum.
"""
import numpy as np

from oracle import pcl_oracle as orc


def _finite(xyz):
    return np.isfinite(xyz).all(axis=1)


def _queries(n, indices):
    return np.arange(n, dtype=np.int64) if indices is None else np.asarray(indices, np.int64)


def sor_mean_distances(cloud, mean_k, indices=None, tree=None):
    """Per query (the cloud's points, or `indices` in their order): (mean distance float32 [m], valid bool [m])."""
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    q = _queries(len(xyz), indices)
    fin = _finite(xyz)
    nfin = int(fin.sum())
    K = min(int(mean_k) + 1, nfin)
    dist = np.zeros(len(q), np.float32)
    valid = fin[q] if len(q) else np.zeros(0, bool)
    if K == 0 or not valid.any():
        return dist, valid
    tree = tree or orc.KdTree(xyz)
    qv = q[valid]
    _, d2 = tree.knn(np.ascontiguousarray(xyz[qv]), K)
    s = np.zeros(len(qv), np.float64)
    for c in range(1, K):  # dist_sum += sqrt(nn_dists[k]): sqrt in double of the float d2, summed in order
        s += np.sqrt(d2[:, c].astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        dist[valid] = (s / np.float64(K - 1)).astype(np.float32)
    return dist, valid


def sor_statistics(dist, valid, std_mul):
    """(sum, sq_sum, valid, mean, stddev, threshold): the reference's sequential double sums."""
    d = dist.astype(np.float64)
    sq = (dist * dist).astype(np.float64)  # distance * distance in float, then widened
    s = float(np.add.accumulate(d)[-1]) if len(d) else 0.0
    ss = float(np.add.accumulate(sq)[-1]) if len(d) else 0.0
    v = int(valid.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(s) / np.float64(v)
        var = (np.float64(ss) - np.float64(s) * np.float64(s) / np.float64(v)) / (np.float64(v) - 1.0)
        std = np.sqrt(var)
        thr = mean + np.float64(std_mul) * std
    return s, ss, v, float(mean), float(std), float(thr)


def sor_keep(dist, thr, negative):
    d = dist.astype(np.float64)
    with np.errstate(invalid="ignore"):
        removed = (d <= thr) if negative else (d > thr)  # NaN compares false both ways
    return ~removed


def statistical_outlier_removal(cloud, mean_k, std_mul, negative=False, indices=None, tree=None):
    """-> dict(kept, removed (original ids, in query order), dist, valid, mean, stddev, threshold, sum, sq_sum)."""
    dist, valid = sor_mean_distances(cloud, mean_k, indices, tree)
    s, ss, v, mean, std, thr = sor_statistics(dist, valid, std_mul)
    keep = sor_keep(dist, thr, negative)
    q = _queries(len(cloud), indices)
    return dict(kept=q[keep].astype(np.int32), removed=q[~keep].astype(np.int32), dist=dist, valid=v, mean=mean,
                stddev=std, threshold=thr, sum=s, sq_sum=ss)


def ror_threshold(radius, dense):
    """The float t with "within" == (d2 <= t): dense (k-NN path) (double)d2 <= r*r; non-dense (radiusSearch) d2 < float(r*r)."""
    r2 = float(radius) * float(radius)
    t = np.float32(r2)
    if dense:
        if float(t) > r2:
            t = np.nextafter(t, np.float32(-np.inf))
    else:
        t = np.nextafter(t, np.float32(-np.inf))
    return t


def radius_outlier_removal(cloud, radius, min_pts, negative=False, dense=True, indices=None, tree=None):
    """-> dict(kept, removed) original ids in query order."""
    if radius == 0:
        raise ValueError("radius 0 is the reference's error path")
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    q = _queries(len(xyz), indices)
    fin = _finite(xyz)
    nfin = int(fin.sum())
    need = int(min_pts) + 1
    t = ror_threshold(radius, dense)
    enough = np.zeros(len(q), bool)
    qfin = fin[q] if len(q) else np.zeros(0, bool)
    if need <= nfin and qfin.any():
        tree = tree or orc.KdTree(xyz)
        _, d2 = tree.knn(np.ascontiguousarray(xyz[q[qfin]]), need)
        enough[qfin] = d2[:, need - 1] <= t
    if dense:
        keep = enough ^ bool(negative)
    else:
        keep = qfin & (enough ^ bool(negative))
    return dict(kept=q[keep].astype(np.int32), removed=q[~keep].astype(np.int32))
