"""numpy restatement of pcl::SampleConsensusPrerejective (registration/include/pcl/registration/
sample_consensus_prerejective.h, impl/sample_consensus_prerejective.hpp:78-348, correspondence_rejection_poly.h:208-338) with
the project's draw function (pcl_amd/csrc/scp_draw.hpp): a draw is a pure function of (seed, iteration, slot).

Precisions are the reference's: feature distances are FLANN's L2_Simple<float> (float32, dimension by dimension), the polygon
test is float32, umeyama is float64 (Eigen's, rounded to float32), the moved cloud is Transformer::se3 in float32, getFitness
compares float32 d2 < float32(corr_dist * corr_dist) and sums the inliers' d2 sequentially in float32."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
FLT_MAX = np.float32(np.finfo(np.float32).max)


# ---- draws (scp_draw.hpp) ---------------------------------------------------------------------------------------------
def draw_bits(seed, iteration, slot):
    z = (seed + 0x9E3779B97F4A7C15 * (((iteration << 8) | slot) + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_index(seed, iteration, slot, n):
    """getRandomIndex(n): int(n * u), u = (x >> 11) * 2^-53 -- mirrors n * (rand() / (RAND_MAX + 1.0))"""
    u = float(draw_bits(seed, iteration, slot) >> 11) * (1.0 / 9007199254740992.0)
    return int(float(n) * u)


def insert_samples(draws):
    """selectSamples (:96-117) on given draws (draw j in [0, n - j)): the sorted, duplicate-free sample list"""
    s = []
    for i, d in enumerate(draws):
        s.append(int(d))
        for j in range(i):
            if s[i] >= s[j]:
                s[i] += 1
            else:
                tmp = s[i]
                for k in range(i, j, -1):
                    s[k] = s[k - 1]
                s[j] = tmp
                break
    return s


def select_samples(seed, iteration, nr_samples, n):
    return insert_samples([draw_index(seed, iteration, i, n - i) for i in range(nr_samples)])


# ---- feature search ---------------------------------------------------------------------------------------------------
def feature_d2(target_rows, q):
    """L2_Simple<float> of one query row against every target row: float32, dimension 0 .. D-1 in order"""
    t = np.asarray(target_rows, np.float32)
    q = np.asarray(q, np.float32)
    acc = np.zeros(len(t), np.float32)
    with np.errstate(all="ignore"):
        for d in range(t.shape[1]):
            diff = q[d] - t[:, d]
            acc = acc + diff * diff
    return acc


def feature_knn(target_rows, query_rows, k):
    """-> (idx [nq, k] int32, d2 [nq, k] float32, counts [nq]): ascending (d2, index); non-finite target rows are never
    candidates, k is clamped to the finite ones, a non-finite query row has count 0; -1 / +inf behind the count"""
    t = np.asarray(target_rows, np.float32)
    qs = np.asarray(query_rows, np.float32)
    ok = np.isfinite(t).all(axis=1)
    cand = np.nonzero(ok)[0]
    kk = min(int(k), len(cand))
    idx = np.full((len(qs), k), -1, np.int32)
    d2 = np.full((len(qs), k), np.inf, np.float32)
    cnt = np.zeros(len(qs), np.uint32)
    for i, q in enumerate(qs):
        if not np.isfinite(q).all():
            continue
        d = feature_d2(t[cand], q)
        order = np.lexsort((cand, d))[:kk]
        idx[i, :kk] = cand[order]
        d2[i, :kk] = d[order]
        cnt[i] = kk
    return idx, d2, cnt


# ---- pre-rejection ------------------------------------------------------------------------------------------------------
def edge_sq(a, b):
    """computeSquaredDistance (correspondence_rejection_poly.h:302-310): float32, (dx*dx + dy*dy) + dz*dz"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = b - a
    return np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def edge_similar(dist_src, dist_tgt, simsq):
    """thresholdEdgeLength (:320-338) on the two squared lengths"""
    dist_src, dist_tgt, simsq = np.float32(dist_src), np.float32(dist_tgt), np.float32(simsq)
    with np.errstate(all="ignore"):
        sim = np.float32(dist_src / dist_tgt) if dist_src < dist_tgt else np.float32(dist_tgt / dist_src)
    return bool(sim >= simsq)


def threshold_polygon(src_pts, tgt_pts, similarity_threshold):
    """thresholdPolygon (:208-230) over the polygon's vertices in order: one edge when there are two"""
    thr = np.float32(similarity_threshold)
    simsq = np.float32(thr * thr)
    c = len(src_pts)
    edges = 1 if c == 2 else c
    for i in range(edges):
        j = (i + 1) % c
        if not edge_similar(edge_sq(src_pts[i], src_pts[j]), edge_sq(tgt_pts[i], tgt_pts[j]), simsq):
            return False
    return True


# ---- pose and score -----------------------------------------------------------------------------------------------------
def umeyama(src_pts, tgt_pts):
    """TransformationEstimationSVD: pcl::umeyama without scaling (common/include/pcl/common/impl/eigen.hpp:675-738) in
    float64 -> (4, 4) float64"""
    s = np.asarray(src_pts, np.float64)
    d = np.asarray(tgt_pts, np.float64)
    sm, dm = s.mean(axis=0), d.mean(axis=0)
    sigma = (d - dm).T @ (s - sm) / len(s)
    U, sv, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = dm - R @ sm
    return T


def transform_se3(T, pts):
    """Transformer<float>::se3 (common/include/pcl/common/impl/transforms.hpp:117-123): r0*x + (r1*y + (r2*z + r3))"""
    T = np.asarray(T, np.float32)
    p = np.asarray(pts, np.float32)
    out = np.empty((len(p), 3), np.float32)
    for r in range(3):
        out[:, r] = T[r, 0] * p[:, 0] + (T[r, 1] * p[:, 1] + (T[r, 2] * p[:, 2] + T[r, 3]))
    return out


def nearest_d2(moved, tgt):
    """float32 1-NN squared distance of every moved point in the target, (dx*dx + dy*dy) + dz*dz; +inf without a target or
    for a non-finite point"""
    tgt = np.asarray(tgt, np.float32)
    tgt = tgt[np.isfinite(tgt).all(axis=1)]
    out = np.full(len(moved), np.inf, np.float32)
    if len(tgt) == 0:
        return out
    with np.errstate(all="ignore"):
        for c0 in range(0, len(moved), 512):
            m = moved[c0:c0 + 512, None, :]
            d = m - tgt[None, :, :3]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            d2 = np.where(np.isfinite(m).all(axis=2), d2, np.float32(np.inf))
            out[c0:c0 + 512] = np.nanmin(np.where(np.isnan(d2), np.float32(np.inf), d2), axis=1)
    return out


def get_fitness(src, tgt, T, corr_dist):
    """getFitness (:310-348) -> (inlier indices, error float32 as the reference sums it, error float64 = the exact mean)"""
    with np.errstate(over="ignore"):
        max_range = np.float32(float(corr_dist) * float(corr_dist))  # +inf for the default distance
    d2 = nearest_d2(transform_se3(T, np.asarray(src)[:, :3]), np.asarray(tgt)[:, :3])
    inl = np.nonzero(d2 < max_range)[0]
    if len(inl) == 0:
        return inl, FLT_MAX, float(FLT_MAX)
    seq = np.cumsum(d2[inl], dtype=np.float32)[-1]  # a sequential float32 sum
    return inl, np.float32(seq / np.float32(len(inl))), float(d2[inl].astype(np.float64).sum() / len(inl))


def is_identity_guess(guess):
    """guess.isApprox(Identity, 0.01f): |G - I|^2 <= prec^2 * min(|G|^2, |I|^2)"""
    g = np.asarray(guess, np.float64).reshape(4, 4)
    return float(((g - np.eye(4)) ** 2).sum()) <= 1e-4 * min(float((g ** 2).sum()), 4.0)


def align(src, tgt, src_feat, tgt_feat, max_iterations=5000, nr_samples=3, k=2, similarity=0.6, inlier_fraction=0.0,
          corr_dist=np.sqrt(np.finfo(np.float64).max), seed=0, guess=None, transforms=None):
    """computeTransformation (:157-306).  transforms (optional): {iteration: (4, 4) float32} to score in place of the
    restatement's own umeyama (the device's, when a test compares the rest).
    -> dict(converged, T (4, 4) float32, inliers, best_iteration (-1: the guess, -2: none), lowest_error, rejected,
            trace [per iteration: samples, matches, rejected (0 scored, 1 polygon, 2 no usable match), T, T64, inliers (count),
            error, error64])"""
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32)
    n = len(src)
    cache = {}
    finite_tgt = int(np.isfinite(np.asarray(tgt_feat, np.float32)).all(axis=1).sum())
    final_T = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32).reshape(4, 4).copy()
    lowest = FLT_MAX
    converged = False
    inliers = np.zeros(0, np.int64)
    best_it = -2
    if not is_identity_guess(final_T):
        inl, err, _ = get_fitness(src, tgt, final_T, corr_dist)
        if np.float32(len(inl)) / np.float32(n) >= np.float32(inlier_fraction) and err < lowest:
            inliers, lowest, converged, best_it = inl, err, True, -1
    rejected = 0
    trace = []
    for it in range(max_iterations):
        s = select_samples(seed, it, nr_samples, n)
        m = []
        bad = False
        for j, row in enumerate(s):
            if row not in cache:
                cache[row] = feature_knn(tgt_feat, np.asarray(src_feat, np.float32)[row:row + 1], k)
            idx, _, cnt = cache[row]
            if cnt[0] == 0:
                m.append(-1)
                bad = True
                continue
            pick = 0 if k == 1 else draw_index(seed, it, nr_samples + j, int(cnt[0]))
            m.append(int(idx[0, pick]))
            if not np.isfinite(tgt[m[-1], :3]).all():
                bad = True
        rec = dict(iteration=it, samples=s, matches=m, rejected=0, T=None, T64=None, inliers=0, error=FLT_MAX, error64=None)
        trace.append(rec)
        if bad:
            rec["rejected"] = 2
        elif not threshold_polygon(src[s, :3], tgt[m, :3], similarity):
            rec["rejected"] = 1
        if rec["rejected"]:
            rejected += 1
            continue
        rec["T64"] = umeyama(src[s, :3], tgt[m, :3])
        rec["T"] = rec["T64"].astype(np.float32) if transforms is None else np.asarray(transforms[it], np.float32)
        inl, err, err64 = get_fitness(src, tgt, rec["T"], corr_dist)
        rec["inliers"], rec["error"], rec["error64"] = len(inl), err, err64
        if np.float32(len(inl)) / np.float32(n) >= np.float32(inlier_fraction) and err < lowest:
            inliers, lowest, converged, best_it = inl, err, True, it
            final_T = rec["T"]
    return dict(converged=converged, T=final_T, inliers=inliers, best_iteration=best_it, lowest_error=lowest, rejected=rejected,
                trace=trace, finite_targets=finite_tgt)


# ---- fixtures -----------------------------------------------------------------------------------------------------------
def load_bunny_pair():
    """the reference test's clouds (test/registration/test_sac_ia.cpp:140-160): bun0 moved by (100, 0, 0) and 90 degrees
    about z (transformPointCloud with offset and quaternion: the float32 matrix of the quaternion, Eigen's se3 order), and
    bun4 (tests/golden/bunny.npz) -> (source [397, 3], target [361, 3], the 4x4 that moved the source)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "bunny.npz"))
    a, b = np.ascontiguousarray(z["bun0"][:, :3], np.float32), np.ascontiguousarray(z["bun4"][:, :3], np.float32)
    assert a.shape == (397, 3) and b.shape == (361, 3)
    ang = np.float32(np.pi) / np.float32(2.0)
    w, z = np.float32(np.cos(ang / np.float32(2))), np.float32(np.sin(ang / np.float32(2)))
    T = np.eye(4, dtype=np.float32)
    T[0, 0] = T[1, 1] = np.float32(1) - np.float32(2) * z * z
    T[0, 1] = -np.float32(2) * w * z
    T[1, 0] = np.float32(2) * w * z
    T[0, 3] = 100.0
    return transform_se3(T, a), np.ascontiguousarray(b), T
