"""SampleConsensusPrerejective timing on one MI355X: synth.icp_pair downsampled with VoxelGrid to about 10^5 points per cloud,
the source moved by a large rigid motion, k = 8 normals, FPFH; 50,000 iterations, 3 samples, randomness 5, similarity 0.9.
Records, in one run: the time per align and per launch kind (feature k-NN, hypotheses, fitness), the hypotheses that
survive the pre-rejection, source points scored per second -- and the two baselines, never the code under test:
  scoring         the same surviving transforms (the first --baseline-transforms of them) through a host loop of
                  pclhip_icp_fitness_score, the only composition the library offered before, against pclhip_scp_evaluate
                  of the same transforms; the inlier counts must agree (the loop's `d2 <= max_range` in double is given
                  the float below float(corr_dist^2), which is `d2 < float(corr_dist^2)` on float distances)
  feature search  torch.cdist + topk on the device over the same rows against pclhip_feature_knn
Writes profiles/scp_timing.json (and prints it).

    python scripts/scp_timing.py [n_raw] [--leaf L]

The GPU work runs as a child process under its own `timeout`; a failure ends the run.
"""
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_TIMEOUT_S = 540
PEAK_BYTES_PER_S = 8.0e12  # HBM3E of the MI355X
ITERATIONS, SAMPLES, RANDOMNESS, SIMILARITY = 50000, 3, 5, 0.9


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def big_motion():
    import numpy as np
    a = math.pi / 2
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [10.0, -3.0, 2.0]
    return T


def prepare(n_raw, leaf):
    import numpy as np
    import torch

    import pcl_amd
    ctx = pcl_amd.Context(0)
    tgt_raw, src_raw, _ = pcl_amd.synth.icp_pair(n_raw)
    src_raw = pcl_amd.synth.apply_rigid(np.linalg.inv(big_motion()), src_raw)
    clouds, feats, trees = [], [], []
    radius = None
    for raw in (src_raw, tgt_raw):
        vg = pcl_amd.VoxelGrid(ctx)
        vg.setInputCloud(torch.from_numpy(raw).cuda())
        vg.setLeafSize(leaf)
        c = vg.filter().contiguous()
        if radius is None:  # about 30 neighbours on a surface of ~4 units of area
            radius = math.sqrt(30.0 * 4.0 / (math.pi * len(c)))
        tree = pcl_amd.KdTree(ctx)
        tree.setInputCloud(c)
        ne = pcl_amd.NormalEstimation(ctx)
        ne.setInputCloud(c)
        ne.setSearchMethod(tree)
        ne.setKSearch(8)
        ne.compute()
        f = pcl_amd.FPFHEstimation(ctx)
        f.setInputCloud(c)
        f.setSearchMethod(tree)
        f.setRadiusSearch(radius)
        fp = f.compute()
        clouds.append(c)
        feats.append(torch.nan_to_num(fp).contiguous())
        trees.append(tree)
    torch.cuda.synchronize()
    return torch, pcl_amd, ctx, clouds, feats, trees, radius


def step(n_raw, leaf, n_base, reps=3):
    import numpy as np
    torch, pcl_amd, ctx, (src, tgt), (fs, ft), (_, ttree), radius = prepare(n_raw, leaf)
    corr = 1.5 * leaf
    out = {"source_points": len(src), "target_points": len(tgt), "fpfh_radius": radius, "max_correspondence_distance": corr}
    s = pcl_amd.SampleConsensusPrerejective(ctx)
    s.setInputSource(src)
    s.setSearchMethodTarget(ttree)
    s.setSourceFeatures(fs)
    s.setTargetFeatures(ft)
    s.setMaxCorrespondenceDistance(corr)
    s.setMaximumIterations(ITERATIONS)
    s.setNumberOfSamples(SAMPLES)
    s.setCorrespondenceRandomness(RANDOMNESS)
    s.setSimilarityThreshold(SIMILARITY)
    s.setSeed(1)
    # the first align searches the feature neighbours (the cache is empty); the later ones find them cached
    rows = []
    for rep in range(reps + 1):
        if rep <= 1:
            s.setTargetFeatures(ft)  # drops the cache: rep 0 is the warm-up, rep 1 the cold call that is reported
        s.align()
        r = s.result
        rows.append(dict(total_ms=r.total_ms, knn_ms=r.knn_ms, hypothesis_ms=r.hypothesis_ms, fitness_ms=r.fitness_ms,
                         knn_rows=int(r.knn_rows)))
    cold, warm = rows[1], rows[2:]
    survivors = ITERATIONS - int(s.result.rejected)
    fit_ms = median([w["fitness_ms"] for w in warm])
    out["align_cold_cache"] = {k: round(v, 3) if isinstance(v, float) else v for k, v in cold.items()}
    out["align_cached_median"] = {k: round(median([w[k] for w in warm]), 3) for k in ("total_ms", "knn_ms", "hypothesis_ms", "fitness_ms")}
    out["iterations"] = ITERATIONS
    out["survivors"] = survivors
    out["converged"] = bool(s.result.converged)
    out["best_count"] = int(s.result.best_count)
    out["best_error"] = float(s.result.best_error)
    out["pose_error_vs_truth"] = float(np.abs(s.getFinalTransformation().astype(np.float64) @ np.linalg.inv(big_motion()) @
                                              np.linalg.inv(pcl_amd.synth.ground_truth_transform()) - np.eye(4)).max())
    out["source_points_scored_per_s"] = survivors * len(src) / (fit_ms * 1e-3) if fit_ms > 0 else None
    icp = pcl_amd.IterativeClosestPoint(ctx)
    icp.setSearchMethodTarget(ttree)
    icp.setInputSource(src)
    bound = np.float32(corr * corr)
    below = float(np.nextafter(bound, np.float32(0)))

    def scoring(similarity):
        """the surviving transforms of a traced run (not timed) through pclhip_scp_evaluate and through the host loop"""
        s.setSimilarityThreshold(similarity)
        s.align(trace_capacity=ITERATIONS)
        scored = [t for t in s.trace if not t["rejected"]]
        Ts = np.stack([t["transformation"] for t in scored])[:n_base]
        dev_cnt = np.array([t["inliers"] for t in scored][:n_base], np.uint32)
        walls = []
        for _ in range(reps + 1):  # wall time around a call that ends in a synchronise; the first is the warm-up
            t0 = time.perf_counter()
            cnt, err = s.evaluate(Ts)
            walls.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(cnt, dev_cnt)
        batched_ms = median(walls[1:])

        def loop():
            counts = np.zeros(len(Ts), np.uint32)
            for h, T in enumerate(Ts):
                icp.getFitnessScore(max_range=below, transform=T)
                counts[h] = icp.fitness_points
            return counts
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            base_cnt = loop()
            walls.append((time.perf_counter() - t0) * 1e3)
        loop_ms = walls[1]
        return {"similarity_threshold": similarity, "survivors": len(scored), "transforms": len(Ts),
                "batched_evaluate_ms": round(batched_ms, 3), "host_loop_fitness_score_ms": round(loop_ms, 3),
                "ratio_loop_over_batched": round(loop_ms / batched_ms, 2),
                "source_points_scored_per_s_batched": len(Ts) * len(src) / (batched_ms * 1e-3),
                "inlier_counts_agree": bool(np.array_equal(base_cnt, cnt)), "count_mismatches": int((base_cnt != cnt).sum())}
    out["scoring"] = scoring(SIMILARITY)
    # the same comparison where the pre-rejection lets more through (the reference's default threshold): the workload above
    # leaves a handful of hypotheses, which measures launch overheads on both sides
    out["scoring_similarity_0.6"] = scoring(0.6)
    # feature search: every source row against the target rows
    k = RANDOMNESS
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    pcl_amd.featureKSearch(ctx, ft, fs[:4096], k)  # warm-up
    walls = []
    for _ in range(3):  # wall time: the call ends in a synchronise (and copies 5 indices per query to the host)
        t0 = time.perf_counter()
        idx, d2, _ = pcl_amd.featureKSearch(ctx, ft, fs, k)
        walls.append((time.perf_counter() - t0) * 1e3)

    def cdist_topk():
        res = []
        for a in range(0, len(fs), 8192):
            d = torch.cdist(fs[a:a + 8192], ft)
            res.append(torch.topk(d, k, dim=1, largest=False).indices)
        return torch.cat(res)
    cdist_topk()
    e[2].record()
    ref = cdist_topk()
    e[3].record()
    torch.cuda.synchronize()
    agree = float((torch.from_numpy(idx.astype(np.int64)).cuda() == ref).float().mean())
    knn_ms, cd_ms = median(walls), e[2].elapsed_time(e[3])
    out["feature_search"] = {"queries": len(fs), "targets": len(ft), "k": k, "feature_knn_call_ms": round(knn_ms, 3),
                             "torch_cdist_topk_ms": round(cd_ms, 3), "ratio_cdist_over_knn": round(cd_ms / knn_ms, 3),
                             "index_agreement": round(agree, 5)}
    # rooflines: the target rows a query must see (132 B each), 16 B per scored source point
    nbytes_knn = len(ft) * 132
    out["roofline_feature_knn"] = {"target_row_bytes_per_query": nbytes_knn,
                                   "flops_per_query": 3 * 33 * len(ft),
                                   "ms_at_8TBps_if_read_once_per_64_queries": round(nbytes_knn * len(fs) / 64 / PEAK_BYTES_PER_S * 1e3, 4)}
    nbytes_fit = 16 * survivors * len(src)
    out["roofline_fitness"] = {"algorithmic_bytes": nbytes_fit, "ms_at_8TBps": round(nbytes_fit / PEAK_BYTES_PER_S * 1e3, 4),
                               "fraction_of_8TBps": round(nbytes_fit / PEAK_BYTES_PER_S * 1e3 / fit_ms, 4) if fit_ms > 0 else None}
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n_raw", nargs="?", type=int, default=2_000_000)
    ap.add_argument("--leaf", type=float, default=0.0066, help="VoxelGrid leaf: about 10^5 points on the synthetic surface")
    ap.add_argument("--baseline-transforms", type=int, default=1000)
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process")
    ap.add_argument("--out", default=None, help="with --step: where the JSON goes")
    a = ap.parse_args()
    if a.step:
        text = json.dumps(step(a.n_raw, a.leaf, a.baseline_transforms))
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return 0
    out = {"metric": "scp_timing", "raw_points": a.n_raw, "leaf": a.leaf,
           "cloud": "synth.icp_pair through VoxelGrid, source moved by 90 degrees about z and (10, -3, 2); k = 8 normals, FPFH",
           "nr_samples": SAMPLES, "correspondence_randomness": RANDOMNESS, "similarity_threshold": SIMILARITY}
    with tempfile.TemporaryDirectory() as tmp:
        piece = os.path.join(tmp, "step.json")
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), str(a.n_raw), "--leaf",
               repr(a.leaf), "--baseline-transforms", str(a.baseline_transforms), "--step", "--out", piece]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("the GPU step failed with status %d: stopping" % rc, file=sys.stderr)
            return rc
        with open(piece) as f:
            out.update(json.load(f))
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scp_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
