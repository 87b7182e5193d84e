"""StatisticalOutlierRemoval / RadiusOutlierRemoval timing at 10M points: GPU time of the fused filters (HIP events around
all of a call's kernels), of the composition a user could write without them (pclhip_knn(k = 51) into device tensors,
then the mean distances, statistics and classification in torch), and the oracle's CPU k-NN with 16 threads for the
same mean distances.  Writes profiles/outlier_timing.json (and prints it).

    python scripts/outlier_timing.py [n] [--no-oracle]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pcl_amd  # noqa: E402


def noisy_surface(n, seed=11):
    """synth.gaussian_surface with 2 % uniform outliers, 1 % duplicates and 1 % NaN rows"""
    rng = np.random.default_rng(seed)
    c = pcl_amd.synth.gaussian_surface(n)[:, :3].astype(np.float32).copy()
    lo, hi = c.min(0), c.max(0)
    o = rng.choice(n, n // 50, replace=False)
    c[o] = rng.uniform(lo, hi, size=(len(o), 3)).astype(np.float32)
    d = rng.choice(n, n // 100, replace=False)
    c[d] = c[rng.choice(n, len(d))]
    z = rng.choice(n, n // 100, replace=False)
    c[z, rng.integers(0, 3, len(z))] = np.nan
    return c


def median_ms(fn, reps=5):
    fn()  # warm-up
    v = sorted(fn() for _ in range(reps))
    return v[len(v) // 2]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 10_000_000
    import torch
    ctx = pcl_amd.Context(0)
    c = noisy_surface(n)
    out = {"metric": "outlier_timing", "points": n, "cloud": "synth.gaussian_surface + 2% uniform outliers, 1% duplicates, 1% NaN"}
    tree = pcl_amd.KdTree(ctx)
    tree.setInputCloud(c)
    out["index_build_ms"] = round(tree.build_ms(), 3)

    sor = pcl_amd.StatisticalOutlierRemoval(ctx, extract_removed_indices=True)
    sor.setInputCloud(c)
    sor.setSearchMethod(tree)
    sor.setMeanK(50)
    sor.setStddevMulThresh(1.0)

    def run_sor():
        sor.filterIndices()
        return sor.lastKernelMs()
    ms = median_ms(run_sor)
    out["sor_50_1.0"] = {"gpu_ms": round(ms, 3), "kept": int(n - len(sor.getRemovedIndices())),
                         "removed": int(len(sor.getRemovedIndices())), "statistics": sor.lastStatistics()}
    for name, r, mp in (("ror_0.0012_8", 0.0012, 8), ("ror_0.0015_4", 0.0015, 4)):
        ror = pcl_amd.RadiusOutlierRemoval(ctx, extract_removed_indices=True)
        ror.setInputCloud(c)
        ror.setSearchMethod(tree)
        ror.setRadiusSearch(r)
        ror.setMinNeighborsInRadius(mp)

        def run_ror():
            ror.filterIndices()
            return ror.lastKernelMs()
        ms = median_ms(run_ror)
        rem = len(ror.getRemovedIndices())
        out[name] = {"gpu_ms": round(ms, 3), "removed": int(rem), "removed_fraction": round(rem / n, 4)}

    # the composition: k-NN lists (k = 51) into device memory, then torch
    q = torch.from_numpy(c).cuda()
    torch.cuda.synchronize()

    def run_knn():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        idx, d2 = tree.nearestKSearch(q, 51)
        e1.record()
        torch.cuda.synchronize()
        run_knn.last = (idx, d2, tree.lastKernelMs())
        return e0.elapsed_time(e1)
    knn_ms = median_ms(run_knn, reps=3)
    idx, d2, knn_kernel_ms = run_knn.last
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fin = torch.isfinite(q).all(1)
    dist = torch.sqrt(d2[:, 1:].double()).sum(1) / 50.0
    dist = torch.where(fin, dist, torch.zeros_like(dist)).float()
    v = fin.sum().double()
    s, ss = dist.double().sum(), (dist * dist).double().sum()
    mean = s / v
    thr = mean + torch.sqrt((ss - s * s / v) / (v - 1.0))
    keep = ~(dist.double() > thr)
    kept = torch.nonzero(keep).flatten()
    e1.record()
    torch.cuda.synchronize()
    out["composition_knn51_torch"] = {
        "gpu_ms": round(knn_ms + e0.elapsed_time(e1), 3), "knn_call_ms": round(knn_ms, 3),
        "knn_kernel_ms": round(knn_kernel_ms, 3), "torch_ms": round(e0.elapsed_time(e1), 3),
        "knn_output_bytes": int(idx.numel() * 4 + d2.numel() * 4), "kept": int(kept.numel())}
    del idx, d2, dist, keep, kept
    torch.cuda.empty_cache()

    if "--no-oracle" not in sys.argv:
        from oracle import pcl_oracle
        t0 = time.perf_counter()
        ot = pcl_oracle.KdTree(c)
        t1 = time.perf_counter()
        fq = np.isfinite(c).all(1)
        _, od2 = ot.knn(np.ascontiguousarray(c[fq]), 51, nthreads=16)
        t2 = time.perf_counter()
        out["oracle_cpu_16_threads"] = {"build_s": round(t1 - t0, 3), "knn51_s": round(t2 - t1, 3)}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "outlier_timing.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
