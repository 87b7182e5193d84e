"""Timing of CorrespondenceRejectorSampleConsensus at n pairs (default 10M) on the GPU, with HIP events.

  evaluate   pclhip_rejector_sac_evaluate of H = 1, 64 and 1,024 transforms over n pairs held in device memory (synth's sheet,
             its copy moved by the ground-truth transform plus noise, a third of the pairs mismatched): events on the context's
             stream around the call.  A call stages nothing (device pointers), gathers the pairs once and scores them in one
             pass, so time(H) - time(1) is the scoring kernel's share for H - 1 hypotheses; all three figures are printed.
  chain      one ICP iteration (pclhip_icp_iterate, its own events: search + chain + accumulate) at n points with
             [MedianDistance(4)] and with [MedianDistance(4), SampleConsensus(0.05, 1,000)]: the first iteration of an
             alignment and iterations of the converged loop; the difference is one application of the rejector.

Medians over the repeats; spread = (max - min) / median.  Writes profiles/rejector_sac_timing.json (and prints it).

    python scripts/rejector_sac_timing.py [n] [--repeats R]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med_spread(v):
    v = sorted(v)
    m = v[len(v) // 2]
    return dict(median_ms=round(m, 4), spread=round((v[-1] - v[0]) / m, 3) if m > 0 else 0.0, repeats=len(v))


def main():
    import torch

    import pcl_amd
    from pcl_amd import synth
    from pcl_amd._lib import check
    n = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 10_000_000
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 7
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = pcl_amd.Context(0, stream=stream.cuda_stream)
    out = dict(n=n, device=torch.cuda.get_device_name(0))

    # ---- evaluate --------------------------------------------------------------------------------------------------------
    T_gt = synth.ground_truth_transform()
    src = synth.gaussian_surface_device(n, seed=synth.SOURCE_SEED, device=dev)[:, :3].contiguous()
    tgt = synth.apply_rigid_device(T_gt, src)[:, :3].contiguous()
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    tgt += torch.randn(n, 3, generator=g, device=dev) * 1e-3
    q = torch.arange(n, dtype=torch.int32, device=dev)
    m = q.clone()
    bad = torch.rand(n, generator=g, device=dev) < (1.0 / 3.0)
    m[bad] = torch.randint(0, n, (int(bad.sum()),), generator=g, device=dev, dtype=torch.int32)
    rng = np.random.default_rng(0)
    lib = ctx.lib
    ev = {}
    for H in (1, 64, 1024):
        Ts = np.tile(np.asarray(T_gt, np.float32).reshape(1, 16), (H, 1))
        Ts[:, [3, 7, 11]] += rng.normal(0, 0.01, (H, 3)).astype(np.float32)  # H different hypotheses near the truth
        Ts[0] = np.asarray(T_gt, np.float32).reshape(16)
        cnt = np.zeros(H, np.uint32)
        times = []
        for rep in range(repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            check(lib.pclhip_rejector_sac_evaluate(
                ctx.h, C.c_void_p(src.data_ptr()), n, 12, C.c_void_p(tgt.data_ptr()), n, 12, C.c_void_p(q.data_ptr()),
                C.c_void_p(m.data_ptr()), n, 0.05, Ts.ctypes.data_as(C.POINTER(C.c_float)), H,
                C.c_void_p(cnt.ctypes.data)), ctx.h)
            e1.record(stream)
            e1.synchronize()
            if rep >= 2:  # two warm-up calls
                times.append(e0.elapsed_time(e1))
        ev["H=%d" % H] = dict(med_spread(times), inliers_of_truth=int(cnt[0]))
    ev["scoring_share_ms"] = {"63 hypotheses": round(ev["H=64"]["median_ms"] - ev["H=1"]["median_ms"], 4),
                              "1023 hypotheses": round(ev["H=1024"]["median_ms"] - ev["H=1"]["median_ms"], 4)}
    out["evaluate"] = ev
    del src, tgt, q, m, bad
    torch.cuda.empty_cache()

    # ---- chain -----------------------------------------------------------------------------------------------------------
    target = synth.gaussian_surface_device(n, device=dev)
    source = synth.apply_rigid_device(np.linalg.inv(T_gt), synth.gaussian_surface_device(n, seed=synth.SOURCE_SEED, device=dev))
    tree = pcl_amd.KdTree(ctx)
    tree.setInputCloud(target)
    chain = {}
    for name in ("median", "median+sac"):
        icp = pcl_amd.IterativeClosestPoint(ctx)
        icp.setSearchMethodTarget(tree)
        icp.setInputSource(source)
        icp.setMaxCorrespondenceDistance(0.1)
        med = pcl_amd.CorrespondenceRejectorMedianDistance()
        med.setMedianFactor(4.0)
        icp.addCorrespondenceRejector(med)
        sac = None
        if name == "median+sac":
            sac = pcl_amd.CorrespondenceRejectorSampleConsensus(ctx)
            icp.addCorrespondenceRejector(sac)
        first, conv, stats = [], [], None
        for rep in range(3):
            icp.reset()
            T = np.eye(4, dtype=np.float32)
            for it in range(12):
                sums = icp.iterate(T)
                ms = icp.lastKernelMs()
                T = icp.solve(sums)
                if it == 0:
                    first.append(ms)
                elif it >= 8:
                    conv.append(ms)
            if sac is not None:
                stats = sac.lastStats()
        chain[name] = dict(first_iteration=med_spread(first), converged_iteration=med_spread(conv))
        if stats is not None:
            chain[name]["last_application"] = {k: stats[k] for k in ("trials", "iterations", "best_count", "n", "has_model")}
        del icp
    chain["sac_application_ms"] = {
        "first_iteration": round(chain["median+sac"]["first_iteration"]["median_ms"] - chain["median"]["first_iteration"]["median_ms"], 4),
        "converged_iteration": round(chain["median+sac"]["converged_iteration"]["median_ms"] -
                                     chain["median"]["converged_iteration"]["median_ms"], 4)}
    out["chain"] = chain
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "rejector_sac_timing.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
