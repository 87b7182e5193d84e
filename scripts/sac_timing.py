"""SACSegmentation (planes, RANSAC) timing at 10M points: synth's Gaussian surface with a fifth of the points turned into
uniform clutter, 1,024 hypotheses scored in one pass of sac_count_kernel (a segment() call that cannot stop early:
probability 1, max_iterations 1,023, batch_size 1,024).  The baseline, taken in the same run, is what the library offered
before: the same 1,024 models (read from the call's trace) scored in torch on the device,
((P @ M.T + d).abs() < thr).sum(0), over chunks of the points (the whole product would be 40 GB).  Records for both the
milliseconds and the points x hypotheses per second, how many counts differ (the matmul rounds in another order), the
ratio, and the fraction of the fp32 VALU roofline the fused pass reaches: per pair of (point, hypothesis) pairs three packed
multiplies, three packed adds and two compares, so 4 issue slots per pair against CUs x 64 lanes x clock.
Writes profiles/sac_timing.json (and prints it).

    python scripts/sac_timing.py [n] [--hypotheses H]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS_PER_PAIR = 4.0
CHUNK = 1 << 18  # points per matmul of the baseline: a 1 GB product at 1,024 hypotheses


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    import pcl_amd
    n, H, thr = a.n, a.hypotheses, 0.002
    assert 1 <= H <= 1024
    ctx = pcl_amd.Context(0)
    cloud = pcl_amd.synth.gaussian_surface_device(n)[:, :3].contiguous()
    g = torch.Generator(device=cloud.device)
    g.manual_seed(7)
    off = torch.rand(n, generator=g, device=cloud.device) < 0.2
    cloud[off, 2] = torch.rand(int(off.sum()), generator=g, device=cloud.device) * 1.5 - 0.5
    seg = pcl_amd.SACSegmentation(ctx)
    seg.setModelType(pcl_amd.SACMODEL_PLANE)
    seg.setMethodType(pcl_amd.SAC_RANSAC)
    seg.setDistanceThreshold(thr)
    seg.setProbability(1.0)
    seg.setMaxIterations(H - 1)
    seg.setBatchSize(H)
    seg.setOptimizeCoefficients(False)
    seg.setSeed(1)
    seg.setInputCloud(cloud)
    rows = []
    for _ in range(a.reps + 1):  # the first is the warm-up
        inl, coeff = seg.segment()
        torch.cuda.synchronize()
        s = seg.lastStats()
        rows.append((s["count_ms"], s["total_ms"]))
    assert s["trials"] == H and s["batches"] == 1 and s["skipped"] == 0, s
    count_ms, call_ms = sorted(rows[1:])[len(rows[1:]) // 2]
    trace = seg.trace()
    models = np.stack([t["coefficients"] for t in trace]).astype(np.float32)
    fused = np.array([t["count"] for t in trace], np.int64)
    # the composition
    M = torch.from_numpy(models[:, :3].copy()).to(cloud.device)
    d = torch.from_numpy(models[:, 3].copy()).to(cloud.device)

    def composed():
        cnt = torch.zeros(H, dtype=torch.int64, device=cloud.device)
        for b in range(0, n, CHUNK):
            cnt += ((cloud[b:b + CHUNK] @ M.T + d).abs() < thr).sum(0)
        return cnt
    times = []
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cnt = composed()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    torch_ms = sorted(times[1:])[len(times[1:]) // 2]
    base = cnt.cpu().numpy()
    prop = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(prop, "clock_rate", 2400000)) * 1e3
    peak_pairs = prop.multi_processor_count * 64.0 * clock_hz / SLOTS_PER_PAIR
    pairs = float(n) * H
    out = {"metric": "sac_timing", "points": n, "hypotheses": H, "threshold": thr,
           "best_count": int(s["best_count"]),
           "fused": {"count_kernel_ms": round(count_ms, 3), "segment_call_gpu_ms": round(call_ms, 3),
                     "pairs_per_s": round(pairs / (count_ms * 1e-3), 0)},
           "composition_torch_matmul": {"gpu_ms": round(torch_ms, 3), "pairs_per_s": round(pairs / (torch_ms * 1e-3), 0),
                                        "chunk_points": CHUNK},
           "counts_agree": bool((fused == base).all()), "counts_that_differ": int((fused != base).sum()),
           "largest_count_difference": int(np.abs(fused - base).max()),
           "speedup_count_kernel_vs_composition": round(torch_ms / count_ms, 2),
           "roofline": {"compute_units": int(prop.multi_processor_count), "clock_ghz": round(clock_hz * 1e-9, 3),
                        "issue_slots_per_pair": SLOTS_PER_PAIR, "peak_pairs_per_s": round(peak_pairs, 0),
                        "fraction": round(pairs / (count_ms * 1e-3) / peak_pairs, 3),
                        "bytes_read_per_pass": n * 16}}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sac_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
