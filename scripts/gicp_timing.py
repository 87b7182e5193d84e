"""GeneralizedIterativeClosestPoint timing: one JSON line with the covariance ms, ms per outer iteration, ms per Newton
pass (GPU time, HIP events) and Newton iterations per outer iteration, for synth.icp_pair at 1M and 10M points (default parameters; the second
align() of each size reuses the cached covariances and is the one timed for the loop).

    python scripts/gicp_timing.py [sizes...]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pcl_amd  # noqa: E402


def main():
    sizes = [int(s) for s in sys.argv[1:]] or [1_000_000, 10_000_000]
    ctx = pcl_amd.Context(0)
    out = {"metric": "gicp_timing"}
    for n in sizes:
        tgt, src, T_gt = pcl_amd.synth.icp_pair(n)
        reg = pcl_amd.GeneralizedIterativeClosestPoint(ctx)
        reg.setInputTarget(tgt)
        reg.setInputSource(src)
        reg.align()  # covariances + first (warm-up) alignment
        cov_ms = reg.result.covariance_ms
        t0 = time.perf_counter()
        reg.align()
        wall = (time.perf_counter() - t0) * 1e3
        r = reg.result
        loop_ms = r.total_ms
        host_ms = loop_ms - r.search_ms - r.pack_ms - r.eval_ms
        out[str(n)] = {
            "covariance_ms": round(cov_ms, 3),
            "outer_iterations": r.nr_iterations,
            "ms_per_outer_iteration": round(loop_ms / max(1, r.nr_iterations), 3),
            "search_ms": round(r.search_ms, 3),
            "pack_ms_per_outer_iteration": round(r.pack_ms / max(1, r.nr_iterations), 4),
            "newton_passes": r.eval_passes,
            # GPU time of one evaluation pass + its fixed-order reduction (HIP events around the two launches)
            "gpu_ms_per_newton_pass": round(r.eval_ms / max(1, r.eval_passes), 4),
            "newton_iterations_per_outer": round(r.newton_iterations / max(1, r.nr_iterations), 2),
            "line_searches_at_alpha_1": "%d/%d" % (r.newton_steps_alpha_one, r.newton_steps),
            "align_ms": round(loop_ms, 3),
            # what is not GPU time of search / pack / evaluation: copies, launches, the host's serial step and read-backs
            "other_ms": round(host_ms, 3),
            "other_ms_per_pass": round(host_ms / max(1, r.eval_passes + r.nr_iterations), 4),
            "wall_ms": round(wall, 3),
            "err_vs_ground_truth": float(np.abs(reg.getFinalTransformation().astype(np.float64) - T_gt).max()),
        }
        del reg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
