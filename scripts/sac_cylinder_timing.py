"""Scoring-pass timing of SampleConsensusModelCylinder at 10M points x 1,024 hypotheses, beside the plane and the normal
plane of the same build: the scene of scripts/sac_models_timing.py (synth's Gaussian surface with analytic normals, a fifth
of the points uniform clutter) with every tenth point moved onto a cylinder of radius 0.2 standing on it, radial normals;
ndw 0.1.  Every figure is the median over the repeats of the GPU time of the scoring launch of a call that cannot stop early
(probability 1, max_iterations H - 1, batch_size H: one pass), read from the call's HIP events.

Each arm runs in a process of its own, under its own timeout, and the arms alternate, round after round:
  plane, normal         SACMODEL_PLANE and SACMODEL_NORMAL_PLANE through the segmentation classes, this build
  cylinder              RandomSampleConsensus over the cylinder: sac_cylinder_count_kernel
  cylinder_counted      the same built -DPCLHIP_SACC_STATS: the share of pairs that reach tier 2 (the exact function)
  cylinder_noscreen     built -DPCLHIP_SACC_NO_SCREEN: no tier 1, every pair takes the exact function
  refit                 optimizeModelCoefficients over 10^6 inliers of a noisy cylinder from a start 2 % off: wall time of the
                        call (device buffers) and the Levenberg-Marquardt steps it tried
The two extra builds are this script's own (scripts/build_variant.sh ... radius.hip, made here when they are missing).
spread = (max - min) / median of an arm's per-round medians.

Before anything is timed the cylinder arms check their flags: the 1,024 counts and gate bits of the call's trace against
pclhip_sac_cylinder_evaluate on the traced coefficients, and the length of the winner's inlier list against its count; the
driver then compares the three cylinder arms' counts (tier 1 must not change one).  Any difference: exit 1.
Writes profiles/sac_cylinder_timing.json (and prints it).

    python scripts/sac_cylinder_timing.py [n] [--hypotheses H] [--rounds R]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
VARIANTS = {"cylinder_counted": ("saccstats", "-DPCLHIP_SACC_STATS"),
            "cylinder_noscreen": ("saccnoscreen", "-DPCLHIP_SACC_NO_SCREEN")}
NDW = 0.1
RADIUS = 0.2


def scene(n, device):
    """sac_models_timing's scene with every tenth point on a vertical cylinder of radius 0.2 around (0.1, -0.2)"""
    import torch

    import sac_models_timing as smt
    cloud, normals = smt.scene(n, device)
    g = torch.Generator(device=device)
    g.manual_seed(11)
    k = cloud[::10].shape[0]
    phi = torch.rand(k, generator=g, device=device) * 6.283185307179586
    r = RADIUS + (torch.rand(k, generator=g, device=device) - 0.5) * 2e-3
    cloud[::10, 0] = 0.1 + r * torch.cos(phi)
    cloud[::10, 1] = -0.2 + r * torch.sin(phi)
    cloud[::10, 2] = torch.rand(k, generator=g, device=device)
    normals[::10, 0] = torch.cos(phi)
    normals[::10, 1] = torch.sin(phi)
    normals[::10, 2] = 0.0
    return cloud.contiguous(), normals.contiguous()


def refit_arm(a):
    import numpy as np
    import torch

    import pcl_amd
    m = 1_000_000 if a.n >= 1_000_000 else a.n
    rng = np.random.default_rng(3)
    axis = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    e1 = np.cross(axis, [1.0, 0, 0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(axis, e1)
    phi, h = rng.uniform(0, 2 * np.pi, m), rng.uniform(-1, 1, m)
    pts = h[:, None] * axis + (RADIUS + rng.uniform(-1e-3, 1e-3, m))[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    cloud = np.ascontiguousarray(pts, np.float32)
    inl = np.arange(m, dtype=np.int32)
    if a.device != "cpu":
        cloud, inl = torch.from_numpy(cloud).cuda(), torch.from_numpy(inl).cuda()
    model = pcl_amd.SampleConsensusModelCylinder(cloud, None, pcl_amd.Context(0))
    start = np.concatenate([[0.004, -0.003, 0.0], axis + [0.01, -0.01, 0.0], [RADIUS * 1.02]]).astype(np.float32)
    rows = []
    for _ in range(a.reps + 1):  # the first is the warm-up
        t0 = time.perf_counter()
        out = model.optimizeModelCoefficients(inl, start)
        rows.append((time.perf_counter() - t0) * 1e3)
    info = model.lastOptimize()
    ok = info["refined"] and abs(float(out[6]) - RADIUS) < 1e-4 and abs(abs(float(out[3:6] @ axis)) - 1.0) < 1e-5
    ms = sorted(rows[1:])[len(rows[1:]) // 2]
    print(json.dumps({"arm": "refit", "flags_agree": bool(ok), "count_ms": ms, "inliers": m, "lm_iterations": info["iterations"],
                      "radius": float(out[6])}))
    return 0 if ok else 1


def worker(a):
    import numpy as np
    import torch

    import sac_models_timing as smt
    arm = a.worker
    if arm == "refit":
        return refit_arm(a)
    device, n, H = a.device, a.n, a.hypotheses
    cloud, normals = scene(n, device)
    if device == "cpu":  # (the rehearsal on the emulation: host arrays)
        cloud, normals = cloud.numpy(), normals.numpy()
    import pcl_amd
    ctx = pcl_amd.Context(0)
    if arm in ("plane", "normal"):
        seg = pcl_amd.SACSegmentationFromNormals(ctx)
        seg.setModelType(0 if arm == "plane" else 11)
        seg.setInputNormals(normals)
        seg.setNormalDistanceWeight(NDW)
        seg.setMethodType(0)
        seg.setDistanceThreshold(a.threshold)
        seg.setOptimizeCoefficients(False)
        seg.setInputCloud(cloud)
        run, stats, trace = seg.segment, seg.lastStats, seg.trace
        evaluate = lambda models: seg.evaluate(models)  # noqa: E731
    else:
        model = pcl_amd.SampleConsensusModelCylinder(cloud, None, ctx)
        model.setInputNormals(normals)
        model.setNormalDistanceWeight(NDW)
        seg = pcl_amd.RandomSampleConsensus(model, a.threshold)
        run, stats, trace = seg.computeModel, seg.stats, seg.trace
        evaluate = lambda models: model.evaluate(models, a.threshold)  # noqa: E731
    seg.setProbability(1.0)
    seg.setMaxIterations(H - 1)
    seg.setBatchSize(H)
    seg.setSeed(1)
    take = getattr(ctx.lib, "pclhip_sacc_exact_pairs_take", None) if arm == "cylinder_counted" else None
    if arm == "cylinder_counted":
        assert take is not None, "the library was not built with -DPCLHIP_SACC_STATS"
        take.restype = C.c_ulonglong
        take.argtypes = []
    # ---- the flags, before any timing ----
    run()
    s = stats()
    assert s["trials"] == H and s["batches"] == 1, s
    tr = trace()
    counts = [t["count"] for t in tr]
    models = np.stack([t["coefficients"] for t in tr]).astype(np.float32)
    usable = np.isfinite(models).all(axis=1)  # (a NaN coefficient is not pinned bit for bit through a copy)
    ev, valid = evaluate(models)
    ok = s["n_inliers"] == s["best_count"] == max(counts)
    ok = ok and ev[usable].tolist() == np.array(counts)[usable].tolist()
    ok = ok and (valid & usable).tolist() == (np.array([t["valid"] for t in tr]) & usable).tolist()
    if not ok:
        print(json.dumps({"arm": arm, "flags_agree": False}))
        return 1
    exact = None
    if take is not None:
        take()
        run()
        exact = int(take())
    rows = []
    for _ in range(a.reps + 1):  # the first is the warm-up
        run()
        if device != "cpu":
            torch.cuda.synchronize()
        rows.append(stats()["count_ms"])
    ms = sorted(rows[1:])[len(rows[1:]) // 2]
    print(json.dumps({"arm": arm, "flags_agree": True, "count_ms": ms, "best_count": int(s["best_count"]),
                      "valid": int(sum(t["valid"] for t in tr)), "skipped": int(s["skipped"]), "exact_pairs": exact,
                      "counts_crc": smt.crc_of(counts)}))
    return 0


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    assert 1 <= a.hypotheses <= 1024
    if a.worker:
        return worker(a)
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    libs = {"plane": lib, "normal": lib, "cylinder": lib, "refit": lib}
    if "PCLHIP_LIB" not in os.environ:  # (a rehearsal on another library times that library alone)
        for arm, (name, flags) in VARIANTS.items():
            path = os.path.join(ROOT, "pcl_amd", "variants", "libpclhip_%s.so" % name)
            if not os.path.exists(path):
                subprocess.check_call(["bash", os.path.join(ROOT, "scripts", "build_variant.sh"), name, flags, "radius.hip"])
            libs[arm] = path
    order = [k for k in ("plane", "normal", "cylinder", "cylinder_counted", "cylinder_noscreen", "refit") if k in libs]
    runs = {k: [] for k in order}
    for r in range(a.rounds):
        for arm in order:
            if arm in VARIANTS and r > 0:  # (the comparison arms: one round)
                continue
            cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(a.n), "--hypotheses",
                   str(a.hypotheses), "--reps", str(a.reps), "--threshold", str(a.threshold), "--device", a.device, "--worker", arm]
            p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PCLHIP_LIB=libs[arm]))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line or not json.loads(line[-1])["flags_agree"]:
                print("arm %s failed its checks (exit %d): nothing more is started\n%s\n%s"
                      % (arm, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
                return 1
            runs[arm].append(json.loads(line[-1]))
            print("round %d %s: %s" % (r, arm, line[-1]), file=sys.stderr, flush=True)
    crc = {k: v[0]["counts_crc"] for k, v in runs.items() if k.startswith("cylinder")}
    if len(set(crc.values())) != 1:
        print("the cylinder arms' counts differ: %s" % crc)
        return 1

    def arm_summary(k):
        ms = sorted(v["count_ms"] for v in runs[k])
        med = ms[len(ms) // 2]
        return {"ms": round(med, 3), "rounds_ms": [round(v["count_ms"], 3) for v in runs[k]],
                "spread": round((ms[-1] - ms[0]) / med, 4) if len(ms) > 1 else None}
    pairs = float(a.n) * a.hypotheses
    c0 = runs["cylinder"][0]
    out = {"metric": "sac_cylinder_timing", "points": a.n, "hypotheses": a.hypotheses, "threshold": a.threshold,
           "normal_distance_weight": NDW, "rounds": a.rounds, "reps_per_round": a.reps, "best_count_cylinder": c0["best_count"],
           "valid_hypotheses": c0["valid"], "skipped": c0["skipped"], "arms": {k: arm_summary(k) for k in order},
           "refit_inliers": runs["refit"][0]["inliers"], "refit_lm_iterations": runs["refit"][0]["lm_iterations"],
           "flags_agree": True, "counts_identical_without_tier_1": "cylinder_noscreen" in runs}
    out["cylinder_over_plane"] = round(out["arms"]["cylinder"]["ms"] / out["arms"]["plane"]["ms"], 2)
    out["cylinder_over_normal"] = round(out["arms"]["cylinder"]["ms"] / out["arms"]["normal"]["ms"], 2)
    if "cylinder_counted" in runs:
        out["share_of_pairs_in_tier_2"] = runs["cylinder_counted"][0]["exact_pairs"] / pairs
        out["noscreen_over_screen"] = round(out["arms"]["cylinder_noscreen"]["ms"] / out["arms"]["cylinder"]["ms"], 2)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sac_cylinder_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
