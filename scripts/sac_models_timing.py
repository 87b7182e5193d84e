"""Scoring-pass timing of the plane models of SACSegmentation at 10M points x 1,024 hypotheses: synth's Gaussian surface with
its analytic normals (a fifth of the points uniform clutter with random normals), ndw 0.1, a threshold that makes about a
third of the points inliers of the best plane.  Every figure is the median over the repeats of the GPU time of the scoring
launch of a segment() call that cannot stop early (probability 1, max_iterations H - 1, batch_size H: one pass), read from
the call's HIP events.

Each arm runs in a process of its own (a library is chosen when it is loaded), and the arms alternate, round after round:
  plane                 SACMODEL_PLANE through pclhip_sac_segment_plane, this build
  plane_parent          the same through the library of the parent commit (--parent-lib; left out without it)
  perpendicular, parallel   models 9 and 15 with gates nearly every hypothesis passes: sac_count_kernel behind the gate
  normal                SACMODEL_NORMAL_PLANE: sac_normal_count_kernel
  normal_counted        the same kernel built -DPCLHIP_SAC_SCREEN_STATS: the share of pairs that reached the double acos
  normal_noscreen       built -DPCLHIP_SAC_NO_SCREEN: every pair takes the double acos
The two extra builds are this script's own (scripts/build_variant.sh ... radius.hip, made here when they are missing); the
library that ships has neither switch.  spread = (max - min) / median of an arm's per-round medians: the run-to-run noise
that a difference between two arms has to exceed.

Before anything is timed every arm checks its flags: the 1,024 counts of the call's trace against
pclhip_sac_model_evaluate on the traced coefficients, and the length of the winner's inlier list against its count; the
driver then compares the normal arms' counts with each other (the screen must not change one).  Any difference: exit 1.
Writes profiles/sac_models_timing.json (and prints it).

    python scripts/sac_models_timing.py [n] [--hypotheses H] [--rounds R] [--parent-lib PATH]
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = {"normal_counted": ("sacstats", "-DPCLHIP_SAC_SCREEN_STATS"),
            "normal_noscreen": ("sacnoscreen", "-DPCLHIP_SAC_NO_SCREEN")}
NDW = 0.1


def scene(n, device):
    """(cloud (n, 3), normals (n, 4)) float32 tensors on `device`"""
    import torch

    from pcl_amd import synth
    cloud = synth.gaussian_surface_device(n, device=device)[:, :3].contiguous()
    x, y = cloud[:, 0].double(), cloud[:, 1].double()
    sx, sy = torch.zeros_like(x), torch.zeros_like(x)
    for cx, cy, s, a in synth._BUMPS:
        e = float(a) * torch.exp(-((x - float(cx)) ** 2 + (y - float(cy)) ** 2) / (2.0 * float(s) * float(s)))
        sx -= e * (x - float(cx)) / (float(s) * float(s))
        sy -= e * (y - float(cy)) / (float(s) * float(s))
    nrm = torch.stack([-sx, -sy, torch.ones_like(sx)], 1)
    nrm = (nrm / nrm.norm(dim=1, keepdim=True)).float()
    g = torch.Generator(device=device)
    g.manual_seed(7)
    off = torch.rand(n, generator=g, device=device) < 0.2
    k = int(off.sum())
    cloud[off, 2] = torch.rand(k, generator=g, device=device) * 1.5 - 0.5
    rnd = torch.randn(k, 3, generator=g, device=device)
    nrm[off] = rnd / rnd.norm(dim=1, keepdim=True)
    curv = torch.rand(n, generator=g, device=device) * 0.05
    return cloud, torch.cat([nrm, curv[:, None]], 1).contiguous()


def plane_arm(a, cloud, n):
    """the plane through pclhip_sac_segment_plane and nothing newer: the same calls on this build and on the parent's"""
    import numpy as np

    from pcl_amd import _lib
    lib = C.CDLL(os.environ["PCLHIP_LIB"])
    for name in ("pclhip_ctx_create", "pclhip_sac_plane_params_default", "pclhip_sac_segment_plane", "pclhip_sac_plane_evaluate",
                 "pclhip_sac_last_trace"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    h = C.c_void_p()
    assert lib.pclhip_ctx_create(0, None, C.byref(h)) == 0
    H = a.hypotheses
    p = _lib.SacPlaneParams()
    lib.pclhip_sac_plane_params_default(C.byref(p))
    p.distance_threshold, p.max_iterations, p.probability, p.optimize_coefficients, p.seed, p.batch_size = \
        a.threshold, H - 1, 1.0, 0, 1, H
    ptr = C.c_void_p(cloud.ctypes.data if isinstance(cloud, np.ndarray) else cloud.data_ptr())
    coeff = np.zeros(4, np.float32)
    n_in, n_out = C.c_uint64(0), C.c_uint64(0)
    st = _lib.SacPlaneStats()

    def segment():
        rc = lib.pclhip_sac_segment_plane(h, ptr, n, 12, None, 0, C.byref(p), coeff.ctypes.data_as(C.POINTER(C.c_float)), None, 0,
                                          C.byref(n_in), None, 0, C.byref(n_out), C.byref(st))
        assert rc == 0 and st.trials == H and st.batches == 1, (rc, st.trials, st.batches)
        return float(st.count_ms)
    segment()
    buf = (_lib.SacPlaneTrace * H)()
    cnt = C.c_uint64(0)
    assert lib.pclhip_sac_last_trace(h, buf, H, C.byref(cnt)) == 0 and cnt.value == H
    counts = [int(t.count) for t in buf]
    models = np.array([list(t.coefficients) for t in buf], np.float32)
    ev = np.zeros(H, np.uint32)
    assert lib.pclhip_sac_plane_evaluate(h, ptr, n, 12, None, 0, a.threshold, models.ctypes.data_as(C.POINTER(C.c_float)), H,
                                         C.c_void_p(ev.ctypes.data)) == 0
    if not (ev.tolist() == counts and n_in.value == st.best_count == max(counts)):
        print(json.dumps({"arm": a.worker, "flags_agree": False}))
        return 1
    rows = [segment() for _ in range(a.reps + 1)]  # the first is the warm-up
    ms = sorted(rows[1:])[len(rows[1:]) // 2]
    print(json.dumps({"arm": a.worker, "flags_agree": True, "count_ms": ms, "best_count": int(st.best_count), "valid": H,
                      "exact_pairs": None, "counts_crc": crc_of(counts)}))
    return 0


def crc_of(counts):
    import numpy as np
    return int(np.bitwise_xor.reduce(np.array(counts, np.int64) * (np.arange(len(counts)) + 1)))


def worker(a):
    import numpy as np
    import torch
    device = a.device
    n, H = a.n, a.hypotheses
    cloud, normals = scene(n, device)
    if device == "cpu":  # (the rehearsal on the emulation: host arrays)
        cloud, normals = cloud.numpy(), normals.numpy()
    arm = a.worker
    if arm in ("plane", "plane_parent"):
        return plane_arm(a, cloud, n)
    import pcl_amd
    ctx = pcl_amd.Context(0)
    arm = a.worker
    if arm == "perpendicular":
        seg = pcl_amd.SACSegmentation(ctx)
        seg.setModelType(9)
        seg.setAxis((0, 0, 1))
        seg.setEpsAngle(1.5707)
    elif arm == "parallel":
        seg = pcl_amd.SACSegmentation(ctx)
        seg.setModelType(15)
        seg.setAxis((1, 0, 0))
        seg.setEpsAngle(1.5707)
    else:
        seg = pcl_amd.SACSegmentationFromNormals(ctx)
        seg.setModelType(11)
        seg.setInputNormals(normals)
        seg.setNormalDistanceWeight(NDW)
    seg.setMethodType(0)
    seg.setDistanceThreshold(a.threshold)
    seg.setProbability(1.0)
    seg.setMaxIterations(H - 1)
    seg.setBatchSize(H)
    seg.setOptimizeCoefficients(False)
    seg.setSeed(1)
    seg.setInputCloud(cloud)
    take = getattr(ctx.lib, "pclhip_sac_exact_pairs_take", None) if arm == "normal_counted" else None
    if arm == "normal_counted":
        assert take is not None, "the library was not built with -DPCLHIP_SAC_SCREEN_STATS"
        take.restype = C.c_ulonglong
        take.argtypes = []
    # ---- the flags, before any timing ----
    inl, coeff = seg.segment()
    s = seg.lastStats()
    assert s["trials"] == H and s["batches"] == 1, s
    trace = seg.trace()
    counts = [t["count"] for t in trace]
    models = np.stack([t["coefficients"] for t in trace]).astype(np.float32)
    ev, valid = seg.evaluate(models)
    ok = len(inl) == s["best_count"] == max(counts) and ev.tolist() == counts and valid.tolist() == [t["valid"] for t in trace]
    if not ok:
        print(json.dumps({"arm": arm, "flags_agree": False}))
        return 1
    exact = None
    if take is not None:
        take()
        seg.segment()
        exact = int(take())
    rows = []
    for _ in range(a.reps + 1):  # the first is the warm-up
        seg.segment()
        if device != "cpu":
            torch.cuda.synchronize()
        st = seg.lastStats()
        rows.append(st["count_ms"])
    ms = sorted(rows[1:])[len(rows[1:]) // 2]
    print(json.dumps({"arm": arm, "flags_agree": True, "count_ms": ms, "best_count": int(s["best_count"]),
                      "valid": int(sum(t["valid"] for t in trace)), "exact_pairs": exact,
                      "counts_crc": crc_of(counts)}))
    return 0


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    assert 1 <= a.hypotheses <= 1024
    if a.worker:
        return worker(a)
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    libs = {"plane": lib, "perpendicular": lib, "parallel": lib, "normal": lib}
    if a.parent_lib:
        libs["plane_parent"] = os.path.abspath(a.parent_lib)
    if "PCLHIP_LIB" not in os.environ:  # (a rehearsal on another library times that library alone)
        for arm, (name, flags) in VARIANTS.items():
            path = os.path.join(ROOT, "pcl_amd", "variants", "libpclhip_%s.so" % name)
            if not os.path.exists(path):
                subprocess.check_call(["bash", os.path.join(ROOT, "scripts", "build_variant.sh"), name, flags, "radius.hip"])
            libs[arm] = path
    order = [k for k in ("plane", "plane_parent", "perpendicular", "parallel", "normal", "normal_counted", "normal_noscreen")
             if k in libs]
    runs = {k: [] for k in order}
    for r in range(a.rounds):
        for arm in order:
            if arm in VARIANTS and r > 0:  # (the comparison arms: one round)
                continue
            cmd = [sys.executable, os.path.abspath(__file__), str(a.n), "--hypotheses", str(a.hypotheses), "--reps", str(a.reps),
                   "--threshold", str(a.threshold), "--device", a.device, "--worker", arm]
            p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PCLHIP_LIB=libs[arm]), timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line or not json.loads(line[-1])["flags_agree"]:
                print("arm %s failed its checks (exit %d)\n%s\n%s" % (arm, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
                return 1
            runs[arm].append(json.loads(line[-1]))
            print("round %d %s: %s" % (r, arm, line[-1]), file=sys.stderr, flush=True)
    crc = {k: v[0]["counts_crc"] for k, v in runs.items()}
    if len({crc[k] for k in crc if k.startswith("normal")}) != 1 or len({crc[k] for k in crc if k.startswith("plane")}) != 1:
        print("the arms' counts differ: %s" % crc)
        return 1

    def arm_summary(k):
        ms = sorted(v["count_ms"] for v in runs[k])
        med = ms[len(ms) // 2]
        return {"count_kernel_ms": round(med, 3), "rounds_ms": [round(v["count_ms"], 3) for v in runs[k]],
                "spread": round((ms[-1] - ms[0]) / med, 4) if len(ms) > 1 else None}
    pairs = float(a.n) * a.hypotheses
    out = {"metric": "sac_models_timing", "points": a.n, "hypotheses": a.hypotheses, "threshold": a.threshold,
           "normal_distance_weight": NDW, "rounds": a.rounds, "reps_per_round": a.reps,
           "best_count_plane": runs["plane"][0]["best_count"], "best_count_normal": runs["normal"][0]["best_count"],
           "inlier_share_of_the_best_normal_plane": round(runs["normal"][0]["best_count"] / float(a.n), 3),
           "valid_hypotheses": {k: runs[k][0]["valid"] for k in ("perpendicular", "parallel")},
           "arms": {k: arm_summary(k) for k in order}, "flags_agree": True}
    plane = out["arms"]["plane"]["count_kernel_ms"]
    out["normal_over_plane"] = round(out["arms"]["normal"]["count_kernel_ms"] / plane, 2)
    for k in ("perpendicular", "parallel", "plane_parent"):
        if k in out["arms"]:
            out[k + "_over_plane"] = round(out["arms"][k]["count_kernel_ms"] / plane, 4)
    if "normal_counted" in runs:
        out["share_of_pairs_on_the_double_path"] = runs["normal_counted"][0]["exact_pairs"] / pairs
        out["noscreen_over_screen"] = round(out["arms"]["normal_noscreen"]["count_kernel_ms"] /
                                            out["arms"]["normal"]["count_kernel_ms"], 2)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sac_models_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
