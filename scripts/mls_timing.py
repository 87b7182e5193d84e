"""MovingLeastSquares timing at 10M points: synth.gaussian_surface, search radius 0.001954 (the radius of scripts/fpfh_timing.py
and scripts/iss_timing.py: 26.2 neighbours per point), order 2, the SIMPLE projection, normals on.  Records, in one run, the GPU
time of pclhip_mls_process (whole call, and its two kernels) and the time of the same outputs composed from what the library
offered before it: pclhip_radius_search of the cloud against itself into device memory, then the centroid and covariance
sums, a batched torch.linalg.eigh, the weighted normal equations and torch.cholesky_solve in float64 on the device, chunked
to fit memory.  The baseline is that composition; counts and indices must be equal and the points must agree within the
bound of tests/mls_restatement.py, (m + 32) * 2^-53 * kappa * r + far_point_term, outside its excluded records.  Writes
profiles/mls_timing.json (and prints it).

    python scripts/mls_timing.py [n] [--radius R] [--compare-lib OTHER/libpclhip.so]

With --compare-lib the fused step also runs with PCLHIP_LIB set to that library, three rounds in alternation with this
build, each a process of its own: "fit_pass_ab" holds both builds' pass times per round, medians and spreads.

Each GPU step runs as a child process under its own `timeout`; the first failure ends the run.  A comparison that misses
(counts, indices, m, or a difference beyond the bound) does not: its figures are written with "ok": false and the script
exits 1.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STEP_TIMEOUT_S = {"fused": 240, "composition": 900}
AB_ROUNDS = 3                  # --compare-lib: alternating rounds per build
PEAK_BYTES_PER_S = 8.0e12      # HBM3E of the MI355X
PEAK_FP64_FLOPS = 78.6e12      # vector fp64 of AMD's specification
U = 2.0 ** -53
ALLOWANCE = 32                 # tests/mls_restatement.py: SOLVER_ALLOWANCE
# fp64 operations per pair, counted from pcl_amd/csrc/mls.hpp (an fma is 2): the plane walk widens and subtracts (3), adds
# the three sums (3) and six fmas (12); the fit walk subtracts twice (6: the query, then mean - q), d.d (5) and the scale (1), three dot products (15), ten
# products (10), ten adds and five fmas of the u, v moments (20), one add and five fmas and three products of the f moments
# (14) -- and one exp
FLOPS_PLANE_PER_PAIR = 18
FLOPS_FIT_PER_PAIR = 71


def setup(n):
    import torch

    import pcl_amd
    ctx = pcl_amd.Context(0)
    q = torch.from_numpy(pcl_amd.synth.gaussian_surface(n)[:, :3].copy()).cuda()
    tree = pcl_amd.KdTree(ctx)
    tree.setInputCloud(q)
    torch.cuda.synchronize()
    return torch, pcl_amd, ctx, q, tree, {"index_build_ms": round(tree.build_ms(), 3)}


def smoother(pcl_amd, ctx, q, tree, r):
    s = pcl_amd.MovingLeastSquares(ctx)
    s.setInputCloud(q)
    s.setSearchMethod(tree)
    s.setSearchRadius(r)
    s.setPolynomialOrder(2)
    s.setComputeNormals(True)
    return s


def step_fused(n, r, reps=5):
    torch, pcl_amd, ctx, q, tree, out = setup(n)
    s = smoother(pcl_amd, ctx, q, tree, r)
    rows = []
    for _ in range(reps + 1):  # the first is the warm-up
        pts, nrm, curv, idx = s.process()
        torch.cuda.synchronize()
        rows.append((s.lastKernelMs(),) + s.lastPassMs())
    rows = sorted(rows[1:])
    call, plane_ms, fit_ms = rows[len(rows) // 2]
    out["fused"] = {"call_gpu_ms": round(call, 3), "plane_ms": round(plane_ms, 3), "fit_ms": round(fit_ms, 3),
                    "records": int(len(idx)), "checksum": int(idx.long().sum())}
    return out


def neighbour_lists(torch, np, pcl_amd, ctx, tree, q, radius):
    """pclhip_radius_search of the cloud against itself into device memory -> offsets (device int64), idx, call ms"""
    lib = ctx.lib
    n = len(q)
    qp, stride = C.c_void_p(q.data_ptr()), q.shape[1] * 4
    offsets = np.zeros(n + 1, np.uint64)
    optr = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    total = C.c_uint64(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = lib.pclhip_radius_search(tree.h, qp, stride, n, float(radius), 0, optr, None, None, 0, C.byref(total))
    assert st in (0, -5), st
    m = int(total.value)
    idx = torch.empty(m, dtype=torch.int32, device=q.device)
    d2 = torch.empty(m, dtype=torch.float32, device=q.device)
    e0.record()
    pcl_amd._lib.check(lib.pclhip_radius_search(tree.h, qp, stride, n, float(radius), 0, optr, C.c_void_p(idx.data_ptr()),
                                               C.c_void_p(d2.data_ptr()), m, C.byref(total)), ctx.h)
    e1.record()
    torch.cuda.synchronize()
    del d2
    return torch.from_numpy(offsets.astype(np.int64)).to(q.device), idx, e0.elapsed_time(e1)


def step_composition(n, r):
    import numpy as np
    torch, pcl_amd, ctx, q, tree, out = setup(n)
    dev = q.device
    # the code under test, for the comparison only
    s = smoother(pcl_amd, ctx, q, tree, r)
    _, _, _, d_idx, d_dbl = s.processAll()
    torch.cuda.synchronize()

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    off, idx, search_ms = neighbour_lists(torch, np, pcl_amd, ctx, tree, q, r)
    pairs = int(off[-1])
    t0.record()
    m = off[1:] - off[:-1]
    q64 = q.double()
    point = torch.empty((n, 3), dtype=torch.float64, device=dev)
    normal = torch.empty((n, 3), dtype=torch.float64, device=dev)
    curv = torch.empty(n, dtype=torch.float64, device=dev)
    gap = torch.empty(n, dtype=torch.float64, device=dev)
    fitted = torch.zeros(n, dtype=torch.bool, device=dev)
    system = torch.zeros((n, 21), dtype=torch.float64, device=dev)  # the lower triangle of the fit matrix, for kappa
    tri = torch.tril_indices(6, 6, device=dev)
    step = 1 << 18
    for a in range(0, n, step):
        b = min(n, a + step)
        k = b - a
        lo, hi = int(off[a]), int(off[b])
        cnt = m[a:b]
        src = torch.repeat_interleave(torch.arange(k, device=dev), cnt)
        p = q64[idx[lo:hi].long()]
        mm = cnt.double().clamp(min=1).unsqueeze(1)
        c = torch.zeros((k, 3), dtype=torch.float64, device=dev).index_add_(0, src, p) / mm
        d = p - c[src]
        cov = torch.zeros((k, 9), dtype=torch.float64, device=dev).index_add_(
            0, src, (d.unsqueeze(2) * d.unsqueeze(1)).reshape(-1, 9)).view(k, 3, 3)
        w, V = torch.linalg.eigh(cov)
        nn = V[:, :, 0]
        lead = nn.gather(1, nn.abs().argmax(dim=1, keepdim=True))
        nn = torch.where(lead < 0, -nn, nn)
        trace = cov.diagonal(dim1=1, dim2=2).sum(dim=1)
        qq = q64[a:b]
        mean = qq - ((qq - c) * nn).sum(dim=1, keepdim=True) * nn
        curv[a:b] = torch.where(trace != 0, (w[:, 0] / trace).abs(), torch.zeros_like(trace))
        gap[a:b] = torch.where(trace > 0, (w[:, 1] - w[:, 0]) / trace, torch.zeros_like(trace))
        # Eigen's unitOrthogonal, u = n x v
        first = ~((nn[:, 0].abs() <= nn[:, 2].abs() * 1e-12) & (nn[:, 1].abs() <= nn[:, 2].abs() * 1e-12))
        z = torch.zeros_like(nn[:, 0])
        v1 = torch.stack([-nn[:, 1], nn[:, 0], z], dim=1) / torch.sqrt(nn[:, 0] ** 2 + nn[:, 1] ** 2).unsqueeze(1)
        v2 = torch.stack([z, -nn[:, 2], nn[:, 1]], dim=1) / torch.sqrt(nn[:, 1] ** 2 + nn[:, 2] ** 2).unsqueeze(1)
        vv = torch.where(first.unsqueeze(1), v1, v2)
        uu = torch.linalg.cross(nn, vv)
        dm = p - mean[src]
        wt = torch.exp(-(dm * dm).sum(dim=1) / (r * r))
        uj, vj, fj = (dm * uu[src]).sum(dim=1), (dm * vv[src]).sum(dim=1), (dm * nn[src]).sum(dim=1)
        P = torch.stack([torch.ones_like(uj), vj, vj * vj, uj, uj * vj, uj * uj], dim=1)
        Pw = P * wt.unsqueeze(1)
        A = torch.zeros((k, 36), dtype=torch.float64, device=dev).index_add_(
            0, src, (Pw.unsqueeze(2) * P.unsqueeze(1)).reshape(-1, 36)).view(k, 6, 6)
        rhs = torch.zeros((k, 6), dtype=torch.float64, device=dev).index_add_(0, src, Pw * fj.unsqueeze(1))
        del P, Pw, dm, d, p
        want = cnt >= 6
        eye = torch.eye(6, dtype=torch.float64, device=dev)
        L, info = torch.linalg.cholesky_ex(torch.where(want.view(-1, 1, 1), A, eye))
        coeff = torch.cholesky_solve(rhs.unsqueeze(2), torch.where((info == 0).view(-1, 1, 1), L, eye)).squeeze(2)
        ok = want & (info == 0) & torch.isfinite(coeff[:, 0])
        o = nn - coeff[:, 3:4] * uu - coeff[:, 1:2] * vv
        o = o / o.norm(dim=1, keepdim=True)
        point[a:b] = torch.where(ok.unsqueeze(1), mean + coeff[:, 0:1] * nn, mean)
        normal[a:b] = torch.where(ok.unsqueeze(1), o, nn)
        fitted[a:b] = ok
        system[a:b] = A[:, tri[0], tri[1]]
    keep = m >= 3
    c_idx = torch.nonzero(keep).squeeze(1)
    t1.record()
    torch.cuda.synchronize()
    torch_ms = t0.elapsed_time(t1)
    del idx
    # the comparison: kappa = max(1, 1 / gap, cond of the fit matrix with u, v in units of r) -- outside the timed region
    cond = torch.ones(n, dtype=torch.float64, device=dev)
    scale = torch.tensor([1.0, 1 / r, 1 / r ** 2, 1 / r, 1 / r ** 2, 1 / r ** 2], dtype=torch.float64, device=dev)
    for a in range(0, n, 1 << 20):
        b = min(n, a + (1 << 20))
        A = torch.zeros((b - a, 6, 6), dtype=torch.float64, device=dev)
        A[:, tri[0], tri[1]] = system[a:b]
        A = A + A.transpose(1, 2) - torch.diag_embed(A.diagonal(dim1=1, dim2=2))
        A = A * scale.view(1, 6, 1) * scale.view(1, 1, 6)
        f = fitted[a:b]
        A = torch.where(f.view(-1, 1, 1), A, torch.eye(6, dtype=torch.float64, device=dev))
        ev = torch.linalg.eigvalsh(A)
        cond[a:b] = torch.where(f, ev[:, 5] / ev[:, 0].clamp(min=1e-300), torch.ones_like(ev[:, 0]))
    kappa = torch.maximum(torch.ones_like(gap), torch.maximum(1.0 / gap, cond))
    bound_unit = (m.double() + ALLOWANCE) * U * kappa
    excluded = ~(bound_unit <= 1e-3)
    same_count = int(len(c_idx)) == int(len(d_idx)) and bool((c_idx == d_idx.long()).all())
    cmp = {"records_device": int(len(d_idx)), "records_composition": int(len(c_idx)), "indices_equal": same_count}
    if same_count:
        rows = c_idx
        live = ~excluded[rows]
        dp = (d_dbl[:, :3] - point[rows]).abs().amax(dim=1)
        dn = torch.minimum((d_dbl[:, 3:6] - normal[rows]).abs().amax(dim=1), (d_dbl[:, 3:6] + normal[rows]).abs().amax(dim=1))
        dc = (d_dbl[:, 6] - curv[rows]).abs()
        bu = bound_unit[rows]
        # the point's bound carries tests/mls_restatement.py's far_point_term, 2 * 2^-53 * max_i |q_i|: the rounding of the
        # final q + offset, once per implementation
        far = 2.0 * U * q64[rows].abs().amax(dim=1)
        bp = bu * r + far
        cmp.update({"excluded": int((~live).sum()), "fitted": int(fitted[rows].sum()),
                    "m_equal": bool((d_dbl[:, 7] == m[rows].double()).all()),
                    "worst_point_over_bound": float((dp / bp)[live].max()),
                    "worst_point_over_bound_without_the_point_term": float((dp / (bu * r))[live].max()),
                    "worst_normal_over_bound": float((dn / bu)[live].max()),
                    "worst_curvature_over_bound": float((dc / bu)[live].max()),
                    "largest_point_difference": float(dp[live].max())})
        # for the record: the same differences in units of 2^-53 times the point's largest coordinate, one rounding of a double
        # at the point, and how many points the bound without the point term would have missed
        one = U * point[rows].abs().amax(dim=1)
        late = dp / bp > 1.0
        bare = dp / (bu * r) > 1.0
        cmp.update({"largest_point_difference_in_roundings_at_the_point": float((dp / one)[live].max()),
                    "points_beyond_the_bound": int((late & live).sum()),
                    "points_beyond_the_bound_without_the_point_term": int((bare & live).sum()),
                    "largest_bound_over_rounding_among_them": float((bp / one)[late & live].max()) if bool((late & live).any()) else None,
                    "median_point_bound": float((bu * r)[live].median()),
                    "largest_coordinate": float(point[rows].abs().max())})
    out["neighbours_per_point"] = round((pairs - n) / n, 3)
    out["pairs"] = pairs
    out["pairs_of_fitted_points"] = int(m[fitted].sum())
    out["composition_radius_search_torch"] = {"gpu_ms": round(search_ms + torch_ms, 3), "radius_search_call_ms": round(search_ms, 3),
                                              "torch_ms": round(torch_ms, 3), "radius_search_output_bytes": pairs * 8}
    out["comparison"] = cmp
    # counts equal, points within the bound: checked by main() after the step's figures are on disk
    cmp["ok"] = bool(same_count and cmp["m_equal"] and cmp["excluded"] <= 0.01 * cmp["records_device"] and
                     max(cmp["worst_point_over_bound"], cmp["worst_normal_over_bound"], cmp["worst_curvature_over_bound"]) <= 1.0)
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--radius", type=float, default=0.001954, help="the search radius")
    ap.add_argument("--step", choices=tuple(STEP_TIMEOUT_S), default=None, help="run one step in this process")
    ap.add_argument("--out", default=None, help="with --step: where the step's JSON goes")
    ap.add_argument("--compare-lib", default=None, help="another build of the library (say, the parent commit's): its fused "
                    "step runs in alternation with this build's and both builds' pass times are recorded")
    ap.add_argument("--compare-label", default="parent commit", help="what --compare-lib is, for the record")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "mls_timing.json"), help="where the result goes")
    a = ap.parse_args()
    n, r = a.n, a.radius
    if a.step is not None:
        res = {"fused": lambda: step_fused(n, r), "composition": lambda: step_composition(n, r)}[a.step]()
        text = json.dumps(res)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        if not res.get("comparison", {"ok": True})["ok"]:
            print("the composition and the device disagree: %s" % res["comparison"], file=sys.stderr)
            return 1
        return 0
    out = {"metric": "mls_timing", "points": n, "cloud": "synth.gaussian_surface", "search_radius": r, "sqr_gauss_param": r * r,
           "polynomial_order": 2, "projection_method": "SIMPLE"}
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for step in STEP_TIMEOUT_S:
            piece = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), str(n),
                   "--radius", repr(r), "--step", step, "--out", piece]
            rc = subprocess.call(cmd)
            if rc != 0 and not (rc == 1 and os.path.exists(piece)):  # (1 with its figures written: the comparison failed)
                print("step %s failed with status %d: stopping" % (step, rc), file=sys.stderr)
                return rc
            status = status or rc
            with open(piece) as f:
                out.update(json.load(f))
        if a.compare_lib:  # the fused step of both builds in alternation, a process each: medians of five calls per round
            arms = (("this_build", None), ("other_build", os.path.abspath(a.compare_lib)))
            rounds = {arm: [] for arm, _ in arms}
            for rnd in range(AB_ROUNDS):
                for arm, lib in arms:
                    piece = os.path.join(tmp, "%s_%d.json" % (arm, rnd))
                    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S["fused"]), sys.executable, os.path.abspath(__file__), str(n),
                           "--radius", repr(r), "--step", "fused", "--out", piece]
                    rc = subprocess.call(cmd, env=dict(os.environ, PCLHIP_LIB=lib) if lib else None)
                    if rc != 0:
                        print("A/B round %d of %s failed with status %d: stopping" % (rnd, arm, rc), file=sys.stderr)
                        return rc
                    with open(piece) as f:
                        rounds[arm].append(json.load(f)["fused"])
            ab = {"rounds": AB_ROUNDS, "other_build": a.compare_label}
            for arm, _ in arms:
                for key in ("fit_ms", "plane_ms", "call_gpu_ms"):
                    vals = sorted(x[key] for x in rounds[arm])
                    ab["%s_%s" % (arm, key)] = {"per_round": [x[key] for x in rounds[arm]], "median": vals[len(vals) // 2],
                                                "spread": round((vals[-1] - vals[0]) / vals[len(vals) // 2], 4)}
            ab["same_records"] = len({(x["records"], x["checksum"]) for arm, _ in arms for x in rounds[arm]}) == 1
            ab["fit_ms_this_over_other"] = round(ab["this_build_fit_ms"]["median"] / ab["other_build_fit_ms"]["median"], 4)
            out["fit_pass_ab"] = ab
    fused, comp = out["fused"], out["composition_radius_search_torch"]
    out["speedup_call_vs_composition"] = round(comp["gpu_ms"] / fused["call_gpu_ms"], 2)
    out["pairs_per_second_plane"] = round(out["pairs"] / (fused["plane_ms"] * 1e-3), 0)
    out["pairs_per_second_fit"] = round(out["pairs_of_fitted_points"] / (fused["fit_ms"] * 1e-3), 0) if fused["fit_ms"] > 0 else None
    # algorithmic bytes: 16 B of point per pair per pass against 8 TB/s; the fp64 operations per pair counted from the code
    for name, pairs, flops, key in (("plane", out["pairs"], FLOPS_PLANE_PER_PAIR, "plane_ms"),
                                    ("fit", out["pairs_of_fitted_points"], FLOPS_FIT_PER_PAIR, "fit_ms")):
        nbytes = 16 * pairs
        at_bw, at_fp = nbytes / PEAK_BYTES_PER_S * 1e3, flops * pairs / PEAK_FP64_FLOPS * 1e3
        out["roofline_" + name] = {"algorithmic_bytes": nbytes, "ms_at_8TBps": round(at_bw, 4), "fp64_flops_per_pair": flops,
                                   "fp64_flops": flops * pairs, "ms_at_fp64_peak": round(at_fp, 4),
                                   "fraction_of_the_roof": round(max(at_bw, at_fp) / fused[key], 4) if fused[key] > 0 else None}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(text + "\n")
    return status  # 1: the figures are written, the device and the composition are further apart than the bound allows


if __name__ == "__main__":
    sys.exit(main())
