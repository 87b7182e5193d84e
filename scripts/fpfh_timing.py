"""FPFHEstimation timing at 10M points: synth.gaussian_surface, k = 8 normals, a radius chosen for about 30 neighbours per
point.  Records, in one run, the neighbour count, the GPU time of pclhip_fpfh (whole call, and its two kernels), and the
time of the same descriptors composed from what the library offered before it: pclhip_radius_search of the cloud against
itself into device memory, then the pair features, histograms and weighting in torch on the device.  The baseline is that
composition.  Writes profiles/fpfh_timing.json (and prints it).

    python scripts/fpfh_timing.py [n] [--radius R]

Each GPU step (fused, composition) runs as a child process under its own `timeout`; the first failure ends the run.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_TIMEOUT_S = {"fused": 240, "composition": 420}
PEAK_BYTES_PER_S = 8.0e12  # HBM3E of the MI355X


def setup(n, radius):
    import torch

    import pcl_amd
    ctx = pcl_amd.Context(0)
    q = torch.from_numpy(pcl_amd.synth.gaussian_surface(n)[:, :3].copy()).cuda()
    tree = pcl_amd.KdTree(ctx)
    tree.setInputCloud(q)
    ne = pcl_amd.NormalEstimation(ctx)
    ne.setInputCloud(q)
    ne.setSearchMethod(tree)
    ne.setKSearch(8)
    nrm = ne.compute()
    torch.cuda.synchronize()
    return torch, pcl_amd, ctx, q, tree, nrm, {"index_build_ms": round(tree.build_ms(), 3), "normals_k8_ms": round(tree.lastKernelMs(), 3)}


def step_fused(n, radius, reps=5):
    torch, pcl_amd, ctx, q, tree, nrm, out = setup(n, radius)
    f = pcl_amd.FPFHEstimation(ctx)
    f.setInputCloud(q)
    f.setSearchMethod(tree)  # the normals the tree holds
    f.setRadiusSearch(radius)
    rows = []
    for _ in range(reps + 1):  # the first is the warm-up
        fp = f.compute()
        torch.cuda.synchronize()
        rows.append((tree.lastKernelMs(),) + f.lastPassMs())
    rows = sorted(rows[1:])
    call, spfh_ms, weight_ms = rows[len(rows) // 2]
    out["fused"] = {"call_gpu_ms": round(call, 3), "fpfh_spfh_kernel_ms": round(spfh_ms, 3),
                    "fpfh_weight_kernel_ms": round(weight_ms, 3), "nan_rows": int(f.nan_count),
                    "checksum": float(torch.nan_to_num(fp).double().sum())}
    return out


def pair_features(torch, p1, n1, p2, n2):
    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def cross(a, b):
        return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                            a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=1)
    d = p2 - p1
    f4 = torch.sqrt(dot(d, d))
    a1, a2 = dot(n1, d) / f4, dot(n2, d) / f4
    swap = torch.acos(a1.abs()) > torch.acos(a2.abs())
    u = torch.where(swap[:, None], n2, n1)
    t = torch.where(swap[:, None], n1, n2)
    d = torch.where(swap[:, None], -d, d)
    f3 = torch.where(swap, -a2, a1)
    v = cross(d, u)
    vn = torch.sqrt(dot(v, v))
    v = v / vn[:, None]
    w = cross(u, v)
    f2 = dot(v, t)
    f1 = torch.atan2(dot(w, t), dot(u, t))
    deg = (f4 == 0) | (vn == 0)
    z = torch.zeros_like(f1)
    return torch.where(deg, z, f1), torch.where(deg, z, f2), torch.where(deg, z, f3)


def step_composition(n, radius):
    import numpy as np
    torch, pcl_amd, ctx, q, tree, nrm, out = setup(n, radius)
    lib = ctx.lib
    dev = q.device
    qp, stride = C.c_void_p(q.data_ptr()), q.shape[1] * 4
    offsets = np.zeros(n + 1, np.uint64)
    optr = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    total = C.c_uint64(0)

    def ev():
        return torch.cuda.Event(enable_timing=True)
    e = [ev() for _ in range(4)]
    e[0].record()
    st = lib.pclhip_radius_search(tree.h, qp, stride, n, float(radius), 0, optr, None, None, 0, C.byref(total))
    assert st in (0, -5), st
    e[1].record()
    m = int(total.value)
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    d2 = torch.empty(m, dtype=torch.float32, device=dev)
    pcl_amd._lib.check(lib.pclhip_radius_search(tree.h, qp, stride, n, float(radius), 0, optr, C.c_void_p(idx.data_ptr()),
                                               C.c_void_p(d2.data_ptr()), m, C.byref(total)), ctx.h)
    e[2].record()
    off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    cnt = off[1:] - off[:-1]
    nr = nrm[:, :3].contiguous()
    hist = torch.zeros(n * 33, dtype=torch.float32, device=dev)
    d_pi = float(np.float32(1.0) / (np.float32(2.0) * np.float32(math.pi)))

    def chunks(points):
        for a in range(0, n, points):
            b = min(n, a + points)
            lo, hi = int(off[a]), int(off[b])
            src = torch.repeat_interleave(torch.arange(a, b, device=dev), cnt[a:b])
            yield src, idx[lo:hi].long(), d2[lo:hi]
    for src, nb, _ in chunks(1 << 20):
        keep = nb != src
        src, nb = src[keep], nb[keep]
        f1, f2, f3 = pair_features(torch, q[src], nr[src], q[nb], nr[nb])
        for h, c in enumerate(((f1.double() + math.pi) * d_pi, (f2.double() + 1.0) * 0.5, (f3.double() + 1.0) * 0.5)):
            b = torch.clamp(torch.floor(11.0 * c), 0, 10).long()
            hist.index_add_(0, src * 33 + 11 * h + b, torch.ones_like(f1))
    spfh = hist.view(n, 33) * (100.0 / (cnt - 1).float())[:, None]
    spfh = torch.where((cnt > 1)[:, None], spfh, torch.zeros_like(spfh))
    acc = torch.zeros((n, 33), dtype=torch.float32, device=dev)
    for src, nb, dd in chunks(1 << 18):
        w = torch.where(dd != 0, 1.0 / dd, torch.zeros_like(dd))
        acc.index_add_(0, src, spfh[nb] * w[:, None])
    s = acc.view(n, 3, 11).double().sum(2, keepdim=True)
    fp = (acc.view(n, 3, 11).double() * torch.where(s != 0, 100.0 / s, torch.zeros_like(s))).float().view(n, 33)
    e[3].record()
    torch.cuda.synchronize()
    out["neighbours_per_point"] = round((m - n) / n, 3)
    out["pairs"] = m - n
    out["composition_radius_search_torch"] = {
        "gpu_ms": round(e[1].elapsed_time(e[3]), 3), "radius_search_count_call_ms": round(e[0].elapsed_time(e[1]), 3),
        "radius_search_call_ms": round(e[1].elapsed_time(e[2]), 3), "torch_ms": round(e[2].elapsed_time(e[3]), 3),
        "radius_search_output_bytes": m * 8, "checksum": float(torch.nan_to_num(fp).double().sum())}
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    # default: 30 neighbours on a surface of ~4 units of area, pi r^2 n / 4 = 30
    ap.add_argument("--radius", type=float, default=None)
    ap.add_argument("--step", choices=("fused", "composition"), default=None, help="run one step in this process")
    ap.add_argument("--out", default=None, help="with --step: where the step's JSON goes")
    a = ap.parse_args()
    n = a.n
    radius = a.radius if a.radius is not None else math.sqrt(30.0 * 4.0 / (math.pi * n))
    if a.step is not None:
        res = step_fused(n, radius) if a.step == "fused" else step_composition(n, radius)
        text = json.dumps(res)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return 0
    out = {"metric": "fpfh_timing", "points": n, "cloud": "synth.gaussian_surface, k = 8 normals", "radius": radius}
    with tempfile.TemporaryDirectory() as tmp:
        for step in ("fused", "composition"):
            piece = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), str(n),
                   "--radius", repr(radius), "--step", step, "--out", piece]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %s failed with status %d: stopping" % (step, rc), file=sys.stderr)
                return rc
            with open(piece) as f:
                out.update(json.load(f))
    pairs, fused, comp = out["pairs"], out["fused"], out["composition_radius_search_torch"]
    out["speedup_call_vs_composition"] = round(comp["gpu_ms"] / fused["call_gpu_ms"], 2)
    # algorithmic bytes: 32 B of point + normal per pair (pass 1), 132 B of SPFH row per pair (pass 2)
    for name, per_pair, key in (("spfh", 32, "fpfh_spfh_kernel_ms"), ("weight", 132, "fpfh_weight_kernel_ms")):
        nbytes = per_pair * pairs
        out["roofline_" + name] = {"algorithmic_bytes": nbytes, "ms_at_8TBps": round(nbytes / PEAK_BYTES_PER_S * 1e3, 4),
                                   "fraction_of_8TBps": round(nbytes / PEAK_BYTES_PER_S * 1e3 / fused[key], 4)}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fpfh_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
