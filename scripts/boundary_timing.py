"""BoundaryEstimation timing at 10M points: synth.gaussian_surface, radius 0.001954 (the radius of scripts/iss_timing.py and
scripts/mls_timing.py: 26.2 neighbours per point), k = 10 normals from the device, threshold pi / 2.  Records, in one run,
the GPU time of pclhip_boundary (whole call, its mask pass, its resolve pass) and the share of queries the mask pass left to
the resolve pass, and the time of the same flags composed from what the library offered before it: pclhip_radius_search of
the cloud against itself into device memory, then the angles, a sort and the gaps in torch on the device.  The baseline is
that composition; the flags must be equal outside the unstable band of tests/boundary_restatement.py (a gap within
E = 2^-24 (10 (kappa_a + kappa_b) + 32) of the threshold).  Writes profiles/boundary_timing.json (and prints it).

    python scripts/boundary_timing.py [n] [--radius R]

Each GPU step runs as a child process under its own `timeout`; the first failure ends the run.
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

STEP_TIMEOUT_S = {"fused": 240, "composition": 480}
THRESHOLD = math.pi / 2
NORMALS_K = 10
U24 = 2.0 ** -24
PI_F = 3.1415927410125732


def setup(n):
    import torch

    import pcl_amd
    ctx = pcl_amd.Context(0)
    q = torch.from_numpy(pcl_amd.synth.gaussian_surface(n)[:, :3].copy()).cuda()
    tree = pcl_amd.KdTree(ctx)
    tree.setInputCloud(q)
    ne = pcl_amd.NormalEstimation(ctx)
    ne.setInputCloud(q)
    ne.setSearchMethod(tree)
    ne.setKSearch(NORMALS_K)
    nrm = ne.compute()
    if not hasattr(nrm, "is_cuda"):
        nrm = torch.from_numpy(nrm)
    nrm = nrm[:, :3].contiguous().cuda()
    torch.cuda.synchronize()
    return torch, pcl_amd, ctx, q, nrm, tree, {"index_build_ms": round(tree.build_ms(), 3)}


def estimator(pcl_amd, ctx, q, tree, radius):
    b = pcl_amd.BoundaryEstimation(ctx)
    b.setInputCloud(q)
    b.setSearchMethod(tree)  # the normals are the ones the tree holds
    b.setRadiusSearch(radius)
    b.setAngleThreshold(THRESHOLD)
    return b


def step_fused(n, radius, reps=5):
    torch, pcl_amd, ctx, q, nrm, tree, out = setup(n)
    b = estimator(pcl_amd, ctx, q, tree, radius)
    rows = []
    for _ in range(reps + 1):  # the first is the warm-up
        flags = b.compute()
        torch.cuda.synchronize()
        rows.append((b.lastKernelMs(),) + b.lastPassMs())
    rows = sorted(rows[1:])
    call, mask_ms, resolve_ms = rows[len(rows) // 2]
    out["fused"] = {"call_gpu_ms": round(call, 3), "bnd_mask_kernel_ms": round(mask_ms, 3),
                    "bnd_resolve_kernel_ms": round(resolve_ms, 3), "resolved_queries": b.lastResolved(),
                    "resolved_share": round(b.lastResolved() / n, 6), "boundary_points": int(flags.long().sum()),
                    "invalid": b.invalid_count}
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


def torch_basis(torch, nrm):
    """getCoordinateSystemOnPlane for every normal, float32, the operations of tests/boundary_restatement.py -> u, v [n, 3]"""
    n4 = torch.cat([nrm, torch.zeros_like(nrm[:, :1])], dim=1)
    maxi = n4.abs().argmax(dim=1)  # (ties: any index -- an exact tie of two float components; none on this cloud)
    sndi = (maxi == 0).long()
    nm, ns = n4.gather(1, maxi[:, None])[:, 0], n4.gather(1, sndi[:, None])[:, 0]
    inv = 1.0 / torch.sqrt(ns * ns + nm * nm)
    v = torch.zeros_like(n4)
    v.scatter_(1, maxi[:, None], (-ns * inv)[:, None])
    v.scatter_(1, sndi[:, None], (nm * inv)[:, None])
    u = torch.stack([nrm[:, 1] * v[:, 2] - nrm[:, 2] * v[:, 1], nrm[:, 2] * v[:, 0] - nrm[:, 0] * v[:, 2],
                     nrm[:, 0] * v[:, 1] - nrm[:, 1] * v[:, 0]], dim=1)
    return u, v[:, :3].contiguous()


def torch_flags(torch, q, nrm, off, idx, thr, points=1 << 20):
    """the flags by sorting, chunk by chunk -> flag [n] bool, own [n] bool (an unstable comparison), largest kappa"""
    n, dev = len(q), q.device
    u, v = torch_basis(torch, nrm)
    ok = torch.isfinite(nrm).all(dim=1) & (nrm != 0).any(dim=1)
    thr32 = torch.tensor(thr, dtype=torch.float32, device=dev)
    thr64 = float(thr32)
    two_pi = torch.tensor(2.0, dtype=torch.float32, device=dev) * torch.tensor(PI_F, dtype=torch.float32, device=dev)
    flag = torch.zeros(n, dtype=torch.bool, device=dev)
    own = torch.zeros(n, dtype=torch.bool, device=dev)
    cnt = off[1:] - off[:-1]
    kmax = 0.0
    for a in range(0, n, points):
        b = min(n, a + points)
        lo, hi = int(off[a]), int(off[b])
        src = torch.repeat_interleave(torch.arange(a, b, device=dev), cnt[a:b])
        nb = idx[lo:hi].long()
        d = q[nb] - q[src]
        keep = (d != 0).any(dim=1)
        src, d = src[keep], d[keep]
        us, vs = u[src], v[src]
        x = (us[:, 0] * d[:, 0] + us[:, 1] * d[:, 1]) + us[:, 2] * d[:, 2]
        y = (vs[:, 0] * d[:, 0] + vs[:, 1] * d[:, 1]) + vs[:, 2] * d[:, 2]
        ang = torch.atan2(y, x)
        kappa = d.double().norm(dim=1) / torch.hypot(x.double(), y.double())
        # one sort: the query in the high part of a float64 key, the angle (24 bits) in the low part -- exact
        key = (src - a).double() * 8.0 + (ang.double() + math.pi)
        order = torch.argsort(key)
        src, ang, kappa = src[order], ang[order], kappa[order]
        m = torch.bincount(src - a, minlength=b - a)
        has = m > 0
        first = torch.cumsum(m, 0) - m
        last = first + m - 1
        same = src[1:] == src[:-1]
        gap = ang[1:] - ang[:-1]
        E = U24 * (10.0 * (kappa[1:] + kappa[:-1]) + 32.0)
        big = torch.zeros(b - a, dtype=torch.float32, device=dev)
        big.scatter_reduce_(0, (src[:-1] - a)[same], gap[same], "amax", include_self=True)
        close = same & ((gap.double() - thr64).abs() <= E)
        unstable = torch.zeros(b - a, dtype=torch.bool, device=dev)
        unstable[(src[:-1] - a)[close]] = True
        f, l = first[has], last[has]
        wrap = (two_pi - ang[l]) + ang[f]
        Ew = U24 * (10.0 * (kappa[l] + kappa[f]) + 32.0)
        big[has] = torch.maximum(big[has], wrap)
        unstable[has] |= (wrap.double() - thr64).abs() <= Ew
        live = ok[a:b] & (cnt[a:b] >= 3) & has
        flag[a:b] = live & (big > thr32)
        own[a:b] = live & unstable
        if len(kappa):
            kmax = max(kmax, float(kappa[torch.isfinite(kappa)].max()))
    return flag, own, kmax


def step_composition(n, radius):
    import numpy as np
    torch, pcl_amd, ctx, q, nrm, tree, out = setup(n)
    b = estimator(pcl_amd, ctx, q, tree, radius)  # the code under test, for the comparison only
    dev_flags = b.compute().bool()
    torch.cuda.synchronize()
    off, idx, search_ms = neighbour_lists(torch, np, pcl_amd, ctx, tree, q, radius)
    pairs = int(off[-1])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    flag, own, kmax = torch_flags(torch, q, nrm, off, idx, THRESHOLD)
    t1.record()
    torch.cuda.synchronize()
    torch_ms = t0.elapsed_time(t1)
    differ = int((flag != dev_flags)[~own].sum())
    out["neighbours_per_point"] = round((pairs - n) / n, 3)
    out["pairs"] = pairs
    out["composition_radius_search_torch"] = {
        "gpu_ms": round(search_ms + torch_ms, 3), "radius_search_call_ms": round(search_ms, 3), "torch_ms": round(torch_ms, 3),
        "radius_search_output_bytes": pairs * 8, "boundary_points": int(flag.sum())}
    out["comparison"] = {"boundary_points_device": int(dev_flags.sum()), "own_unstable": int(own.sum()),
                         "differ_outside_the_band": differ, "differ_anywhere": int((flag != dev_flags).sum()),
                         "largest_kappa": round(kmax, 1)}
    assert differ == 0, out["comparison"]
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--radius", type=float, default=0.001954)
    ap.add_argument("--step", choices=tuple(STEP_TIMEOUT_S), default=None, help="run one step in this process")
    ap.add_argument("--out", default=None, help="with --step: where the step's JSON goes")
    a = ap.parse_args()
    n, radius = a.n, a.radius
    if a.step is not None:
        res = {"fused": lambda: step_fused(n, radius), "composition": lambda: step_composition(n, radius)}[a.step]()
        text = json.dumps(res)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return 0
    out = {"metric": "boundary_timing", "points": n, "cloud": "synth.gaussian_surface", "radius": radius,
           "angle_threshold": THRESHOLD, "normals_k": NORMALS_K}
    with tempfile.TemporaryDirectory() as tmp:
        for step in STEP_TIMEOUT_S:
            piece = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), str(n),
                   "--radius", repr(radius), "--step", step, "--out", piece]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %s failed with status %d: stopping" % (step, rc), file=sys.stderr)
                return rc
            with open(piece) as f:
                out.update(json.load(f))
    fused, comp = out["fused"], out["composition_radius_search_torch"]
    out["speedup_call_vs_composition"] = round(comp["gpu_ms"] / fused["call_gpu_ms"], 2)
    out["mask_pass_vs_iss_scatter_2_02_ms"] = round(fused["bnd_mask_kernel_ms"] / 2.02, 2)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "boundary_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
