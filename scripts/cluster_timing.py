"""EuclideanClusterExtraction timing at 10M points, two clouds: synth's Gaussian surface at the radius of
scripts/fpfh_timing.py (about 26 neighbours per point: one component and a few stragglers) and synth's `clusters` family
at half that radius (the thin background falls apart into many components, the ten dense discs stay whole).  Records, in
one run per cloud, the GPU time of pclhip_euclidean_clusters (the whole call, its hook and its flatten kernel), the
cluster count, the unions attempted per point, and the time of the same labels composed from what the library offered
before: pclhip_radius_search of the cloud against itself into device memory, then min-label propagation over those lists in
torch until nothing changes (with pointer jumping, label = label[label], after every sweep: without it the sweeps number
the graph's diameter).  The baseline is that composition; both partitions are checked to be the same.
Writes profiles/cluster_timing.json (and prints it).

    python scripts/cluster_timing.py [n]

Each cloud runs as a child process under its own `timeout`; the first failure ends the run.
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

STEP_TIMEOUT_S = 420
CLOUDS = {"sheet": 1.0, "clusters": 0.5}  # family -> tolerance as a multiple of fpfh_timing's radius


def step(kind, n, tolerance, reps=5):
    import numpy as np
    import torch

    import pcl_amd
    ctx = pcl_amd.Context(0)
    q = torch.from_numpy(pcl_amd.synth.family_cloud(kind, n)[:, :3].copy()).cuda()
    tree = pcl_amd.KdTree(ctx)
    tree.setInputCloud(q)
    out = {"tolerance": tolerance, "index_build_ms": round(tree.build_ms(), 3)}
    e = pcl_amd.EuclideanClusterExtraction(ctx)
    e.setInputCloud(q)
    e.setSearchMethod(tree)
    e.setClusterTolerance(tolerance)
    rows = []
    for _ in range(reps + 1):  # the first is the warm-up
        off, idx, lab = e.extractCSR()
        torch.cuda.synchronize()
        s = e.lastStats()
        rows.append((e.lastKernelMs(), s["hook_ms"], s["flatten_ms"], s["unions"]))
    rows = sorted(rows[1:])
    call, hook, flat, unions = rows[len(rows) // 2]
    sizes = np.diff(off.astype(np.int64))
    out["fused"] = {"call_gpu_ms": round(call, 3), "cluster_hook_kernel_ms": round(hook, 3),
                    "cluster_flatten_kernel_ms": round(flat, 3), "bookkeeping_ms": round(call - hook - flat, 3),
                    "clusters": int(len(sizes)), "largest": int(sizes[0]) if len(sizes) else 0,
                    "singletons": int((sizes == 1).sum()), "unions_attempted_per_point": round(unions / n, 4)}
    # the composition: radius lists into device memory, then min-label propagation
    lib, dev = ctx.lib, q.device
    qp, stride = C.c_void_p(q.data_ptr()), q.shape[1] * 4
    offsets = np.zeros(n + 1, np.uint64)
    optr = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    total = C.c_uint64(0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    st = lib.pclhip_radius_search(tree.h, qp, stride, n, float(tolerance), 0, optr, None, None, 0, C.byref(total))
    assert st in (0, -5), st
    ev[1].record()
    m = int(total.value)
    nb = torch.empty(m, dtype=torch.int32, device=dev)
    d2 = torch.empty(m, dtype=torch.float32, device=dev)
    pcl_amd._lib.check(lib.pclhip_radius_search(tree.h, qp, stride, n, float(tolerance), 0, optr, C.c_void_p(nb.data_ptr()),
                                               C.c_void_p(d2.data_ptr()), m, C.byref(total)), ctx.h)
    ev[2].record()
    o = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    src = torch.repeat_interleave(torch.arange(n, device=dev), o[1:] - o[:-1])
    nbl = nb.long()
    label = torch.arange(n, device=dev)
    sweeps = 0
    while True:
        new = label.scatter_reduce(0, src, label[nbl], "amin")
        new = new[new]
        sweeps += 1
        if torch.equal(new, label):
            break
        label = new
    ev[3].record()
    torch.cuda.synchronize()
    # the same partition: as many distinct (fused, composed) pairs as labels on either side
    pairs = torch.unique(lab.long() * n + label).numel()
    k = int(len(sizes))
    assert int((lab < 0).sum()) == 0 and pairs == k == torch.unique(label).numel(), (pairs, k)
    out["neighbours_per_point"] = round((m - n) / n, 3)
    out["composition_radius_search_torch"] = {
        "gpu_ms": round(ev[1].elapsed_time(ev[3]), 3), "radius_search_count_call_ms": round(ev[0].elapsed_time(ev[1]), 3),
        "radius_search_call_ms": round(ev[1].elapsed_time(ev[2]), 3), "torch_ms": round(ev[2].elapsed_time(ev[3]), 3),
        "sweeps": sweeps, "radius_search_output_bytes": m * 8, "same_partition": True}
    out["speedup_call_vs_composition"] = round(out["composition_radius_search_torch"]["gpu_ms"] / call, 2)
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--step", choices=tuple(CLOUDS), default=None, help="run one cloud in this process")
    ap.add_argument("--out", default=None, help="with --step: where the step's JSON goes")
    a = ap.parse_args()
    n = a.n
    radius = math.sqrt(30.0 * 4.0 / (math.pi * n))  # scripts/fpfh_timing.py
    if a.step is not None:
        text = json.dumps(step(a.step, n, CLOUDS[a.step] * radius))
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return 0
    out = {"metric": "cluster_timing", "points": n, "radius_of_fpfh_timing": radius}
    with tempfile.TemporaryDirectory() as tmp:
        for kind in CLOUDS:
            piece = os.path.join(tmp, kind + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), str(n), "--step", kind,
                   "--out", piece]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("cloud %s failed with status %d: stopping" % (kind, rc), file=sys.stderr)
                return rc
            with open(piece) as f:
                out[kind] = json.load(f)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cluster_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
