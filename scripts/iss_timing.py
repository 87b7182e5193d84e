"""ISSKeypoint3D timing at 10M points: synth.gaussian_surface, salient radius 0.001954 (the radius of scripts/fpfh_timing.py:
26.2 neighbours per point), non-max radius two thirds of it.  Records, in one run, the GPU time of pclhip_iss_keypoints
(whole call, and its two kernels) and the time of the same keypoints composed from what the library offered before it:
pclhip_radius_search of the cloud against itself into device memory, then a segment sum of the outer products,
torch.linalg.eigvalsh and a segment maximum in torch on the device.  The baseline is that composition; the two keypoint sets
must agree outside the unstable band of tests/iss_restatement.py.  A third step puts the detector in front of
SampleConsensusPrerejective at the workload of scripts/scp_timing.py: the rows its feature k-NN searches, and the align
time, with and without it (a figure for the record).  Writes profiles/iss_timing.json (and prints it).

    python scripts/iss_timing.py [n] [--radius R]

Each GPU step runs as a child process under its own `timeout`; the first failure ends the run.
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

STEP_TIMEOUT_S = {"fused": 240, "composition": 480, "prerejective": 420}
PEAK_BYTES_PER_S = 8.0e12      # HBM3E of the MI355X
PEAK_FP64_FLOPS = 78.6e12      # vector fp64 of AMD's specification
GAMMA, MIN_NEIGHBORS = 0.975, 5
U = 2.0 ** -53


def setup(n):
    import torch

    import pcl_amd
    ctx = pcl_amd.Context(0)
    q = torch.from_numpy(pcl_amd.synth.gaussian_surface(n)[:, :3].copy()).cuda()
    tree = pcl_amd.KdTree(ctx)
    tree.setInputCloud(q)
    torch.cuda.synchronize()
    return torch, pcl_amd, ctx, q, tree, {"index_build_ms": round(tree.build_ms(), 3)}


def detector(pcl_amd, ctx, q, tree, rs, rn):
    d = pcl_amd.ISSKeypoint3D(ctx)
    d.setInputCloud(q)
    d.setSearchMethod(tree)
    d.setSalientRadius(rs)
    d.setNonMaxRadius(rn)
    d.setThreshold21(GAMMA)
    d.setThreshold32(GAMMA)
    d.setMinNeighbors(MIN_NEIGHBORS)
    return d


def step_fused(n, rs, rn, reps=5):
    torch, pcl_amd, ctx, q, tree, out = setup(n)
    d = detector(pcl_amd, ctx, q, tree, rs, rn)
    rows = []
    for _ in range(reps + 1):  # the first is the warm-up
        keys = d.compute()
        torch.cuda.synchronize()
        rows.append((d.lastKernelMs(),) + d.lastPassMs())
    rows = sorted(rows[1:])
    call, scatter_ms, nms_ms = rows[len(rows) // 2]
    out["fused"] = {"call_gpu_ms": round(call, 3), "iss_scatter_kernel_ms": round(scatter_ms, 3),
                    "iss_nms_kernel_ms": round(nms_ms, 3), "keypoints": int(len(keys)),
                    "checksum": int(keys.long().sum())}
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


def step_composition(n, rs, rn):
    import numpy as np
    torch, pcl_amd, ctx, q, tree, out = setup(n)
    dev = q.device
    # the code under test, for the comparison only
    d = detector(pcl_amd, ctx, q, tree, rs, rn)
    keys = d.compute().long()
    torch.cuda.synchronize()

    def chunks(off, idx, points):
        cnt = off[1:] - off[:-1]
        for a in range(0, n, points):
            b = min(n, a + points)
            lo, hi = int(off[a]), int(off[b])
            yield torch.repeat_interleave(torch.arange(a, b, device=dev), cnt[a:b]), idx[lo:hi].long()

    t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    off, idx, search_ms = neighbour_lists(torch, np, pcl_amd, ctx, tree, q, rs)
    pairs = int(off[-1])
    t0.record()
    m = off[1:] - off[:-1]
    q64 = q.double()
    sums = torch.zeros((n, 6), dtype=torch.float64, device=dev)
    for src, nb in chunks(off, idx, 1 << 20):
        dd = q64[nb] - q64[src]
        prod = torch.stack([dd[:, 0] * dd[:, 0], dd[:, 0] * dd[:, 1], dd[:, 0] * dd[:, 2], dd[:, 1] * dd[:, 1],
                            dd[:, 1] * dd[:, 2], dd[:, 2] * dd[:, 2]], dim=1)
        sums.index_add_(0, src, prod)
    del idx
    eig = torch.empty((n, 3), dtype=torch.float64, device=dev)
    for a in range(0, n, 1 << 20):
        s6 = sums[a:a + (1 << 20)]
        c = torch.stack([s6[:, 0], s6[:, 1], s6[:, 2], s6[:, 1], s6[:, 3], s6[:, 4], s6[:, 2], s6[:, 4], s6[:, 5]],
                        dim=1).view(-1, 3, 3)
        eig[a:a + (1 << 20)] = torch.linalg.eigvalsh(c).flip(1)
    trace = sums[:, 0] + sums[:, 3] + sums[:, 5]
    e1, e2, e3 = eig[:, 0], eig[:, 1], eig[:, 2]
    ok = (m >= MIN_NEIGHBORS) & torch.isfinite(eig).all(dim=1) & (e3 >= 0) & (e2 / e1 < GAMMA) & (e3 / e2 < GAMMA)
    sal = torch.where(ok, e3, torch.zeros_like(e3))
    t1.record()
    off2, idx2, search2_ms = neighbour_lists(torch, np, pcl_amd, ctx, tree, q, rn)
    pairs2 = int(off2[-1])
    t2.record()
    m2 = off2[1:] - off2[:-1]
    top = torch.zeros(n, dtype=torch.float64, device=dev)
    for src, nb in chunks(off2, idx2, 1 << 21):
        top.scatter_reduce_(0, src, sal[nb], "amax", include_self=True)
    key = (sal > 0) & (m2 >= MIN_NEIGHBORS) & ~(sal < top)
    t3 = torch.cuda.Event(enable_timing=True)
    t3.record()
    torch.cuda.synchronize()
    # the unstable band (tests/iss_restatement.py): points that own a comparison closer than the bound, and their neighbours
    B = (m + 32).double() * U * trace
    live = m >= MIN_NEIGHBORS
    own = live & (((e2 - GAMMA * e1).abs() <= 2 * B) | ((e3 - GAMMA * e2).abs() <= 2 * B) | (e3 <= B) | (e2 <= B))
    for src, nb in chunks(off2, idx2, 1 << 21):
        diff = (sal[src] - sal[nb]).abs()
        close = (sal[src] > 0) & (diff != 0) & (diff <= B[src] + B[nb])
        own[src[close]] = True
    excluded = own.clone()
    for src, nb in chunks(off2, idx2, 1 << 21):
        excluded[src[own[nb]]] = True
    flag = torch.zeros(n, dtype=torch.bool, device=dev)
    flag[keys] = True
    differ = int((flag != key)[~excluded].sum())
    torch_ms = t0.elapsed_time(t1) + t2.elapsed_time(t3)
    out["neighbours_per_point"] = round((pairs - n) / n, 3)
    out["pairs_salient"] = pairs
    out["pairs_non_max"] = pairs2
    out["salient_points"] = int((sal > 0).sum())
    out["composition_radius_search_torch"] = {
        "gpu_ms": round(search_ms + search2_ms + torch_ms, 3), "radius_search_calls_ms": round(search_ms + search2_ms, 3),
        "torch_ms": round(torch_ms, 3), "radius_search_output_bytes": (pairs + pairs2) * 8, "keypoints": int(key.sum())}
    out["comparison"] = {"keypoints_device": int(len(keys)), "own_unstable": int(own.sum()), "left_out": int(excluded.sum()),
                         "differ_outside_the_band": differ, "differ_anywhere": int((flag != key).sum())}
    assert differ == 0, out["comparison"]
    return out


def step_prerejective(n_raw=2_000_000, leaf=0.0066):
    """the workload of scripts/scp_timing.py, the source once whole and once as its ISS keypoints"""
    import numpy as np

    import scp_timing as st
    torch, pcl_amd, ctx, (src, tgt), (fs, ft), (stree, ttree), radius = st.prepare(n_raw, leaf)
    d = detector(pcl_amd, ctx, src, stree, radius, radius * 2.0 / 3.0)
    keys = d.compute().long()
    torch.cuda.synchronize()
    res = {"source_points": len(src), "target_points": len(tgt), "salient_radius": radius, "keypoints": int(len(keys)),
           "iss_call_gpu_ms": round(d.lastKernelMs(), 3)}
    for name, cloud, feats in (("without_keypoints", src, fs), ("with_keypoints", src[keys].contiguous(), fs[keys].contiguous())):
        s = pcl_amd.SampleConsensusPrerejective(ctx)
        s.setInputSource(cloud)
        s.setSearchMethodTarget(ttree)
        s.setSourceFeatures(feats)
        s.setTargetFeatures(ft)
        s.setMaxCorrespondenceDistance(1.5 * leaf)
        s.setMaximumIterations(st.ITERATIONS)
        s.setNumberOfSamples(st.SAMPLES)
        s.setCorrespondenceRandomness(st.RANDOMNESS)
        s.setSimilarityThreshold(st.SIMILARITY)
        s.setSeed(1)
        for rep in range(2):  # the second is reported: the first align of a fresh feature cache, code objects warm
            s.setTargetFeatures(ft)
            s.align()
        r = s.result
        err = float(np.abs(s.getFinalTransformation().astype(np.float64) @ np.linalg.inv(st.big_motion()) @
                           np.linalg.inv(pcl_amd.synth.ground_truth_transform()) - np.eye(4)).max())
        res[name] = {"knn_rows": int(r.knn_rows), "align_total_ms": round(r.total_ms, 3), "knn_ms": round(r.knn_ms, 3),
                     "survivors": st.ITERATIONS - int(r.rejected), "converged": bool(r.converged),
                     "pose_error_vs_truth": err}
    return {"prerejective": res}


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--radius", type=float, default=0.001954, help="the salient radius; the non-max radius is 2 / 3 of it")
    ap.add_argument("--step", choices=tuple(STEP_TIMEOUT_S), default=None, help="run one step in this process")
    ap.add_argument("--out", default=None, help="with --step: where the step's JSON goes")
    a = ap.parse_args()
    n, rs = a.n, a.radius
    rn = rs * 2.0 / 3.0
    if a.step is not None:
        res = {"fused": lambda: step_fused(n, rs, rn), "composition": lambda: step_composition(n, rs, rn),
               "prerejective": step_prerejective}[a.step]()
        text = json.dumps(res)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return 0
    out = {"metric": "iss_timing", "points": n, "cloud": "synth.gaussian_surface", "salient_radius": rs, "non_max_radius": rn,
           "gamma_21": GAMMA, "gamma_32": GAMMA, "min_neighbors": MIN_NEIGHBORS}
    with tempfile.TemporaryDirectory() as tmp:
        for step in STEP_TIMEOUT_S:
            piece = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), str(n),
                   "--radius", repr(rs), "--step", step, "--out", piece]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %s failed with status %d: stopping" % (step, rc), file=sys.stderr)
                return rc
            with open(piece) as f:
                out.update(json.load(f))
    fused, comp = out["fused"], out["composition_radius_search_torch"]
    out["speedup_call_vs_composition"] = round(comp["gpu_ms"] / fused["call_gpu_ms"], 2)
    # algorithmic bytes: 16 B of point per pair (scatter), 8 B of saliency per pair (non-max); 6 fp64 FMA per scatter pair
    for name, per_pair, pairs, key in (("scatter", 16, out["pairs_salient"], "iss_scatter_kernel_ms"),
                                       ("nms", 8, out["pairs_non_max"], "iss_nms_kernel_ms")):
        nbytes = per_pair * pairs
        out["roofline_" + name] = {"algorithmic_bytes": nbytes, "ms_at_8TBps": round(nbytes / PEAK_BYTES_PER_S * 1e3, 4),
                                   "fraction_of_8TBps": round(nbytes / PEAK_BYTES_PER_S * 1e3 / fused[key], 4)}
    flops = 12 * out["pairs_salient"]
    out["roofline_scatter"].update({"fp64_fma_per_pair": 6, "fp64_flops": flops,
                                    "ms_at_fp64_peak": round(flops / PEAK_FP64_FLOPS * 1e3, 4)})
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "iss_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
