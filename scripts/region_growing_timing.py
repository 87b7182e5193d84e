"""Stage timing of RegionGrowing at 10M points: synth's Gaussian surface with its analytic normals, curvatures uniform in
[0, 0.06) (a sixth of the points above the default threshold: leaves and leftover points exist), k = 30 and the reference's
default thresholds.  Every figure is the median over the repeats of what pclhip_index_last_region_growing_stats reports
for one extract(): the GPU time of the k-NN lists, of the collapse and of the two round loops, the whole call, and the
rounds of the two phases.

Each arm runs in a process of its own under its own `timeout` (a library is chosen when it is loaded):
  collapse      this build
  no_collapse   radius.hip built -DPCLHIP_RG_NO_COLLAPSE: the union-find pass left out, every component a single point
The extra build is this script's own (scripts/build_variant.sh ... radius.hip, made here when it is missing); the library
that ships has no such switch.  Before anything is timed every arm runs the call twice and compares the labels of the two
runs; the driver then compares the arms' label checksums and segment counts (the collapse must not change a label).  Any
difference: exit 1.  Writes profiles/region_growing_timing.json (and prints it).

    python scripts/region_growing_timing.py [n] [--k K] [--reps R]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = {"no_collapse": ("rgnocollapse", "-DPCLHIP_RG_NO_COLLAPSE")}


def scene(n, device):
    """(cloud (n, 3), normals (n, 4) = analytic normal + curvature) float32 tensors on `device`"""
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
    curv = torch.rand(n, generator=g, device=device) * 0.06
    return cloud, torch.cat([nrm, curv[:, None]], 1).contiguous()


def worker(a):
    import torch

    import pcl_amd
    cloud, normals = scene(a.n, a.device)
    if a.device == "cpu":  # (the rehearsal on the emulation: host arrays)
        cloud, normals = cloud.numpy(), normals.numpy()
    ctx = pcl_amd.Context(0)
    rg = pcl_amd.RegionGrowing(ctx)
    rg.setInputCloud(cloud)
    rg.setInputNormals(normals)
    rg.setNumberOfNeighbours(a.k)
    off, idx, lab = rg.extractCSR()
    off2, idx2, lab2 = rg.extractCSR()
    as_t = (lambda v: v) if a.device != "cpu" else torch.from_numpy
    same = off.tobytes() == off2.tobytes() and torch.equal(as_t(idx), as_t(idx2)) and torch.equal(as_t(lab), as_t(lab2))
    if not same:
        print(json.dumps({"arm": a.worker, "labels_agree": False}))
        return 1
    t = as_t(lab).to(torch.int64)
    crc = int((t * (torch.arange(len(t), device=t.device) % 65521 + 1)).sum().item())
    rows = []
    for _ in range(a.reps):
        rg.extractCSR()
        st = rg.lastStats()
        st["call_ms"] = rg.lastKernelMs()
        rows.append(st)

    def med(key):
        v = sorted(r[key] for r in rows)
        return v[len(v) // 2]
    out = {key: (round(med(key), 3) if key.endswith("_ms") else med(key)) for key in rows[0]}
    out.update(arm=a.worker, labels_agree=True, labels_crc=crc, segments=int(len(off) - 1), clustered=int(len(idx)))
    print(json.dumps(out))
    return 0


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--arm-timeout", type=int, default=240, help="seconds an arm's process may take")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    libs = {"collapse": lib}
    if "PCLHIP_LIB" not in os.environ:  # (a rehearsal on another library times that library alone)
        for arm, (name, flags) in VARIANTS.items():
            path = os.path.join(ROOT, "pcl_amd", "variants", "libpclhip_%s.so" % name)
            if not os.path.exists(path):
                subprocess.check_call(["bash", os.path.join(ROOT, "scripts", "build_variant.sh"), name, flags, "radius.hip"])
            libs[arm] = path
    arms = {}
    for arm, path in libs.items():
        cmd = ["timeout", "-k", "10", str(a.arm_timeout), sys.executable, os.path.abspath(__file__), str(a.n), "--k", str(a.k),
               "--reps", str(a.reps), "--device", a.device, "--worker", arm]
        p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PCLHIP_LIB=path))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line or not json.loads(line[-1])["labels_agree"]:
            print("arm %s failed (exit %d)\n%s\n%s" % (arm, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return 1  # (nothing more is started after an arm that failed)
        arms[arm] = json.loads(line[-1])
        print("%s: %s" % (arm, line[-1]), file=sys.stderr, flush=True)
    if len({(v["labels_crc"], v["segments"], v["clustered"]) for v in arms.values()}) != 1:
        print("the arms' labels differ: %s" % {k: (v["labels_crc"], v["segments"]) for k, v in arms.items()})
        return 1
    out = {"metric": "region_growing_timing", "points": a.n, "k": a.k, "reps": a.reps,
           "segments": arms["collapse"]["segments"], "clustered": arms["collapse"]["clustered"], "labels_agree": True,
           "arms": {k: {f: v[f] for f in v if f not in ("arm", "labels_agree", "labels_crc", "segments", "clustered")}
                    for k, v in arms.items()}}
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "region_growing_timing.json"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
