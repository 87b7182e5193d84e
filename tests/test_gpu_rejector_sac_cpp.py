"""CorrespondenceRejectorSampleConsensus in the C++ mirror (include/pclhip/pcl_compat.hpp): tests/cpp/
test_rejector_sac_compat.cpp compiled with plain g++ against the C ABI and run on the bunny pairs of the reference's test,
with the count of tests/rejector_sac_restatement.py for its seeded call."""
import json
import os
import subprocess

import numpy as np
import pytest

import rejector_sac_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    d = os.path.dirname(os.path.abspath(lib))
    exe = str(tmp_path / "test_rejector_sac_compat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_rejector_sac_compat.cpp"), "-o", exe,
                           "-L" + d, "-l:" + os.path.basename(lib), "-Wl,-rpath," + d])
    return exe


def test_rejector_sac_compat_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2  # usage error: no arguments -> nothing touched the GPU


@pytest.mark.gpu
def test_rejector_sac_compat(tmp_path):
    exe = build(tmp_path)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    f = json.load(open(os.path.join(ROOT, "tests", "golden", "rejector_sac_bun.json")))
    z = np.load(os.path.join(ROOT, "tests", "golden", "bunny.npz"))
    src = np.ascontiguousarray(z["bun0"][:, :3], np.float32)
    tgt = np.ascontiguousarray(z["bun4"][:, :3], np.float32)
    co = np.array(g["correspondences_original"], np.int32)
    seed = 2
    own = rr.reject(src, tgt, co[:, 0], co[:, 1], f["rej_sac_max_dist"], f["rej_sac_max_iter"], seed=seed)
    assert own["has_model"] and own["k_margin"] > 64 * 2.0 ** -52
    with open(tmp_path / "bunny_pairs.txt", "w") as out:
        out.write("%d %d %d\n" % (len(src), len(tgt), len(co)))
        np.savetxt(out, src, fmt="%.9g")
        np.savetxt(out, tgt, fmt="%.9g")
        np.savetxt(out, co, fmt="%d")
        np.savetxt(out, np.array(f["transform_from_SAC"], np.float32), fmt="%.9g")
    r = subprocess.run([exe, str(tmp_path / "bunny_pairs.txt"), str(seed), str(own["best_count"]), str(own["iterations"])],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout, r.stdout + r.stderr
