"""SampleConsensusModelCylinder and RandomSampleConsensus in the C++ mirror (include/pclhip/pcl_compat.hpp):
tests/cpp/test_sac_cylinder_compat.cpp compiled with plain g++ against the C ABI and run on the 20 points of the reference's
cylinder test, with the iterations and the sample of tests/sac_cylinder_restatement.py for its seeded call."""
import os
import subprocess

import numpy as np
import pytest

import sac_cylinder_restatement as cy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    d = os.path.dirname(os.path.abspath(lib))
    exe = str(tmp_path / "test_sac_cylinder_compat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_sac_cylinder_compat.cpp"), "-o", exe,
                           "-L" + d, "-l:" + os.path.basename(lib), "-Wl,-rpath," + d])
    return exe


def test_sac_cylinder_compat_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2  # usage error: no arguments -> nothing touched the GPU


@pytest.mark.gpu
def test_sac_cylinder_compat(tmp_path):
    exe = build(tmp_path)
    g = np.load(os.path.join(ROOT, "tests", "golden", "sac_cylinder_20.npz"))
    cloud, normals = g["cloud"], np.column_stack([g["normals"], np.zeros(20, np.float32)])
    np.savetxt(tmp_path / "sac_cylinder_20.txt", np.column_stack([cloud, normals[:, :3]]), fmt="%.9g")
    ref = cy.compute_model(cy.Model(0.1), cloud, normals, 0.03, seed=1)
    assert ref["in_band"] == 0 and ref["found"] and ref["best_count"] == 20
    args = [str(v) for v in (ref["iterations"], ref["sample"][0], ref["sample"][1])]
    r = subprocess.run([exe, str(tmp_path / "sac_cylinder_20.txt")] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout, r.stdout + r.stderr
