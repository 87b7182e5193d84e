"""BoundaryEstimation in the C++ mirror (include/pclhip/pcl_compat.hpp): tests/cpp/test_boundary_compat.cpp compiled with
plain g++ against the C ABI and run on the reference's bun0 cloud (tests/golden/pcd/bun0.pcd) against the expectations of
test/features/test_boundary_estimation.cpp."""
import os
import subprocess

import numpy as np
import pytest

import boundary_restatement as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    d = os.path.dirname(os.path.abspath(lib))
    exe = str(tmp_path / "test_boundary_compat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_boundary_compat.cpp"), "-o", exe,
                           "-L" + d, "-l:" + os.path.basename(lib), "-Wl,-rpath," + d])
    return exe


def test_boundary_compat_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2  # usage error: no arguments -> nothing touched the GPU


@pytest.mark.gpu
def test_boundary_compat_bunny(tmp_path):
    exe = build(tmp_path)
    np.savetxt(tmp_path / "bun0.txt", br.load_bun0()[0], fmt="%.9g")
    r = subprocess.run([exe, str(tmp_path / "bun0.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout, r.stdout + r.stderr
