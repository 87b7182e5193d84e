"""MovingLeastSquares in the C++ mirror (include/pclhip/pcl_compat.hpp): tests/cpp/test_mls_compat.cpp compiled with plain g++
against the C ABI and run on the reference's bun0 cloud (tests/golden/pcd/bun0.pcd) against the reference's own criterion
(test/surface/test_moving_least_squares.cpp:95-118) and the records of the restatement at r = 0.01."""
import os
import subprocess

import numpy as np
import pytest

import mls_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    d = os.path.dirname(os.path.abspath(lib))
    exe = str(tmp_path / "test_mls_compat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_mls_compat.cpp"), "-o", exe,
                           "-L" + d, "-l:" + os.path.basename(lib), "-Wl,-rpath," + d])
    return exe


def test_mls_compat_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2  # usage error: no arguments -> nothing touched the GPU


@pytest.mark.gpu
def test_mls_compat_bunny(tmp_path):
    exe = build(tmp_path)
    bun0 = mr.load_bun0()
    ref = mr.restate(bun0, 0.01)
    rows = np.concatenate([ref["indices"][:, None].astype(np.float64), ref["point"], ref["normal"], ref["curvature"][:, None]],
                          axis=1)
    assert rows.shape == (380, 8)
    np.savetxt(tmp_path / "bun0.txt", bun0, fmt="%.9g")
    np.savetxt(tmp_path / "want.txt", rows, fmt="%.17g")
    r = subprocess.run([exe, str(tmp_path / "bun0.txt"), str(tmp_path / "want.txt")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout, r.stdout + r.stderr
