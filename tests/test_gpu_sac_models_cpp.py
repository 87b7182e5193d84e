"""The constrained planes of SACSegmentation and SACSegmentationFromNormals in the C++ mirror (include/pclhip/
pcl_compat.hpp): tests/cpp/test_sac_models_compat.cpp compiled with plain g++ against the C ABI and run on the cloud and the
normals of the reference's plane tests, with the counts of tests/sac_models_restatement.py for its two seeded calls."""
import os
import subprocess

import numpy as np
import pytest

import sac_models_restatement as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    d = os.path.dirname(os.path.abspath(lib))
    exe = str(tmp_path / "test_sac_models_compat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_sac_models_compat.cpp"), "-o", exe,
                           "-L" + d, "-l:" + os.path.basename(lib), "-Wl,-rpath," + d])
    return exe


def test_sac_models_compat_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2  # usage error: no arguments -> nothing touched the GPU


@pytest.mark.gpu
def test_sac_models_compat(tmp_path):
    exe = build(tmp_path)
    cloud = np.load(os.path.join(ROOT, "tests", "golden", "sac_plane_radius.npz"))["cloud"][:, :3]
    normals = np.load(os.path.join(ROOT, "tests", "golden", "sac_plane_normals.npz"))["normals"]
    np.savetxt(tmp_path / "sac_plane_normals.txt", np.column_stack([cloud, normals]), fmt="%.9g")
    a = sm.segment(sm.Model(sm.NORMAL_PLANE, ndw=0.01), cloud, normals, 0.03, seed=1)
    b = sm.segment(sm.Model(sm.PERPENDICULAR_PLANE, axis=(-0.8964, -0.5868, -1.208), eps_angle=0.1), cloud, None, 0.03, seed=1)
    assert a["in_band"] == 0 and b["gate_band"] == 0 and a["found"] and b["found"]
    args = [str(v) for v in (a["best_count"], a["iterations"], b["best_count"], b["iterations"])]
    r = subprocess.run([exe, str(tmp_path / "sac_plane_normals.txt")] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout, r.stdout + r.stderr
