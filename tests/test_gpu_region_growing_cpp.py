"""RegionGrowing in the C++ mirror (include/pclhip/pcl_compat.hpp): tests/cpp/test_region_growing_compat.cpp compiled with
plain g++ against the C ABI and run on the roof of tests/region_growing_restatement.py, whose labels it compares with the
literal restatement's."""
import os
import subprocess

import numpy as np
import pytest

import region_growing_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    lib = os.environ.get("PCLHIP_LIB") or os.path.join(ROOT, "pcl_amd", "libpclhip.so")
    d = os.path.dirname(os.path.abspath(lib))
    exe = str(tmp_path / "test_region_growing_compat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_region_growing_compat.cpp"), "-o", exe,
                           "-L" + d, "-l:" + os.path.basename(lib), "-Wl,-rpath," + d])
    return exe


def test_region_growing_compat_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2  # usage error: no arguments -> nothing touched the GPU


@pytest.mark.gpu
def test_region_growing_compat_roof(tmp_path):
    exe = build(tmp_path)
    pts, nrm, _ = rr.roof()
    lists = rr.knn_lists(pts, 30)
    assert rr.near_threshold(nrm, lists, rr.DEFAULT_THETA) == 0
    clusters, labels, _ = rr.literal(pts, nrm, lists=lists)
    sized, labels_sized, _ = rr.literal(pts, nrm, mn=30, mx=160, lists=lists)
    assert len(clusters) == 2 and len(sized) == 1
    np.savetxt(tmp_path / "roof.txt", np.concatenate([pts, nrm], axis=1), fmt="%.9g")
    np.savetxt(tmp_path / "labels.txt", np.stack([labels, labels_sized], axis=1), fmt="%d")
    r = subprocess.run([exe, str(tmp_path / "roof.txt"), str(tmp_path / "labels.txt")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout, r.stdout + r.stderr
