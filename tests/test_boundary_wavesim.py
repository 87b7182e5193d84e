"""BoundaryEstimation in the CPU tier: the `-m gpu` tests of tests/test_gpu_boundary.py and tests/test_gpu_boundary_regimes.py
and the C++ mirror's bun0 test (tests/test_gpu_boundary_cpp.py) run on the wavefront emulation of tests/wavesim (the recipe of
tests/test_iss_wavesim.py: PCLHIP_LIB = the emulation, PCLHIP_ALLOW_WAVESIM=1, in a subprocess; boundary.hpp arrives there
through radius.hip).  Deselected: the torch case (device buffers need the GPU) and the 65,619-point index."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = os.path.join(ROOT, "tests", "wavesim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def wavesim_lib():
    if not os.path.exists(CLANG) or shutil.which("make") is None:
        pytest.skip("needs the ROCm clang++ and make")
    r = subprocess.run(["make", "-C", WS, "-j", str(min(16, os.cpu_count() or 1))], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(WS, "libpclhip_wavesim.so")


def test_boundary_gpu_tests_on_the_emulation(wavesim_lib):
    env = dict(os.environ, PCLHIP_LIB=wavesim_lib, PCLHIP_ALLOW_WAVESIM="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(ROOT, "tests", "test_gpu_boundary.py"), os.path.join(ROOT, "tests", "test_gpu_boundary_cpp.py"),
           os.path.join(ROOT, "tests", "test_gpu_boundary_regimes.py"),
           "--deselect", "tests/test_gpu_boundary.py::test_torch_device_buffers",
           "--deselect", "tests/test_gpu_boundary_regimes.py::test_three_box_levels"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, tail
    assert "3 deselected" in r.stdout, tail  # the two above and the C++ module's link test, which carries no gpu mark
