"""EuclideanClusterExtraction in the CPU tier: the `-m gpu` tests of tests/test_gpu_cluster.py run on the wavefront
emulation of tests/wavesim (the recipe of tests/test_radius_rejector_wavesim.py: PCLHIP_LIB = the emulation,
PCLHIP_ALLOW_WAVESIM=1, in a subprocess).  No case takes a minute there (the slowest, the 8,192 coincident points, takes
a few seconds): only the torch-buffer case stays on the GPU.  The emulation's workgroups run on host threads and its
atomics are the host's, so the hooks really race here."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = os.path.join(ROOT, "tests", "wavesim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GPU_ONLY = "not torch"


@pytest.fixture(scope="module")
def wavesim_lib():
    if not os.path.exists(CLANG) or shutil.which("make") is None:
        pytest.skip("needs the ROCm clang++ and make")
    r = subprocess.run(["make", "-C", WS, "-j", str(min(16, os.cpu_count() or 1))], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(WS, "libpclhip_wavesim.so")


def on_the_emulation(wavesim_lib, module, select):
    env = dict(os.environ, PCLHIP_LIB=wavesim_lib, PCLHIP_ALLOW_WAVESIM="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", select,
           os.path.join(ROOT, "tests", module)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, tail


def test_cluster_gpu_tests_on_the_emulation(wavesim_lib):
    on_the_emulation(wavesim_lib, "test_gpu_cluster.py", GPU_ONLY)


def test_cluster_regimes_on_the_emulation(wavesim_lib):
    """tests/test_gpu_cluster_regimes.py: the `fullgrid` cases stay on the GPU as well -- their sizes follow the device's
    CU count, and with its 32 blocks the emulation reaches the hook kernel's second query group at the sizes of the module
    above already"""
    on_the_emulation(wavesim_lib, "test_gpu_cluster_regimes.py", GPU_ONLY + " and not fullgrid")
