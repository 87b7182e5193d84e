"""SACSegmentation (planes, RANSAC) in the CPU tier: the `-m gpu` tests of tests/test_gpu_sac.py run on the wavefront
emulation of tests/wavesim (the recipe of tests/test_cluster_wavesim.py: PCLHIP_LIB = the emulation,
PCLHIP_ALLOW_WAVESIM=1, in a subprocess).  The whole module takes a few seconds there, the 100,007-point case included: only
the torch-buffer case stays on the GPU.  The emulation's workgroups run on host threads and its atomics are the host's, so
the blocks' adds to count[h] really interleave here."""
import os
import shutil
import subprocess

import pytest

from test_cluster_wavesim import on_the_emulation

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


def test_sac_gpu_tests_on_the_emulation(wavesim_lib):
    on_the_emulation(wavesim_lib, "test_gpu_sac.py", GPU_ONLY)


def test_sac_regimes_on_the_emulation(wavesim_lib):
    """tests/test_gpu_sac_regimes.py: the `fullgrid` cases stay on the GPU as well -- their sizes follow the device's CU
    count, and with its 32 blocks the emulation reaches the scoring kernel's second tile at the sizes of the module above
    already"""
    on_the_emulation(wavesim_lib, "test_gpu_sac_regimes.py", GPU_ONLY + " and not fullgrid")
