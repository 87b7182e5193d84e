"""CorrespondenceRejectorSampleConsensus in the CPU tier: the `-m gpu` tests of tests/test_gpu_rejector_sac.py and
tests/test_gpu_rejector_sac_regimes.py run on the wavefront emulation of tests/wavesim (the recipe of
tests/test_sac_models_wavesim.py).  The first module takes seconds there, its largest size included, and none of its cases
needs torch: nothing is deselected.  Of the regimes only the device-buffer case (torch) and the case sized from the device's
CU count (fullgrid) stay on the GPU.  The replay's log and pow and the eigenvalues' cos, sin and atan2 are the host's
here, the ballots of the scoring pass and the atomics of the duplicate bitmaps are the emulation's."""
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


def test_rejector_sac_gpu_tests_on_the_emulation(wavesim_lib):
    on_the_emulation(wavesim_lib, "test_gpu_rejector_sac.py", GPU_ONLY)


def test_rejector_sac_regimes_on_the_emulation(wavesim_lib):
    on_the_emulation(wavesim_lib, "test_gpu_rejector_sac_regimes.py", GPU_ONLY + " and not fullgrid")
