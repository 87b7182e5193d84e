"""SampleConsensusModelCylinder and RandomSampleConsensus in the CPU tier: the `-m gpu` tests of
tests/test_gpu_sac_cylinder.py and tests/test_gpu_sac_cylinder_regimes.py run on the wavefront emulation of tests/wavesim
(the recipe of tests/test_sac_models_wavesim.py).  Both modules take seconds there: only the torch-buffer case and the case
sized from the device's CU count stay on the GPU.  The double acos and sqrt are the host's here, the ballots and the lane
masks of the scoring pass are the emulation's."""
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


def test_sac_cylinder_gpu_tests_on_the_emulation(wavesim_lib):
    on_the_emulation(wavesim_lib, "test_gpu_sac_cylinder.py", GPU_ONLY)


def test_sac_cylinder_regimes_on_the_emulation(wavesim_lib):
    on_the_emulation(wavesim_lib, "test_gpu_sac_cylinder_regimes.py", GPU_ONLY + " and not fullgrid")
