"""The far-from-the-origin cases in the CPU tier: the `-m gpu` tests of tests/test_gpu_far_clouds.py run on the wavefront
emulation of tests/wavesim (the recipe of tests/test_mls_wavesim.py: PCLHIP_LIB = the emulation, PCLHIP_ALLOW_WAVESIM=1, in a
subprocess).  Every case of the module runs: none needs device buffers or a large index."""
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


def test_far_cloud_gpu_tests_on_the_emulation(wavesim_lib):
    env = dict(os.environ, PCLHIP_LIB=wavesim_lib, PCLHIP_ALLOW_WAVESIM="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(ROOT, "tests", "test_gpu_far_clouds.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, tail
    assert " deselected" not in r.stdout, tail
