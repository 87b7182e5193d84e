"""The half-leaf resolve cases in the CPU tier: the `-m gpu` tests of tests/test_gpu_resolve_half.py run on the wavefront
emulation of tests/wavesim (the recipe of tests/test_far_clouds_wavesim.py: PCLHIP_LIB = the emulation,
PCLHIP_ALLOW_WAVESIM=1, in a subprocess).  Every case of the module runs at the shapes the device runs -- the shapes are the
smallest at which each path is taken, the emulation only makes them slower: the module takes about 30 s here on 16 cores,
its slowest case (five steps of the loop at 2^17 points: five alignments and five oracle searches) 11 s, every other
case under 4 s.

The seeded body's pipeline depth follows the groups per wave of the persistent grid; the emulation is built two deep from 2
groups per wave on and reports WAVESIM_CUS compute units (2 blocks each).  The module runs with 16 of them -- the loop
case two deep -- and the loop case once more with 1024: one deep."""
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


def run_module(lib, cus, expect_deep, only=None):
    env = dict(os.environ, PCLHIP_LIB=lib, PCLHIP_ALLOW_WAVESIM="1", WAVESIM_CUS=str(cus), PCLHIP_EXPECT_DEEP=expect_deep)
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"]
    if only:
        cmd += ["-k", only]
    cmd.append(os.path.join(ROOT, "tests", "test_gpu_resolve_half.py"))
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, tail
    return r.stdout


def test_resolve_half_gpu_tests_on_the_emulation(wavesim_lib):
    out = run_module(wavesim_lib, 16, "1")
    assert " deselected" not in out, out[-2000:]


def test_loop_case_with_the_one_deep_body_on_the_emulation(wavesim_lib):
    out = run_module(wavesim_lib, 1024, "0", only="pipeline_depth or five_steps_of_the_device_driven_loop")
    assert "2 passed" in out, out[-2000:]
