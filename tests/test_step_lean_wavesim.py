"""tests/test_gpu_step_lean.py on the CPU emulation of the wavefront (tests/wavesim; see tests/test_wavesim.py): the group
counters re-armed by the kernel that closes an iteration and the matches kept as positions, checked where no GPU exists.

The emulated device reports 2 compute units, so its grids hold 8 workgroups = 32 waves and a wave takes groups from the
counters from 64 groups on: with a 1k-point target the source "past the target's size" is 1025 points, and the interleaving
cases run at 4097 points (65 groups), the smallest size at which a counter left non-zero loses a group.  Launches are
synchronous in the emulation: what is checked here is the logic of the flag and of the kernels, not the order of the stream.
"""
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


def run_on_the_emulation(lib, keyword, timeout=1500):
    env = dict(os.environ, PCLHIP_LIB=lib, PCLHIP_ALLOW_WAVESIM="1", WAVESIM_CUS="2", PCLHIP_STEP_LEAN_TARGET="1024",
               PCLHIP_STEP_LEAN_FEED="4097")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", keyword,
           os.path.join(ROOT, "tests", "test_gpu_step_lean.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=timeout)
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, tail
    last = [ln for ln in r.stdout.splitlines() if " passed" in ln][-1]
    return int(last.split(" passed")[0].split()[-1])


def test_device_loop_sizes_on_the_emulation(wavesim_lib):
    # 7 source sizes x 2 modes: oracle pairs per iteration, the host-driven twin, restarts inside one queue
    assert run_on_the_emulation(wavesim_lib, "device_loop_equals_oracle_and_host_loop") == 14


def test_interleaving_on_the_emulation(wavesim_lib):
    # k-NN between two queues, two registrations stepped alternately, speculative launches behind a finished alignment
    assert run_on_the_emulation(wavesim_lib, "knn_between or stepped_alternately or speculative_launches") == 3


def test_match_readers_on_the_emulation(wavesim_lib):
    # ties on a lattice, OneToOne / reciprocal, GICP's pairs, served groups, empty and non-finite sources
    assert run_on_the_emulation(wavesim_lib, "lattice or one_to_one or gicp_pairs or served_groups or non_finite") == 5
