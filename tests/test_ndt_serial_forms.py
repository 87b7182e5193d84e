"""The serial step of NormalDistributionsTransform beside its restatement, directly: nf::mt_trial_value,
nf::mt_update_interval and nf::svd_solve6 of pcl_amd/csrc/ndt_forms.hpp are host code, so a test-only shared object
(tests/ndt_serial_forms.cpp, built here with the host clang++ and the flags of the wavefront emulation) puts them next to
tests/ndt_restatement.py's trial_value / update_interval / svd_solve.

Why directly: case 3 of trialValueSelectionMT (impl/ndt.hpp:665-776) is reached by no alignment tried so far (the suite's
three, the three of tests/test_gpu_ndt_regimes.py, four more on the sheet with step sizes 0.005 to 0.02 near the optimum),
and cases 2 and 4 only a few times; the rank test of the Newton direction never drops a singular value on those inputs either."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ndt_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    if not os.path.exists(CLANG) or shutil.which("make") is None:
        pytest.skip("needs the ROCm clang++ and make")  # the condition of the emulation's own tests
    so = str(tmp_path_factory.mktemp("ndt_serial_forms") / "libndt_serial_forms.so")
    cmd = [CLANG, "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden", "-DPCLHIP_WAVESIM",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "tests", "wavesim"), "-I" + os.path.join(ROOT, "pcl_amd", "csrc"),
           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-Wno-unknown-pragmas", "-Wno-pass-failed",
           "-include", "wavesim.hpp", "-x", "c++", os.path.join(ROOT, "tests", "ndt_serial_forms.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(so)
    lib.ndt_test_trial_value.restype = C.c_double
    lib.ndt_test_trial_value.argtypes = [DP, C.c_double, C.c_double, C.c_double]
    lib.ndt_test_update_interval.restype = C.c_int
    lib.ndt_test_update_interval.argtypes = [DP, C.c_double, C.c_double, C.c_double]
    lib.ndt_test_svd_solve6.restype = None
    lib.ndt_test_svd_solve6.argtypes = [DP, DP, DP]
    return lib


KEYS = ("a_l", "f_l", "g_l", "a_u", "f_u", "g_u")


def interval_states(n=20000, seed=51):
    """Interval states and trials as a line search meets them: step lengths from a short grid (so that a_t == a_l and
    a_t == a_l == a_u occur), values and slopes of both signs and of magnitudes 1e-6 to 1, some slopes exactly 0 or exactly
    opposite to g_l."""
    rng = np.random.default_rng(seed)
    grid = np.array([0.0, 0.01, 0.025, 0.05, 0.0625, 0.1, 0.2, 0.5])
    for _ in range(n):
        a_l, a_u, a_t = rng.choice(grid, 3)
        mag = 10.0 ** rng.uniform(-6, 0, 6)
        f_l, f_u, f_t, g_l, g_u, g_t = rng.uniform(-1, 1, 6) * mag
        k = rng.integers(0, 12)
        if k == 0:
            g_t = 0.0
        elif k == 1:
            g_t = -g_l
        elif k == 2:
            g_t = g_l
        elif k == 3:
            f_t = f_l
        yield dict(a_l=a_l, f_l=f_l, g_l=g_l, a_u=a_u, f_u=f_u, g_u=g_u), float(a_t), float(f_t), float(g_t)


def sub_branch(S, a_t, f_t, g_t, case, value):
    """Which side of the case's own comparison the restatement took: told from the value it returned."""
    with np.errstate(all="ignore"):
        if case == 3:
            lim = a_t + 0.66 * (S["a_u"] - a_t)
            return ("up" if a_t > S["a_l"] else "down") + ("-lim" if value == lim else "-next")
        if case in (1, 2):
            z = np.float64(3 * (f_t - S["f_l"])) / np.float64(a_t - S["a_l"]) - g_t - S["g_l"]
            w = np.sqrt(np.float64(z * z - g_t * S["g_l"]))
            a_c = S["a_l"] + (a_t - S["a_l"]) * (w - S["g_l"] - z) / (g_t - S["g_l"] + 2 * w)
            return "cubic" if value == float(a_c) else "other"
    return "-"


def close(a, b):
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= 1e-15 * max(abs(a), abs(b))


def test_mt_trial_value_all_cases(forms):
    """nf::mt_trial_value against rs.trial_value on 20000 seeded states: equal to 1e-15 relative (NaN where the cubic's
    root is imaginary, on both sides).  The states cover the early return, cases 1, 2, 3 and 4, and within cases 1, 2 and
    3 both results of the case's own comparison (case 3: for a_t above and below a_l) -- asserted."""
    seen = {}
    for S, a_t, f_t, g_t in interval_states():
        case = rs.trial_case(S, a_t, f_t, g_t)
        want = rs.trial_value(dict(S), a_t, f_t, g_t)
        got = forms.ndt_test_trial_value((C.c_double * 6)(*[S[k] for k in KEYS]), a_t, f_t, g_t)
        assert close(got, want), (S, a_t, f_t, g_t, case, got, want)
        if not np.isnan(want):
            key = (case, sub_branch(S, a_t, f_t, g_t, case, want))
            seen[key] = seen.get(key, 0) + 1
    print("trial_value: (case, side) -> states: %s" % sorted(seen.items()))
    for key in [(0, "-"), (4, "-"), (1, "cubic"), (1, "other"), (2, "cubic"), (2, "other"), (3, "up-lim"), (3, "up-next"),
                (3, "down-lim"), (3, "down-next")]:
        assert seen.get(key, 0) >= 20, (key, seen)


def test_mt_update_interval_all_branches(forms):
    """nf::mt_update_interval against rs.update_interval: the same interval afterwards, bit for bit (it only moves values),
    and the same verdict, over the four exits (f_t > f_l; the slope times the distance positive, negative, zero)."""
    seen = {}
    for S, a_t, f_t, g_t in interval_states(seed=52):
        want = dict(S)
        conv = rs.update_interval(want, a_t, f_t, g_t)
        buf = (C.c_double * 6)(*[S[k] for k in KEYS])
        got_conv = forms.ndt_test_update_interval(buf, a_t, f_t, g_t)
        assert bool(got_conv) == conv and list(buf) == [want[k] for k in KEYS], (S, a_t, f_t, g_t)
        d = g_t * (S["a_l"] - a_t)
        key = "higher" if f_t > S["f_l"] else ("positive" if d > 0 else ("negative" if d < 0 else "zero"))
        assert (key == "zero") == conv
        seen[key] = seen.get(key, 0) + 1
    print("update_interval: exit -> states: %s" % sorted(seen.items()))
    assert all(seen.get(k, 0) >= 100 for k in ("higher", "positive", "negative", "zero")), seen


def test_svd_solve6_full_and_deficient_rank(forms):
    """nf::svd_solve6 (one-sided Jacobi) against rs.svd_solve (LAPACK's SVD), on definite, indefinite and rank-deficient
    Hessians of rank 5, 4 and 3 (B B^T: the dropped singular values are ~1e-17 of the largest, far under the 6 eps of
    Eigen's rank()), and on non-finite input.  Two SVDs of the same matrix agree in the solution to eps times the condition
    of the part they keep; that condition is at most 1e3 by construction (asserted), and the bar is 64 eps * condition *
    |delta| per solve.  Worst seen: 0.28 of the bar."""
    rng = np.random.default_rng(53)
    eps = np.finfo(np.float64).eps
    worst, ranks = 0.0, {}
    for trial in range(600):
        rank = (6, 6, 5, 4, 3)[trial % 5]
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        s = 10.0 ** rng.uniform(-3, 0, 6)
        if trial % 5 == 1:
            s[rng.integers(0, 6, 2)] *= -1  # indefinite
        s[rank:] = 0.0
        H = (Q * s) @ Q.T * 10.0 ** rng.uniform(-3, 6)
        H = (H + H.T) / 2
        b = rng.normal(size=6)
        want = rs.svd_solve(H, b)
        sv = np.linalg.svd(H, compute_uv=False)
        kept = sv[sv > sv.max() * 6 * eps]
        assert len(kept) == rank, (sv, rank)
        cond = kept.max() / kept.min()
        assert cond <= 1.001e3
        got = np.zeros(6)
        forms.ndt_test_svd_solve6(np.ascontiguousarray(H).ctypes.data_as(DP), b.ctypes.data_as(DP), got.ctypes.data_as(DP))
        err = np.abs(got - want).max() / (64 * eps * cond * np.abs(want).max())
        worst = max(worst, err)
        ranks[rank] = ranks.get(rank, 0) + 1
        assert err <= 1.0, (trial, rank, got, want)
    print("svd_solve6: solves by rank %s, worst error / bar %.3g" % (sorted(ranks.items()), worst))
    for bad in (np.nan, np.inf):
        H = np.eye(6)
        H[2, 3] = bad
        got = np.zeros(6)
        forms.ndt_test_svd_solve6(H.ctypes.data_as(DP), np.ones(6).ctypes.data_as(DP), got.ctypes.data_as(DP))
        assert np.isnan(got).all() and np.isnan(rs.svd_solve(H, np.ones(6))).all()
