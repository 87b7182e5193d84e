"""pclhip_solve_transformation(sums, POINT_TO_POINT) -- the host instantiation of cf::rotation_from_sigma -- over every rank
and symmetry of the cross-covariance (tests/solver_reference.py: the regimes, the fp64 reference, what is asserted), and the
same judgement of the oracle's umeyama.  CPU tier: the solve is host code.

Until this module the suite showed the solver full-rank, well-conditioned sums only, and it returned matrices that are no
rotations for planes and lines (HISTORY.md, "the point-to-point solve on planes and lines": max|R^T R - I| up to 0.89 over
the sweep below, 36 of this module's tests failing)."""
import ctypes as C

import numpy as np
import pytest

import solver_reference as sr

CASES = sr.cases()
SWEEP = sr.sweep()


def product_solve(case, mode=0):
    from pcl_amd import _lib
    sums = sr.sums_of(case.src, case.tgt)
    T = np.zeros(16, np.float32)
    assert _lib.load().pclhip_solve_transformation(sums.ctypes.data_as(C.POINTER(C.c_double)), mode,
                                                   T.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return T.reshape(4, 4)


def oracle_solve(case):
    from oracle import pcl_oracle as orc
    return orc.umeyama(case.src, case.tgt, acc_double=True)


SOLVERS = {"product": product_solve, "oracle": oracle_solve}


def test_every_case_is_in_the_regime_it_names():
    for case in CASES + SWEEP:
        sr.in_regime(case)
    # the five thicknesses, five seeds each, of either shape; the shapes of the issue are all here
    assert sum(c.regime == "slab" and c.frame == "unit" for c in CASES) == 25 and sum(c.regime == "rod" for c in CASES) == 25
    assert len(SWEEP) == 300 and all(len(c.src) == 200 for c in SWEEP)


@pytest.mark.parametrize("solver", ["product", "oracle"])
@pytest.mark.parametrize("case", CASES, ids=[c.name.replace(" ", "_") for c in CASES])
def test_solve(case, solver):
    sr.check(SOLVERS[solver](case), case)


@pytest.mark.parametrize("solver", ["product", "oracle"])
def test_sweep_of_tilted_planes(solver):
    bad = {}
    worst = {"orth": 0.0, "det": 0.0, "excess": -1.0, "diff": 0.0}
    for case in SWEEP:
        f, j = sr.failures(SOLVERS[solver](case), case)
        if f:
            bad[case.name] = f
        for k in worst:
            worst[k] = max(worst[k], j[k])
    print("%s, %d planes: %d fail; worst max|R^T R - I| = %.3g B, |det R - 1| = %.3g B, residual excess = %.3g B M, max|T - K| = %.3g"
          % (solver, len(SWEEP), len(bad), worst["orth"] / sr.B, worst["det"] / sr.B, worst["excess"] / sr.B, worst["diff"]))
    assert not bad, (len(bad), sorted(bad.items())[:5])


def group_of(case):
    return case.name.split(" seed ")[0]


@pytest.mark.parametrize("solver", ["product", "oracle"])
def test_worst_figures_per_regime(solver):
    """Prints, per regime, the worst orthogonality defect as a fraction of B, the worst residual excess as a fraction of B M
    and the worst max|T - K| (of R alone for a scaled cloud; `-` where the rotation is not determined), then asserts."""
    rows, bad = {}, {}
    for case in CASES:
        f, j = sr.failures(SOLVERS[solver](case), case)
        if f:
            bad[case.name] = f
        r = rows.setdefault(group_of(case), [0.0, -1.0, None])
        r[0], r[1] = max(r[0], j["orth"] / sr.B), max(r[1], j["excess"] / sr.B)
        if j["determined"] and case.frame != "offset":
            r[2] = max(r[2] or 0.0, j["diff"] if case.frame == "unit" else j["diff_R"])
    print("\n%-34s %14s %14s %12s   (%s)" % ("regime", "orth / B", "excess / (B M)", "max|T - K|", solver))
    for name, (o, e, d) in rows.items():
        print("%-34s %14.3g %14.3g %12s" % (name, o, e, "-" if d is None else "%.3g" % d))
    print("worst of all: orth %.3g B, excess %.3g B M, max|T - K| %.3g"
          % (max(r[0] for r in rows.values()), max(r[1] for r in rows.values()), max(r[2] or 0.0 for r in rows.values())))
    assert not bad, (len(bad), sorted(bad.items())[:5])


def test_exactly_singular_normal_system_gives_nan():
    """Point-to-plane and symmetric sums against an axis-aligned plane whose normals are all (0, 0, 1): the columns of the
    rotation about z and of the translations along x and y are exactly zero, cf::lu_solve6 finds no pivot, and the twelve
    upper entries are NaN (Eigen's inverse() of the reference yields non-finite too); the last row stays (0, 0, 0, 1)."""
    from oracle import pcl_oracle as orc
    from pcl_amd import _lib
    rng = np.random.default_rng(3)
    src = np.zeros((200, 4), np.float32)
    src[:, :2] = rng.integers(-20, 21, (200, 2))
    src[:, 3] = 1
    tgt = src.copy()
    tgt[:, 2] = 0.5
    nrm = np.zeros((200, 3), np.float32)
    nrm[:, 2] = 1
    for mode, s27 in ((_lib.POINT_TO_PLANE, orc.lls_point_to_plane(src, tgt, nrm)[1]),
                      (_lib.SYMMETRIC, orc.lls_symmetric(src, nrm, tgt, nrm)[1])):
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = s27[:21]
        assert (A[2] == 0).all() and (A[:, 2] == 0).all() and np.linalg.matrix_rank(A) == 3
        sums = np.zeros(_lib.NSUMS)
        sums[:27] = s27
        sums[28] = 200
        T = np.zeros(16, np.float32)
        assert _lib.load().pclhip_solve_transformation(sums.ctypes.data_as(C.POINTER(C.c_double)), mode,
                                                       T.ctypes.data_as(C.POINTER(C.c_float))) == 0
        T = T.reshape(4, 4)
        assert np.isnan(T[:3]).all() and np.array_equal(T[3], [0, 0, 0, 1]), (mode, T)
