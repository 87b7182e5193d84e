"""The oracle's plane fit can report the path it took (orc_solve_plane_parameters_path, oracle/pcl_oracle.c): the record
is written by the very functions that compute the normal, so asking for it must change no bit of the result, and the
covariances below must reach every value a field can take -- tests/test_gpu_normals_regimes.py picks its rows by them."""
import numpy as np
import pytest

FLT_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


def covariances():
    rng = np.random.default_rng(20)
    out = []
    for _ in range(2500):  # full rank, any scale
        a = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3)
        out.append(a @ a.T)
    for _ in range(600):   # one or two directions squeezed: planes and lines to within rounding
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        d = np.array([1.0, rng.uniform(0, 1), rng.uniform(0, 1)]) * np.array([1.0, rng.choice([1.0, 1e-4, 1e-9, 0.0]),
                                                                               rng.choice([1e-4, 1e-9, 0.0])])
        out.append((q * d) @ q.T * 10.0 ** rng.uniform(-2, 2))
    for axis in range(3):  # exact planes, lines and points along the axes, at ordinary and at (sub)normal-edge scales
        for s in (1.0, 0.25, 3e-38, 1e-40, 1e-45):
            line = np.zeros((3, 3))
            line[axis, axis] = s
            plane = np.eye(3) * s
            plane[axis, axis] = 0.0
            out += [line, plane, np.eye(3) * s]
    out += [np.zeros((3, 3)), np.full((3, 3), 0.5), np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0.0]]),
            np.array([[1, 0, 1], [0, 0, 0], [1, 0, 1.0]]), np.diag([1.0, 1.0, 1e-9]), np.diag([-1.0, 1.0, 0.0]),
            np.diag([1.0, 2.0, -3.0])]  # the last: trace 0 with a nonzero matrix
    return [np.asarray(c, np.float32) for c in out]


def test_the_path_record_changes_no_bit_and_every_path_is_reached(orc):
    seen = {name: set() for name in ("roots_path", "eigvec_branch", "orthogonal_arm", "scale_small", "eig_sum_zero")}
    covs = covariances()
    assert len(covs) > 3000
    for cov in covs:
        plain = np.asarray(orc.solve_plane_parameters(cov), np.float32)
        traced, rec = orc.solve_plane_parameters_path(cov)
        assert np.array_equal(plain.view(np.uint32), np.asarray(traced, np.float32).view(np.uint32)), cov
        for name in seen:
            seen[name].add(rec[name])
        # the record agrees with what it describes
        assert rec["eigvec_branch"] == (1 if rec["gap10"] > FLT_EPS else 2 if rec["gap20"] > FLT_EPS else 3), rec
        assert (rec["orthogonal_arm"] != 0) == (rec["eigvec_branch"] == 2), rec
        assert rec["scale_small"] == int(np.abs(cov).max() <= np.finfo(np.float32).tiny), rec
        assert rec["eig_sum_zero"] == int(np.float32(np.float32(cov[0, 0] + cov[1, 1]) + cov[2, 2]) == 0), rec
        if rec["eigvec_branch"] == 3:
            assert traced[:3] == (1.0, 0.0, 0.0)
        if rec["orthogonal_arm"] == 1:
            assert traced[2] == 0.0
        if rec["orthogonal_arm"] == 2:
            assert traced[0] == 0.0
        if rec["eig_sum_zero"]:
            assert traced[3] == 0.0
    assert seen["roots_path"] == {orc.ROOTS_C0, orc.ROOTS_TRIG, orc.ROOTS_TRIG_FALLBACK}
    assert seen["eigvec_branch"] == {1, 2, 3}
    assert seen["orthogonal_arm"] == {0, 1, 2}
    assert seen["scale_small"] == {0, 1} and seen["eig_sum_zero"] == {0, 1}


def test_plane_fit_lists_is_the_per_point_fit_of_the_normals_pass(orc):
    """orc_plane_fit_lists on the neighbour lists of orc_normals_knn gives that pass's normals before the viewpoint flip"""
    rng = np.random.default_rng(21)
    pts = rng.random((500, 3)).astype(np.float32)
    pts[40:60] = pts[40]          # coincident points: the constant branch
    pts[7] = np.nan
    want, knn, nan = orc.KdTree(pts).normals(pts, 8, viewpoint=(0.5, 0.5, 9.0), want_knn=True)
    fit, rec = orc.plane_fit_lists(pts, knn)
    assert nan == 1 and np.isnan(fit[7]).all() and rec["roots_path"][7] == orc.ROOTS_NONE
    ok = ~np.isnan(want[:, 0])
    assert np.array_equal(np.abs(fit[ok]).view(np.uint32), np.abs(want[ok]).view(np.uint32))
    assert (rec["eigvec_branch"][40:60] == 3).all() and (rec["eig_sum_zero"][40:60] == 1).all()
    short = np.full((2, 8), -1, np.int32)
    short[1, :2] = (3, 4)
    fit2, rec2 = orc.plane_fit_lists(pts, short)
    assert np.isnan(fit2).all() and (rec2["roots_path"] == orc.ROOTS_NONE).all()
