"""The NDT tests' CPU restatement (tests/ndt_restatement.py) pinned on the reference's own NDT test
(test/registration/test_ndt.cpp:53-97): bun0 -> bun4, resolution 0.025, step size 0.05, 50 iterations, epsilon 1e-8,
getFitnessScore() < 0.001 -- and on the pieces the device tests lean on."""
import numpy as np

import ndt_restatement as rs


def test_restatement_passes_the_reference_test(bunny):
    src, tgt = bunny["bun0"], bunny["bun4"]
    first = None
    for _ in range(5):  # the reference aligns five times over (the search-method setters do not reach NDT)
        reg = rs.NDT(tgt, src, resolution=0.025, step_size=0.05, transformation_epsilon=1e-8, max_iterations=50)
        out = reg.align()
        assert out["converged"] and rs.fitness(tgt, src, out["T"]) < 0.001
        first = out if first is None else first
        assert np.array_equal(out["T"], first["T"])
    assert len(reg.cells["npoints"]) == 32 and reg.cells["valid"].all()
    assert first["nr_iterations"] == 17 and sum(first["trials"]) >= 1  # a line search iterates: computeHessian is covered


def test_sums_are_the_sums_of_the_pair_terms(bunny):
    src, tgt = bunny["bun0"], bunny["bun4"]
    reg = rs.NDT(tgt, src, resolution=0.025)
    x = np.array([0.004, -0.003, 0.002, 0.05, -0.04, 0.03])
    tc = rs.transform_se3(rs.convert_transform(x), reg.src)
    pi, ci = reg.search.pairs(tc)
    # the neighbours against brute force
    d = tc[:, None, :] - reg.cells["centroids"][None, :, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    bp, bc = np.nonzero(d2 < np.float32(float(np.float32(0.025)) ** 2))
    assert sorted(zip(pi.tolist(), ci.tolist())) == sorted(zip(bp.tolist(), bc.tolist())) and len(pi) > 100
    s, g, H = rs.derivative_sums(x, reg.src, tc, pi, ci, reg.cells["means"], reg.cells["icov"], reg.d1, reg.d2)
    ts, tg, tH = rs.pair_terms(x, reg.src, tc, pi, ci, reg.cells["means"], reg.cells["icov"], reg.d1, reg.d2)
    assert abs(s - ts.sum()) <= 1e-13 * np.abs(ts).sum()
    assert np.all(np.abs(g - tg.sum(0)) <= 1e-13 * np.abs(tg).sum(0))
    assert np.all(np.abs(H - tH.sum(0)) <= 1e-13 * np.abs(tH).sum(0) + 1e-300)
    # the gradient is the derivative of the score, the Hessian that of the gradient (central differences in x)
    def at(y):
        # (fixed pairs and a double transform: the float rounding of T would drown a 1e-6 step)
        R = np.eye(4)
        R[:3, :3] = rot(y[3], 0) @ rot(y[4], 1) @ rot(y[5], 2)
        R[:3, 3] = y[:3]
        tcy = reg.src.astype(np.float64) @ R[:3, :3].T + R[:3, 3]
        return rs.derivative_sums(y, reg.src, tcy, pi, ci, reg.cells["means"], reg.cells["icov"], reg.d1, reg.d2)

    def rot(a, ax):
        c, s_ = np.cos(a), np.sin(a)
        u, v = (ax + 1) % 3, (ax + 2) % 3
        R = np.eye(3)
        R[u, u] = R[v, v] = c
        R[u, v], R[v, u] = -s_, s_
        return R
    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        (sp, gp, _), (sm, gm, _) = at(x + e), at(x - e)
        assert abs((sp - sm) / (2 * h) - g[k]) <= 1e-5 * np.abs(g).max()
        assert np.all(np.abs((gp - gm) / (2 * h) - H[k]) <= 1e-5 * np.abs(H).max())


def test_float_forms_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(20):
        x = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-1.2, 1.2, 3)])
        T = rs.convert_transform(x)
        y = rs.euler_from(T)  # the same rotation, possibly through Eigen's other branch (roll in [0, pi])
        assert np.abs(rs.convert_transform(y) - T).max() < 5e-7
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 5e-7
    assert np.array_equal(rs.euler_from(np.eye(4, dtype=np.float32)), np.zeros(6))
    assert np.array_equal(rs.convert_transform(np.zeros(6)), np.eye(4, dtype=np.float32))
