"""The point-to-point solve (cf::rotation_from_sigma, pcl_amd/csrc/closed_forms.hpp) against a plain fp64 reference, over the
ranks and symmetries of the cross-covariance: numpy only, nothing of pcl_amd.

  optimum(src, tgt)   the Kabsch/umeyama optimum K from a two-pass covariance and np.linalg.svd, S = diag(1, 1,
                      sign(det U det V^T)); the singular values; that sign
  sums_of(src, tgt)   the reduction record pclhip_solve_transformation reads (tests/test_abi.py builds the same)
  judge(T, src, tgt)  what is asserted of every solve (below), measured
  check(T, case)      the assertions
  cases() / sweep()   the regimes; in_regime(case) asserts ON THE REFERENCE'S singular values that a case is in the regime
                      it names (the convention of tests/test_gpu_iss_regimes.py)

What is asserted, with B = 8 * 2^-24: each of the nine entries of R is a double rounded to float, off by at most 2^-25, and
at most 1 in magnitude, so R^T R - I is off by at most 6 * 2^-25 per entry; the rest of B is room for the double arithmetic.
  1. all 16 entries finite, the last row exactly (0, 0, 0, 1)
  2. max|R^T R - I| <= B and |det R - 1| <= 3 B
  3. rms residual of T over the pairs <= that of K + B * M, M the largest absolute coordinate of either cloud (the
     displacement that float rounding of the 4x4 alone can cause)
  4. where the rotation is determined and well conditioned (sv1/sv0 >= 1e-3, and a positive det U det V^T or
     sv1 - sv2 >= 1e-3 sv0): max|T - K| <= 2e-6 for unit-scale clouds at the origin, max|R - R_K| <= 2e-6 for scaled
     ones (the tolerance tests/test_abi.py holds this solver to on its quadric)."""
import collections

import numpy as np

B = 8 * 2.0 ** -24
TOL_K = 2e-6
NSUMS = 32

Optimum = collections.namedtuple("Optimum", "K sv sign")
Case = collections.namedtuple("Case", "name regime src tgt frame arg")  # frame: "unit" | "scaled" | "offset"


def _xyz(a):
    return np.asarray(a)[:, :3].astype(np.float64)


def optimum(src, tgt):
    s, t = _xyz(src), _xyz(tgt)
    sm, tm = s.mean(0), t.mean(0)
    sigma = (t - tm).T @ (s - sm) / len(s)
    U, sv, Vt = np.linalg.svd(sigma)
    sign = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, sign]) @ Vt
    K = np.eye(4)
    K[:3, :3] = R
    K[:3, 3] = tm - R @ sm
    return Optimum(K, sv, sign)


def sums_of(src, tgt):
    s, t = _xyz(src), _xyz(tgt)
    sums = np.zeros(NSUMS)
    sums[0:3] = s.sum(0)
    sums[3:6] = t.sum(0)
    sums[6:15] = (t.T @ s).reshape(9)
    sums[28] = len(s)
    return sums


def rms_residual(T, src, tgt):
    s, t = _xyz(src), _xyz(tgt)
    T = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.mean(np.sum((s @ T[:3, :3].T + T[:3, 3] - t) ** 2, axis=1))))


def determined(opt):
    sv = opt.sv
    return bool(sv[0] > 0 and sv[1] >= 1e-3 * sv[0] and (opt.sign > 0 or sv[1] - sv[2] >= 1e-3 * sv[0]))


def judge(T, src, tgt):
    """-> dict: well_formed; orth = max|R^T R - I| and det = |det R - 1|; excess = (rms of T - rms of K) / M;
    diff = max|T - K| and diff_R = max|R - R_K| with `determined`, whether assertion 4 applies."""
    T = np.asarray(T)
    T64 = T.astype(np.float64).reshape(4, 4)
    opt = optimum(src, tgt)
    R = T64[:3, :3]
    M = float(max(np.abs(_xyz(src)).max(), np.abs(_xyz(tgt)).max()))
    with np.errstate(all="ignore"):
        return {"well_formed": bool(np.isfinite(T64).all() and np.array_equal(T64[3], [0.0, 0.0, 0.0, 1.0])),
                "orth": float(np.abs(R.T @ R - np.eye(3)).max()), "det": float(abs(np.linalg.det(R) - 1.0)),
                "excess": (rms_residual(T64, src, tgt) - rms_residual(opt.K, src, tgt)) / (M if M > 0 else 1.0),
                "diff": float(np.abs(T64 - opt.K).max()), "diff_R": float(np.abs(R - opt.K[:3, :3]).max()),
                "determined": determined(opt), "M": M}


def failures(T, case):
    """the assertions of the module docstring that T misses for this case (empty: all hold), and the measurements"""
    j = judge(T, case.src, case.tgt)
    bad = []
    if not j["well_formed"]:
        bad.append("not finite, or a last row that is not (0, 0, 0, 1)")
    if not j["orth"] <= B:
        bad.append("max|R^T R - I| = %.3g = %.3g B" % (j["orth"], j["orth"] / B))
    if not j["det"] <= 3 * B:
        bad.append("|det R - 1| = %.3g = %.3g B" % (j["det"], j["det"] / B))
    if not j["excess"] <= B:
        bad.append("rms residual exceeds the optimum's by %.3g M = %.3g B M" % (j["excess"], j["excess"] / B))
    if j["determined"] and case.frame != "offset":
        d = j["diff"] if case.frame == "unit" else j["diff_R"]
        if not d <= TOL_K:
            bad.append("max|T - K| = %.3g" % d)
    return bad, j


def check(T, case):
    bad, j = failures(T, case)
    assert not bad, (case.name, bad)
    return j


# ---- the regimes --------------------------------------------------------------------------------------------------------------
THICKNESSES = (1e-3, 1e-5, 1e-6, 1e-7, 0.0)
SEEDS = (0, 1, 2, 3, 4)
SCALES = (1e-30, 1e-10, 1e10, 1e15)
OFFSETS = (1e2, 1e4)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def random_rotation(rng, most=3.0):
    return rotation(rng.normal(size=3), rng.uniform(0.0, most))


def _moved(p, R, t):
    """the pair (src, tgt) in float32, the motion applied to the float source in fp64"""
    src = np.ascontiguousarray(p, np.float32)
    tgt = np.ascontiguousarray(src.astype(np.float64) @ R.T + t, np.float32)
    return src, tgt


def box(rng, n, half):
    return rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(half, np.float64)


def ball(rng, n):
    p = rng.normal(size=(n, 3))
    return p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0, 1, (n, 1)) ** (1 / 3)


def tilted(rng, name, regime, p, arg=None, scale=1.0, offset=0.0, mirror=None, motion=None):
    """tilt p by a random rotation, (scale, move), round to float; the target is its image under a random rigid motion (of the
    mirrored source, if mirror is given: the pairs then are mirror images and the answer is still a proper rotation)"""
    p = (p @ random_rotation(rng).T) * scale + offset * np.array([1.0, -0.5, 0.25])
    R = random_rotation(rng) if motion is None else motion
    t = rng.uniform(-0.5, 0.5, 3) * scale
    src = np.ascontiguousarray(p, np.float32)
    image = src.astype(np.float64)
    if mirror is not None:
        c = image.mean(0)
        image = (image - c) * np.asarray(mirror, np.float64) + c
    tgt = np.ascontiguousarray(image @ R.T + t, np.float32)
    frame = "unit" if scale == 1.0 and offset == 0.0 else ("scaled" if offset == 0.0 else "offset")
    return Case(name, regime, src, tgt, frame, arg)


def lattice_plane():
    i, j = np.meshgrid(np.arange(-10.0, 10.0), np.arange(-5.0, 5.0), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), np.zeros(200)], axis=1)


def cases(n=200):
    out = []
    rng = lambda *key: np.random.default_rng([77, *key])
    # rank 3
    out.append(tilted(rng(1), "ball", "rank3", ball(rng(1, 1), n)))
    out.append(tilted(rng(2), "slab 1", "rank3", box(rng(2, 1), n, (1, 1, 1))))
    octa = np.concatenate([np.eye(3), -np.eye(3)])
    cube = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    out.append(tilted(rng(3), "octahedron", "equal3", octa))
    out.append(tilted(rng(4), "cube corners", "equal3", cube))
    out.append(tilted(rng(5), "octahedron, z halved", "equal01", octa * (1, 1, 0.5)))
    out.append(tilted(rng(6), "octahedron, x doubled", "equal12", octa * (2, 1, 1)))
    # rank 2 and rank 1: five thicknesses, five seeds each
    for k, th in enumerate(THICKNESSES):
        for seed in SEEDS:
            out.append(tilted(rng(10, k, seed), "slab %g seed %d" % (th, seed), "slab", box(rng(11, k, seed), n, (1, 1, th)), th))
            out.append(tilted(rng(12, k, seed), "rod %g seed %d" % (th, seed), "rod", box(rng(13, k, seed), n, (1, th, th)), th))
    p = lattice_plane()
    for name, R in (("z", np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])), ("x", np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]))):
        out.append(Case("lattice plane, 90 degrees about " + name, "exact2", *_moved(p, R, np.array([1.0, -2.0, 3.0])), "unit", None))
    out.append(tilted(rng(20), "three pairs", "rank2", box(rng(20, 1), 3, (1, 1, 1))))
    k = np.arange(-100.0, 100.0)
    out.append(Case("integer line", "exact1", *_moved(np.stack([k, 2 * k, -k], axis=1), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]),
                                                      np.array([1.0, -2.0, 3.0])), "unit", None))
    out.append(tilted(rng(21), "two pairs", "rank1", box(rng(21, 1), 2, (1, 1, 1))))
    # rank 0
    out.append(tilted(rng(22), "coincident points", "rank0", np.tile(box(rng(22, 1), 1, (1, 1, 1)), (n, 1))))
    out.append(tilted(rng(23), "one pair", "rank0", box(rng(23, 1), 1, (1, 1, 1))))
    # mirror images of an ellipsoid (its singular values apart, so that the answer is determined)
    for i, (name, m) in enumerate((("z -> -z", (1, 1, -1)), ("x -> -x", (-1, 1, 1)), ("inversion", (-1, -1, -1)))):
        out.append(tilted(rng(30, i), "mirror " + name, "mirror", ball(rng(31, i), n) * (1.0, 0.7, 0.5), mirror=m))
    # half turns
    for i, axis in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1), None)):
        r = rng(40, i)
        a = r.normal(size=3) if axis is None else axis
        out.append(tilted(r, "half turn about %s" % ("a random axis" if axis is None else "xyz"[i]), "rank3", ball(rng(41, i), n),
                          motion=rotation(a, np.pi)))
    # scale and offset: a ball and an exact plane
    for i, s in enumerate(SCALES):
        out.append(tilted(rng(50, i), "ball x %g" % s, "rank3", ball(rng(51, i), n), scale=s))
        out.append(tilted(rng(52, i), "plane x %g" % s, "slab", box(rng(53, i), n, (1, 1, 0)), 0.0, scale=s))
    for i, o in enumerate(OFFSETS):
        out.append(tilted(rng(60, i), "ball + %g" % o, "rank3", ball(rng(61, i), n), offset=o))
        out.append(tilted(rng(62, i), "plane + %g" % o, "far plane", box(rng(63, i), n, (1, 1, 0)), o, offset=o))
    assert len({c.name for c in out}) == len(out)
    return out


def sweep(count=300, n=200):
    """random tilted float planes (thickness exactly 0 before the tilt)"""
    return [tilted(np.random.default_rng([78, i]), "sweep %d" % i, "slab", box(np.random.default_rng([79, i]), n, (1, 1, 0)), 0.0)
            for i in range(count)]


def in_regime(case):
    """assert on the reference's singular values that the case is in the regime it names; -> the Optimum"""
    opt = optimum(case.src, case.tgt)
    s0, s1, s2 = opt.sv
    why = (case.name, opt.sv.tolist(), opt.sign)
    if case.regime == "rank0":  # the noise of a mean of equal numbers, squared
        M = float(np.abs(case.src).max())
        assert s0 <= 1e-12 * M * M and not determined(opt), why
        return opt
    r1, r2 = s1 / s0, s2 / s0
    th = case.arg
    # float rounding of the two clouds is 2^-24 of a coordinate each: 4e-15 in a product, less by the averaging
    noise = 1e-13
    if case.regime == "rank3":
        assert r2 >= 0.2 and opt.sign > 0, why
    elif case.regime == "equal3":
        assert s0 - s2 <= 1e-6 * s0 and opt.sign > 0, why
    elif case.regime == "equal01":
        assert s0 - s1 <= 1e-6 * s0 and 0.2 <= r2 <= 0.3, why
    elif case.regime == "equal12":
        assert s1 - s2 <= 1e-6 * s0 and 0.2 <= r1 <= 0.3, why
    elif case.regime == "mirror":
        assert opt.sign < 0 and r2 >= 0.1 and s1 - s2 >= 0.1 * s0, why
    elif case.regime == "slab":  # the variances are as 1 : 1 : th^2
        assert r1 >= 0.3 and r2 <= max(4 * th * th, noise), why
        assert th < 1e-6 or r2 >= th * th / 4, why
    elif case.regime == "far plane":  # a plane moved by th: float rounding makes a slab of relative thickness 2^-24 th of it
        assert r1 >= 0.3 and r2 <= (th * 2.0 ** -23) ** 2, why
    elif case.regime == "rod":
        assert r1 <= max(4 * th * th, noise) and r2 <= r1, why
        assert th < 1e-6 or r1 >= th * th / 8, why
    elif case.regime == "exact2":
        assert r1 >= 0.2 and r2 <= 1e-15, why
    elif case.regime == "rank2":
        assert r1 >= 1e-3 and r2 <= noise, why
    elif case.regime in ("exact1", "rank1"):
        assert r1 <= (1e-15 if case.regime == "exact1" else noise), why
    else:
        raise AssertionError("no such regime: %r" % (case.regime,))
    if case.regime in ("rank3", "equal3", "equal01", "equal12", "mirror", "slab", "far plane", "exact2", "rank2"):
        assert determined(opt), why
    else:
        assert not determined(opt), why
    return opt
