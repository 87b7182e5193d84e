"""pclhip_mls_process / pcl_amd.MovingLeastSquares on the device against the numpy restatement (tests/mls_restatement.py),
which tests/test_mls_restatement.py holds to the reference's own criterion on bun0 (test/surface/
test_moving_least_squares.cpp:95-118) and to closed forms.

Per output record that the restatement does not exclude (kappa of about 1e10 and above; at most 1 % of a cloud):
  n_out, corresponding_input_indices and the neighbour count m    exactly
  the double point                                                 within (m + 32) * 2^-53 * kappa * r
  the double normal (up to sign) and curvature                     within (m + 32) * 2^-53 * kappa
  the float outputs                                                the float32 of the device's doubles, and within one
                                                                   float32 ulp of the restatement's value (float_ok)
The worst |d| / bound is printed before it is asserted.  Every case runs twice and the two results are compared bytewise."""
import ctypes as C

import numpy as np
import pytest

import mls_restatement as mr

pytestmark = pytest.mark.gpu
NONE, SIMPLE, ORTHOGONAL = mr.NONE, mr.SIMPLE, mr.ORTHOGONAL
BUN0_RADII = {0.03: (397, 397), 0.01: (380, 163), 0.0075: (234, 11)}  # radius -> (outputs, with a fit)


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def bun0():
    return mr.load_bun0()


@pytest.fixture(scope="module")
def bun0_restated(bun0):
    return {r: mr.restate(bun0, r) for r in BUN0_RADII}


def smoother(gpu, pts, r, sqr_gauss_param=None, order=2, method=SIMPLE, normals=True, tree=None):
    import pcl_amd
    s = pcl_amd.MovingLeastSquares(gpu)
    if tree is not None:
        s.setSearchMethod(tree)
    s.setInputCloud(pts)
    s.setSearchRadius(r)
    if sqr_gauss_param is not None:
        s.setSqrGaussParam(sqr_gauss_param)
    s.setPolynomialOrder(order)
    s.setProjectionMethod(method)
    s.setComputeNormals(normals)
    return s


def run(gpu, pts, r, **kw):
    """-> (points, normals, curvature, indices, doubles) as numpy; the call is made twice, the bytes must agree"""
    s = smoother(gpu, pts, r, **kw)
    a = s.processAll()
    a = tuple(None if x is None else np.array(x) for x in a)
    b = s.processAll()
    for x, y in zip(a, b):
        assert (x is None and y is None) or x.tobytes() == np.asarray(y).tobytes()
    p, n, c, i, d = a
    k = len(i)
    assert p.dtype == np.float32 and p.shape == (k, 3) and i.dtype == np.int32 and d.dtype == np.float64 and d.shape == (k, 8)
    assert n is None or (n.dtype == np.float32 and n.shape == (k, 3) and c.shape == (k,))
    assert np.array_equal(np.asarray(s.getCorrespondingIndices()), i)
    return a


def float_ok(got, want64, bound):
    """float32 `got` against the float32 of `want64`: one float32 ulp apart at most -- the doubles agree within `bound`, far
    below half an ulp, so only a rounding boundary can separate the floats.  (Where the value is so close to 0 that its ulp
    is below the doubles' own bound -- a curvature of 1e-17, a normal component of 1e-20 -- that bound is what is left.)"""
    want = np.asarray(want64, np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    bound = np.asarray(bound, np.float64).reshape((-1,) + (1,) * (want.ndim - 1))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp + bound


def check(out, ref, label, max_excluded=0.01):
    """the contract of the module's docstring -> the worst |d| / bound over point, normal and curvature"""
    p, n, c, idx, d = out
    assert len(idx) == len(ref["indices"]), (label, len(idx), len(ref["indices"]))
    assert np.array_equal(idx, ref["indices"])
    assert np.array_equal(d[:, 7], ref["m"].astype(np.float64))
    k = len(idx)
    keep = ~ref["excluded"]
    print("%s: %d records, %d with a fit, %d excluded" % (label, k, int(ref["fitted"].sum()), int((~keep).sum())))
    if max_excluded is not None:
        assert (~keep).sum() <= max_excluded * k
    assert np.isfinite(d).all()
    # the floats are the device's own doubles, rounded once
    assert np.array_equal(p, d[:, :3].astype(np.float32))
    if n is not None:
        assert np.array_equal(n, d[:, 3:6].astype(np.float32)) and np.array_equal(c, d[:, 6].astype(np.float32))
    assert (np.abs(np.linalg.norm(d[:, 3:6], axis=1) - 1.0) <= 8 * mr.U).all()
    if not keep.any():
        return 0.0
    dp = np.abs(d[:, :3] - ref["point"]).max(axis=1)[keep]
    dn = mr.normal_delta(d[:, 3:6], ref["normal"])[keep]
    dc = np.abs(d[:, 6] - ref["curvature"])[keep]
    ratios = [float((dp / ref["bound_point"][keep]).max()), float((dn / ref["bound_unit"][keep]).max()),
              float((dc / ref["bound_unit"][keep]).max())]
    print("%s: worst |d| / bound: point %.4f, normal %.4f, curvature %.4f" % ((label,) + tuple(ratios)))
    assert max(ratios) <= 1.0, (label, ratios)
    sign = np.where((d[:, 3:6] * ref["normal"]).sum(axis=1) < 0, -1.0, 1.0)[:, None]
    assert float_ok(p, ref["point"], ref["bound_point"])[keep].all()
    if n is not None:
        assert float_ok(n, sign * ref["normal"], ref["bound_unit"])[keep].all()
        assert float_ok(c, ref["curvature"], ref["bound_unit"])[keep].all()
    return max(ratios)


def sign_rule_holds(normals):
    """the component of largest magnitude is positive (ties: the lowest axis)"""
    lead = np.argmax(np.abs(normals), axis=1)
    return (normals[np.arange(len(normals)), lead] > 0).all()


@pytest.mark.parametrize("r", sorted(BUN0_RADII))
def test_bun0(gpu, bun0, bun0_restated, r):
    """r = 0.03: every point fitted; 0.01: records dropped (the compaction) and plane-only and fitted lanes in one wavefront;
    0.0075: almost no fits (whole groups skip the fit walk)"""
    ref = bun0_restated[r]
    assert (len(ref["indices"]), int(ref["fitted"].sum())) == BUN0_RADII[r]
    out = run(gpu, bun0, r)
    check(out, ref, "bun0 r=%g" % r)
    if r == 0.03:  # the reference's own criterion on record 0
        p, n, c = out[0], out[1], out[2]
        assert np.abs(p[0] - mr.BUN0_POINT0).max() <= 1e-3 and np.abs(np.abs(n[0]) - mr.BUN0_ABS_NORMAL0).max() <= 1e-3
        assert abs(c[0] - mr.BUN0_CURVATURE0) <= 1e-3
        s = smoother(gpu, bun0, r)
        s.process()
        a, b = s.lastPassMs()
        assert a >= 0.0 and b >= 0.0 and s.lastKernelMs() >= 0.0


@pytest.mark.parametrize("r", [0.03, 0.01])
def test_orders_and_methods(gpu, bun0, bun0_restated, r):
    """orders 0 and 1 and the method NONE give the plane record, bit for bit the same one; its sign obeys the rule and the
    fitted normal stays on its side"""
    full = bun0_restated[r]
    plane = dict(full, point=full["plane_point"], normal=full["plane_normal"])
    outs = [run(gpu, bun0, r, order=o, method=m) for o, m in ((0, SIMPLE), (1, SIMPLE), (2, NONE), (0, NONE))]
    check(outs[0], plane, "bun0 r=%g plane" % r)
    for o in outs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o, outs[0]))
    assert sign_rule_holds(outs[0][4][:, 3:6])
    fitted = run(gpu, bun0, r)
    assert ((fitted[4][:, 3:6] * outs[0][4][:, 3:6]).sum(axis=1) > 0).all()
    moved = (fitted[4][:, :3] != outs[0][4][:, :3]).any(axis=1)
    assert np.array_equal(moved, full["fitted"])  # (a fit that moves nothing would need coeff[0] == 0)
    assert np.array_equal(fitted[4][:, 6:], outs[0][4][:, 6:])  # curvature and m are the plane's


@pytest.mark.parametrize("factor", [0.25, 4.0])
def test_sqr_gauss_param(gpu, bun0, bun0_restated, factor):
    r = 0.03
    ref = mr.restate(bun0, r, sqr_gauss_param=factor * r * r)
    assert np.abs(ref["point"] - bun0_restated[r]["point"]).max() > 1e-6  # the weights matter
    check(run(gpu, bun0, r, sqr_gauss_param=factor * r * r), ref, "bun0 sqr_gauss_param = %g r^2" % factor)


def test_normals_off(gpu, bun0):
    on, off = run(gpu, bun0, 0.01), run(gpu, bun0, 0.01, normals=False)
    assert off[1] is None and off[2] is None
    assert on[0].tobytes() == off[0].tobytes() and on[3].tobytes() == off[3].tobytes() and on[4].tobytes() == off[4].tobytes()


def test_neighbour_count_edges(gpu):
    """isolated groups of 2, 3, 5 and 6 points and a lone point: the outputs are the groups of 3 and more, only the group of
    6 is fitted"""
    pts, size = mr.edge_groups()
    ref = mr.restate(pts, 1.0)
    assert np.array_equal(ref["m_all"], size)
    assert np.array_equal(ref["indices"], np.nonzero(size >= 3)[0]) and np.array_equal(ref["fitted"], ref["m"] == 6)
    out = run(gpu, pts, 1.0)
    check(out, ref, "groups")
    plane = run(gpu, pts, 1.0, method=NONE)
    assert np.array_equal((out[4][:, :3] != plane[4][:, :3]).any(axis=1), ref["m"] == 6)


def test_torch_device_buffers(gpu, bun0):
    import torch
    t = torch.from_numpy(bun0).cuda()
    s = smoother(gpu, t, 0.01)
    p, n, c, i, d = s.processAll()
    assert p.is_cuda and n.is_cuda and c.is_cuda and i.is_cuda and d.is_cuda and i.dtype == torch.int32
    host = run(gpu, bun0, 0.01)
    for a, b in zip((p, n, c, i, d), host):
        assert a.cpu().numpy().tobytes() == b.tobytes()


def raw_call(lib, tree, r, capacity, sg=None, order=2, method=SIMPLE, pts=None, nrm=None, idx=None, dbl=None):
    k = C.c_uint64(12345)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    st = lib.pclhip_mls_process(tree.h, r, r * r if sg is None else sg, order, method, ptr(pts), ptr(nrm), ptr(idx), capacity,
                                C.byref(k), ptr(dbl))
    return st, int(k.value)


def test_capacity_and_optional_outputs(gpu, bun0):
    import pcl_amd
    from pcl_amd import _lib
    lib = _lib.load()
    r = 0.01
    full = run(gpu, bun0, r)
    tree = pcl_amd.KdTree(gpu)
    tree.setInputCloud(bun0)
    # capacity 0 and no buffer at all: the count alone, reported as an overflow
    assert raw_call(lib, tree, r, 0) == (-5, 380)
    # one short: 379 records are written, nothing behind them
    pts, nrm = np.full((380, 3), -7, np.float32), np.full((380, 4), -7, np.float32)
    idx, dbl = np.full(380, -7, np.int32), np.full((380, 8), -7, np.float64)
    assert raw_call(lib, tree, r, 379, pts=pts, nrm=nrm, idx=idx, dbl=dbl) == (-5, 380)
    assert pts[:379].tobytes() == full[0][:379].tobytes() and (pts[379] == -7).all()
    assert idx[:379].tobytes() == full[3][:379].tobytes() and idx[379] == -7
    assert dbl[:379].tobytes() == full[4][:379].tobytes() and (dbl[379] == -7).all() and (nrm[379] == -7).all()
    # exact, and every output on its own
    for which in range(4):
        pts, nrm = np.full((381, 3), -7, np.float32), np.full((381, 4), -7, np.float32)
        idx, dbl = np.full(381, -7, np.int32), np.full((381, 8), -7, np.float64)
        bufs = [pts, nrm, idx, dbl]
        args = dict(zip(("pts", "nrm", "idx", "dbl"), [b if j == which else None for j, b in enumerate(bufs)]))
        assert raw_call(lib, tree, r, 380, **args) == (0, 380)
        want = [full[0], np.concatenate([full[1], full[2][:, None]], axis=1), full[3], full[4]][which]
        assert bufs[which][:380].tobytes() == want.tobytes() and (bufs[which][380] == -7).all()
    s = smoother(gpu, bun0, r, tree=tree)
    assert s.process()[0].tobytes() == full[0].tobytes() and s.getSearchMethod() is tree


def test_output_feeds_point_to_plane_icp(gpu, bun0):
    """the hand-off: the smoothed bun0 with the MLS normals as the target of IterativeClosestPointWithNormals -- a fitness no
    worse than with NormalEstimation's normals on the same pair (a smoke test of the hand-off, no parity bar)"""
    import pcl_amd
    p, n, c, idx, _ = run(gpu, bun0, 0.03)
    assert len(p) == 397
    th = 0.05
    T = np.eye(4, dtype=np.float32)
    T[0, 0] = T[1, 1] = np.cos(th)
    T[0, 1], T[1, 0] = -np.sin(th), np.sin(th)
    T[:3, 3] = (0.004, -0.003, 0.002)
    src = np.ascontiguousarray((p.astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]).astype(np.float32))

    def fitness(normals):
        tree = pcl_amd.KdTree(gpu)
        tree.setInputCloud(p)
        if normals is None:
            ne = pcl_amd.NormalEstimation(gpu)
            ne.setSearchMethod(tree)
            ne.setInputCloud(p)
            ne.setKSearch(10)
            ne.compute()
        else:
            tree.setNormals(normals)
        icp = pcl_amd.IterativeClosestPointWithNormals(gpu)
        icp.setSearchMethodTarget(tree, True)
        icp.setInputSource(src)
        icp.setMaximumIterations(30)
        icp.setMaxCorrespondenceDistance(0.05)
        icp.align()
        assert icp.hasConverged()
        return icp.getFitnessScore()

    with_mls, with_ne = fitness(n), fitness(None)
    print("fitness: MLS normals %.3e, NormalEstimation normals %.3e" % (with_mls, with_ne))
    # the source is the target moved rigidly: both runs end at the rounding floor of the float32 coordinates (|x| < 0.2, a
    # mean squared distance below (1e-6)^2), where their order means nothing
    assert with_mls <= max(with_ne, 1e-12)
