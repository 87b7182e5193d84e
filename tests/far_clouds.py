"""Clouds far from the origin for tests/test_far_clouds_restatement.py and tests/test_gpu_far_clouds.py.  A plain helper
module, not product code and no conftest.

  grid_sheet   a wavy sheet whose coordinates are multiples of 2^-10 in [0, 1]: every coordinate, and every difference of two,
               has at most 11 significant bits, so a move by multiples of 2^-10 below 2^13 and a scale by a power of two
               change no float of the cloud's geometry
  moved        the float32 sum with the exactness of the move asserted in both directions (the rule of
               tests/test_gpu_iss_regimes.py::test_shifted_cloud): the restatement of the UNMOVED cloud plus the shift is then
               the exact expectation for the moved one
  scaled       the same for a factor 2^e
  far_raw      the same surface at random float64 positions stored as float32 around (1500, -3000, 700): three axes with
               three different ulps (2^-13, 2^-12, 2^-14 -- 1e-4 to 2.4e-4, against a spacing of about 0.03), so the float
               grid produces many equal coordinates

Normals are returned as the (nx, ny, nz, curvature) float32 records the features take; [:, :3] is the analytic normal."""
import numpy as np

F32 = np.float32
SHIFT = (8192.0, -8192.0, 4096.0)
FAR_AT = (1500.0, -3000.0, 700.0)
HOLE_CENTRE = (0.5, 0.5)
HOLE_RADIUS = 0.15


def surface(x, y):
    """z = 0.08 sin 5x cos 4y + 0.5 and its unit normal (-dz/dx, -dz/dy, 1) / |.|, float64"""
    z = 0.08 * np.sin(5 * x) * np.cos(4 * y) + 0.5
    dzdx = 0.4 * np.cos(5 * x) * np.cos(4 * y)
    dzdy = -0.32 * np.sin(5 * x) * np.sin(4 * y)
    nrm = np.stack([-dzdx, -dzdy, np.ones_like(x)], axis=1)
    return z, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def records(nrm, curv):
    return np.ascontiguousarray(np.concatenate([np.asarray(nrm, F32), np.asarray(curv, F32)[:, None]], axis=1))


def outside_hole(x, y):
    return (x - HOLE_CENTRE[0]) ** 2 + (y - HOLE_CENTRE[1]) ** 2 > HOLE_RADIUS ** 2


def grid_sheet(n=1200, seed=3, quantum=2.0 ** -10, hole=None):
    """-> (points [k, 3] float32, records [k, 4] float32): x and y random multiples of `quantum` in [0, 1], z rounded to the
    quantum, duplicates removed (the first of each kept, the order of the draw otherwise), curvatures uniform in [0, 0.08).
    hole: a disc of radius 0.15 around (0.5, 0.5) is cut out, so that boundary flags exist inside the cloud."""
    rng = np.random.default_rng(seed)
    steps = int(round(1.0 / quantum))
    xy = rng.integers(0, steps + 1, (n, 2)) * quantum
    curv = rng.random(n) * 0.08
    z, nrm = surface(xy[:, 0], xy[:, 1])
    z = np.round(z / quantum) * quantum
    p = np.stack([xy[:, 0], xy[:, 1], z], axis=1)
    _, first = np.unique(p, axis=0, return_index=True)
    keep = np.zeros(n, bool)
    keep[first] = True
    if hole:
        keep &= outside_hole(xy[:, 0], xy[:, 1])
    pts = p[keep].astype(F32)
    assert np.array_equal(pts.astype(np.float64), p[keep])  # the grid is a grid of floats
    return np.ascontiguousarray(pts), records(nrm[keep], curv[keep])


def moved(points, shift=SHIFT):
    """points + shift in float32, the move exact in both directions"""
    pts = np.asarray(points, F32)
    s = np.asarray(shift, F32)
    assert np.array_equal(s.astype(np.float64), np.asarray(shift, np.float64))
    out = (pts + s).astype(F32)
    assert np.array_equal(out.astype(np.float64), pts.astype(np.float64) + s.astype(np.float64))
    assert np.array_equal(out - s, pts)
    return np.ascontiguousarray(out)


def scaled(points, e):
    """points * 2^e in float32, the round trip exact"""
    pts = np.asarray(points, F32)
    f = F32(2.0) ** F32(e)
    assert float(f) == 2.0 ** e
    out = (pts * f).astype(F32)
    assert np.array_equal(out.astype(np.float64), pts.astype(np.float64) * 2.0 ** e)
    assert np.array_equal(out / f, pts)
    return np.ascontiguousarray(out)


def far_raw(n=900, seed=3, at=FAR_AT):
    """-> (points [n, 3] float32, records [n, 4] float32): the surface at random float64 (x, y) in [0, 1]^2, moved by `at` in
    float64 and stored as float32 -- nothing about this cloud is exact; its expectation is the restatement of the stored
    floats themselves"""
    rng = np.random.default_rng(seed)
    x, y = rng.random(n), rng.random(n)
    curv = rng.random(n) * 0.08
    z, nrm = surface(x, y)
    p = np.stack([x, y, z], axis=1) + np.asarray(at, np.float64)
    return np.ascontiguousarray(p.astype(F32)), records(nrm, curv)
