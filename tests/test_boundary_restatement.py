"""tests/boundary_restatement.py against the reference's own expectations on bun0 (test/features/
test_boundary_estimation.cpp), its two formulations against each other, and the closed forms the device tests use.  No GPU."""
import numpy as np
import pytest

import boundary_restatement as br

BUN0_RADII = (2, 3, 4, 6)
# boundary points / queries with >= 3 neighbours at thr = pi / 2 with the normals stored in bun0.pcd
BUN0_COUNTS = {2: (277, 396), 3: (132, 397), 4: (119, 397), 6: (105, 397)}
LATTICE_ROTATIONS = {"aligned": None, "x_up": br.rotation((0.3, 1.0, 0.2), 1.4), "y_up": br.rotation((1.0, 0.2, 0.3), -1.3),
                     "tilted": br.rotation((0.5, -0.7, 0.4), 0.6)}


@pytest.fixture(scope="module")
def bun0():
    return br.load_bun0()


def test_bun0_golden(bun0):
    """the reference's test: every point carries the cloud's one plane normal and has every point as a neighbour"""
    pts, _ = bun0
    n = len(pts)
    ref = br.restate(pts, br.global_normal(pts), radius=10.0)
    assert [int(ref["flag"][i]) for i in (0, n // 3, n // 2, n - 1)] == [0, 0, 0, 1]
    assert (ref["m"] == n).all() and not ref["invalid"].any()
    assert br.unstable(ref) == 0 and ref["flips"] == 0
    print("bun0 golden: worst |g32 - g64| / E = %.3f at kappa <= %.1f" % (ref["ratio"], ref["kappa"]))
    assert ref["ratio"] <= 1.0


def test_basis_is_orthogonal(bun0):
    """getCoordinateSystemOnPlane, the reference's own three checks"""
    _, nrm = bun0
    seen = set()
    for nv in list(nrm) + [np.array(v, np.float32) for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 1, 1), (1, 1, -1))]:
        u, v = br.basis(nv)
        seen.add(int(np.argmax(np.abs(nv))))
        assert abs(float(nv @ u)) <= 1e-4 and abs(float(nv @ v)) <= 1e-4 and abs(float(u @ v)) <= 1e-4
        assert abs(float(v @ v) - 1) <= 1e-6
    assert seen == {0, 1, 2}
    # the rule for 4-vectors: a tie goes to the first index, the second index is 1 only for maxi == 0
    u, v = br.basis(np.array((1, 1, 1), np.float32))
    assert np.allclose(v, (-np.sqrt(0.5), np.sqrt(0.5), 0))
    u, v = br.basis(np.array((0, 0, 1), np.float32))
    assert v.tolist() == [1, 0, 0] and u.tolist() == [0, 1, 0]


@pytest.mark.parametrize("factor", BUN0_RADII)
def test_bun0_file_normals(bun0, factor):
    pts, nrm = bun0
    ref = br.restate(pts, nrm, radius=factor * br.BUN0_RESOLUTION)
    assert (int(ref["flag"].sum()), int((ref["m"] >= 3).sum())) == BUN0_COUNTS[factor]
    assert br.unstable(ref) == 0 and ref["flips"] == 0  # the band is empty, float64 gives the same flags
    print("bun0 r = %d x: worst |g32 - g64| / E = %.3f (spread %.2e, kappa <= %.1f), closest gap to thr %.2e"
          % (factor, ref["ratio"], ref["spread"], ref["kappa"], ref["closest"].min()))
    assert ref["ratio"] <= 1.0


@pytest.mark.parametrize("name", sorted(LATTICE_ROTATIONS))
def test_lattice_closed_forms(name):
    pts, nrm, ij = br.planar_lattice(9, LATTICE_ROTATIONS[name])
    want = br.lattice_gap(ij, 9)
    for thr, count in ((0.6, 81), (np.pi / 2, 32), (4.0, 4), (5.0, 0)):
        ref = br.restate(pts, nrm, threshold=thr, radius=1.5)
        assert int(ref["flag"].sum()) == count
        assert np.array_equal(ref["flag"] != 0, want > thr)
        assert br.unstable(ref) == 0 and ref["ratio"] <= 1.0
        assert np.abs(ref["max32"] - want).max() <= 1e-5
    assert {int(m) for m in ref["m"]} == {4, 6, 9}


def test_lattice_rotations_move_the_largest_component():
    tops = {name: int(np.argmax(np.abs(br.planar_lattice(9, r)[1]))) for name, r in LATTICE_ROTATIONS.items()}
    assert tops["aligned"] == 2 and tops["x_up"] == 0 and tops["y_up"] == 1


@pytest.mark.parametrize("thr", (np.pi / 8 + 0.01, np.pi / 4, np.pi / 2, np.pi))
def test_ring(thr):
    """one wedge just above and just below the threshold: the restatement's flag of the centre, at two phases and across
    the +-pi cut"""
    nrm = np.array((0, 0, 1), np.float32)
    for phase in (0.1, -2.0, np.pi - thr / 2):
        for wedge, want in ((thr + 1e-3, 1), (thr - 1e-3, 0)):
            ref = br.restate(br.ring(48, wedge, phase), nrm, threshold=thr, radius=1.5, rows=[0])
            assert int(ref["flag"][0]) == want and br.unstable(ref) == 0 and ref["m"][0] == 49
            assert abs(ref["max32"][0] - wedge) <= 1e-5


def test_few_neighbours_duplicates_and_invalid():
    pts = np.array([(0, 0, 0), (0, 0, 0), (0, 0, 0), (5, 0, 0), (5.5, 0, 0), (9, 9, 9), (np.nan, 0, 0), (20, 0, 0),
                    (20.5, 0, 0), (20, 0.5, 0)], np.float32)
    nrm = np.tile(np.array((0, 0, 1), np.float32), (len(pts), 1))
    nrm[7] = 0
    nrm[8] = np.nan
    ref = br.restate(pts, nrm, radius=1.0)
    assert ref["m"][:6].tolist() == [3, 3, 3, 2, 2, 1]
    assert ref["flag"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert ref["invalid"].tolist() == [False] * 6 + [True, True, True, False]
