"""The order-statistic selection of the Trimmed and MedianDistance rejectors (pcl_amd/csrc/rejectors.hip) at the sizes
where its paths change: the scalar tails of the four-pairs-per-thread kernels (every n % 4), Trimmed's edge modes and
setMinCorrespondences, a Distance threshold that equals a distance, several grid-stride trips of rs_hist_kernel in flight,
and tie passes whose rank lands on a query index with bit 22 set.

No CPU nearest-neighbour search is needed: the target is a shuffled integer lattice and every source point is a lattice
point moved by 0 or 0.25 along each axis, so its nearest target is its own lattice point (any other is at least 0.75 away
along some axis), every coordinate and distance is exact in float32, and the squared distance takes four values only
(0, 1/16, 2/16, 3/16): ties by the hundred thousand, ordered by the query index.  The lists before rejection are known
in closed form; oracle/rejectors.py rejects, and the device's lists are compared with np.array_equal."""
import numpy as np
import pytest

from oracle import rejectors as rej

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


_grids = {}


def lattice(side, n, seed):
    """(target [n,3], source [n,3], and the correspondences before rejection: query, match, squared distance)"""
    if side not in _grids:
        g = np.arange(side, dtype=np.float32)
        _grids[side] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    tgt = _grids[side][:n]
    assert len(tgt) == n
    tgt = tgt[rng.permutation(n)]
    perm = rng.permutation(n)
    off = rng.choice(np.array([0.0, 0.25], np.float32), (n, 3))
    src = (tgt[perm] + off).astype(np.float32)
    d = ((off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2]).astype(np.float32)
    return tgt, src, np.arange(n, dtype=np.int32), perm.astype(np.int32), d


_cases = {}


def case(gpu, side, n, seed):
    """the lattice of one size with its target index built: made once, shared by the tests of that size"""
    import pcl_amd
    key = (side, n, seed)
    if key not in _cases:
        tgt, src, q0, m0, d0 = lattice(side, n, seed)
        ce = pcl_amd.CorrespondenceEstimation(gpu)
        ce.setInputSource(src)
        ce.setInputTarget(tgt)
        _cases[key] = (ce, q0, m0, d0)
    return _cases[key]


def same(got, want):
    return all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want[:3]))


def trimmed(ratio, min_corr=0):
    import pcl_amd
    r = pcl_amd.CorrespondenceRejectorTrimmed()
    r.setOverlapRatio(ratio)
    r.setMinCorrespondences(min_corr)
    return r


def median(factor):
    import pcl_amd
    r = pcl_amd.CorrespondenceRejectorMedianDistance()
    r.setMedianFactor(factor)
    return r


# ---- small sizes: every n % 4 (rej_tail_first in the init, distance, median and trim kernels and the histogram's own
# tail), more than one block of the histogram kernel, on a 17^3 lattice -------------------------------------------------
SMALL = (4097, 4098, 4099, 4100)


@pytest.mark.parametrize("n", SMALL)
def test_no_rejector_gives_the_closed_form(gpu, n):
    # the construction itself: what the rejectors are given is what the references below are given
    ce, q0, m0, d0 = case(gpu, 17, n, n)
    assert same(ce.determineCorrespondences(), (q0, m0, d0))
    assert sorted(np.unique(d0).tolist()) == [0.0, 0.0625, 0.125, 0.1875]


@pytest.mark.parametrize("n", SMALL)
def test_trimmed_edge_modes_and_min_correspondences(gpu, n):
    ce, q0, m0, d0 = case(gpu, 17, n, n)
    # nv = max(floor(float(ratio) * float(count)), min_correspondences): 0 drops everything, nv >= count cuts nothing
    want_len = {(0.0, 0): 0, (0.0, 5): 5, (1.0, 0): n, (1.5, 0): n, (0.3, n - 1): n - 1, (0.3, n): n, (0.3, n + 7): n}
    for ratio, mc in ((0.0, 0), (0.0, 5), (1.0, 0), (1.5, 0), (0.3, 0), (0.3, n - 1), (0.3, n), (0.3, n + 7), (0.999, 0)):
        want = rej.reject_trimmed(q0, m0, d0, ratio, mc)
        if (ratio, mc) in want_len:
            assert len(want[0]) == want_len[(ratio, mc)]
        else:
            assert 0 < len(want[0]) < n
        got = ce.determineCorrespondences(rejectors=[trimmed(ratio, mc)])
        assert same(got, want), (n, ratio, mc, len(got[0]), len(want[0]))


@pytest.mark.parametrize("n", SMALL)
def test_median_factors(gpu, n):
    ce, q0, m0, d0 = case(gpu, 17, n, n)
    for factor in (0.0, 0.5, 1.0, 2.0):
        r = median(factor)
        got = ce.determineCorrespondences(rejectors=[r])
        want = rej.reject_median_distance(q0, m0, d0, factor)
        assert same(got, want), (n, factor, len(got[0]), len(want[0]))
        assert r.getMedianDistance() == want[3]
        assert 0 < len(want[0]) <= n


@pytest.mark.parametrize("n", SMALL)
def test_distance_threshold_equal_to_a_distance(gpu, n):
    # the test is strict: distance < max_distance^2 (correspondence_rejection_distance.cpp:55-60); 0.25^2 = 1/16 is one
    # of the four distances, exactly
    import pcl_amd
    ce, q0, m0, d0 = case(gpu, 17, n, n)
    up = float(np.nextafter(np.float32(0.25), np.float32(1)))
    lens = []
    for md in (0.25, up):
        r = pcl_amd.CorrespondenceRejectorDistance()
        r.setMaximumDistance(md)
        want = rej.reject_distance(q0, m0, d0, md)
        lens.append(len(want[0]))
        assert same(ce.determineCorrespondences(rejectors=[r]), want), (n, md)
    assert lens[0] == int((d0 == 0).sum()) and lens[1] == int((d0 <= 0.0625).sum()) and 0 < lens[0] < lens[1]


# ---- large sizes: the histogram kernel's trips -----------------------------------------------------------------------
# rs_hist_kernel runs at most 2 * num_cus blocks of 256 threads, a thread takes 4 pairs per trip of its grid-stride loop
# and keeps RS_TRIPS = 4 trips of loads in flight per iteration: on 256 CUs one trip covers 512 * 256 * 4 = 524,288
# pairs and one iteration 2,097,152.
#   600,001          a full first trip and a ragged second one (75,713 pairs), n % 4 = 1
#   1,400,002        two full trips and a ragged third one, n % 4 = 2
#   2^22 + 50,001    two full iterations and the start of a third; query indices with bit 22 set: the first digit of
#                    Trimmed's tie passes (q >> 22) leaves bin 0
# all on a 162^3 lattice.
LARGE = (600_001, 1_400_002, (1 << 22) + 50_001)
LARGE_IDS = ["600001", "1400002", "2p22p50001"]


@pytest.mark.parametrize("ratio", [0.1245, 0.5])
@pytest.mark.parametrize("n", LARGE, ids=LARGE_IDS)
def test_trimmed_many_trips_and_high_index_ties(gpu, n, ratio):
    ce, q0, m0, d0 = case(gpu, 162, n, 3)
    want = rej.reject_trimmed(q0, m0, d0, ratio)
    # on the reference alone: the cut falls inside a group of equal distances (the tie passes run) ...
    nv = len(want[0])
    assert 0 < nv < n and int((d0 <= want[2][-1]).sum()) > nv
    # ... and, at the largest size, the last kept query has bit 22 set for the ratio just under 1/8 (the zero distances
    # of the first 2^22 queries do not fill the rank) and not for 1/2
    if n > (1 << 22):
        assert (int(want[0][-1]) >= (1 << 22)) == (ratio == 0.1245), int(want[0][-1])
    got = ce.determineCorrespondences(rejectors=[trimmed(ratio)])
    assert same(got, want), (n, ratio, len(got[0]), nv)


@pytest.mark.parametrize("n", LARGE, ids=LARGE_IDS)
def test_median_many_trips(gpu, n):
    ce, q0, m0, d0 = case(gpu, 162, n, 3)
    r = median(1.0)
    got = ce.determineCorrespondences(rejectors=[r])
    want = rej.reject_median_distance(q0, m0, d0, 1.0)
    assert 0 < len(want[0]) < n
    assert same(got, want), (n, len(got[0]), len(want[0]))
    assert r.getMedianDistance() == want[3]
