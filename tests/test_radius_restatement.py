"""The vectorised radius search of tests/radius_restatement.py (the reference of the scan-edge cases of
tests/test_gpu_radius_lists.py, where the brute force's per-query loop is too slow) gives the brute force's lists, bit
for bit: ties, non-finite rows on both sides, max_nn, empty lists, more than one chunk."""
import numpy as np

import radius_restatement as rr
from oracle import rejectors as rej


def same(a, b):
    return (np.array_equal(a[0], b[0]) and a[0].dtype == b[0].dtype and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def test_vectorised_radius_search_is_the_brute_force():
    rng = np.random.default_rng(17)
    tgt = rng.uniform(0, 1, (48, 3)).astype(np.float32)
    tgt[9:13] = tgt[30:34]  # equal distances: ascending by index
    tgt[20, 1] = np.nan
    qry = rng.uniform(-0.1, 1.1, (300, 3)).astype(np.float32)
    qry[41] = np.inf
    qry[42, 2] = np.nan
    qry[100] = tgt[31]  # distance 0 to two points
    for radius, max_nn in ((0.2, 3), (0.2, 0), (0.45, 5), (1e-3, 0), (3.0, 0), (3.0, 47)):
        want = rej.radius_search_bruteforce(tgt, qry, radius, max_nn)
        for chunk in (1 << 16, 64, 7):
            assert same(rr.radius_search_small_target(tgt, qry, radius, max_nn, chunk=chunk), want), (radius, max_nn, chunk)
    # wider records than xyz, a target of one point, no query at all
    rec = np.full((300, 8), np.nan, np.float32)
    rec[:, :3] = qry
    assert same(rr.radius_search_small_target(tgt, rec, 0.2, 3), rej.radius_search_bruteforce(tgt, rec, 0.2, 3))
    assert same(rr.radius_search_small_target(tgt[:1], qry, 0.6), rej.radius_search_bruteforce(tgt[:1], qry, 0.6))
    off, idx, d2 = rr.radius_search_small_target(tgt, qry[:0], 0.2)
    assert off.tolist() == [0] and len(idx) == 0 and len(d2) == 0
