"""oracle.rejectors.radius_search_bruteforce restated without its per-query Python loop, for SMALL targets and many
queries (TEST INFRASTRUCTURE ONLY): the whole (queries, target) matrix of float32 squared distances, a chunk of queries
at a time, with the brute force's operation order ((dx*dx)+dy*dy)+dz*dz and its test d2 < float32(radius*radius); every
row ordered by a stable argsort, so equal distances stay ascending by index.  tests/test_radius_restatement.py pins it
to the brute force, lists and bits."""
import numpy as np


def radius_search_small_target(tgt, qry, radius, max_nn=0, chunk=1 << 16):
    """CSR (offsets uint64 [nq + 1], indices int32, d2 float32) like radius_search_bruteforce(tgt, qry, radius, max_nn)."""
    t = np.ascontiguousarray(tgt[:, :3], np.float32)
    q = np.ascontiguousarray(qry[:, :3], np.float32)
    r2 = np.float32(np.float64(radius) * np.float64(radius))
    fin_t = np.isfinite(t).all(1)
    counts, idx, dd = [], [], []
    for b in range(0, len(q), chunk):
        qc = q[b:b + chunk]
        fin_q = np.isfinite(qc).all(1)
        with np.errstate(invalid="ignore", over="ignore"):
            dx = qc[:, None, 0] - t[None, :, 0]
            dy = qc[:, None, 1] - t[None, :, 1]
            dz = qc[:, None, 2] - t[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            sel = (d2 < r2) & fin_t[None, :] & fin_q[:, None]
        assert d2.dtype == np.float32
        cnt = sel.sum(1)
        if max_nn:
            cnt = np.minimum(cnt, max_nn)
        width = int(cnt.max()) if len(cnt) else 0
        order = np.argsort(np.where(sel, d2, np.float32(np.inf)), axis=1, kind="stable")[:, :width]
        take = np.arange(width)[None, :] < cnt[:, None]  # row-major: the CSR order
        idx.append(order[take].astype(np.int32))
        dd.append(np.take_along_axis(d2, order, 1)[take])
        counts.append(cnt)
    offsets = np.zeros(len(q) + 1, np.uint64)
    if counts:
        offsets[1:] = np.cumsum(np.concatenate(counts))
    return (offsets, np.concatenate(idx) if idx else np.zeros(0, np.int32),
            np.concatenate(dd) if dd else np.zeros(0, np.float32))
