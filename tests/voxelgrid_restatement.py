"""pcl::VoxelGrid<PointT>::applyFilter (filters/include/pcl/filters/impl/voxel_grid.hpp:597-814) with the CentroidPoint
accumulators (common/include/pcl/common/impl/accumulators.hpp:68-127) restated in numpy: float32 operations in the
reference's order, the WHOLE output record (x y z 1 | nx ny nz 0 | curvature 0 0 0 for 12-column clouds), the voxel ids,
the leaf layout and the grid dims.

  box pass    getMinMax3D over the records with finite x, y, z that pass the field filter against the limits CAST TO FLOAT
              (:615, :513-590)
  refusal     (max - min) * inverse_leaf per axis in float, + 1, the int64 product against INT32_MAX (:620-629) -> None
  grid        min_b / max_b = floor(min * inverse_leaf) (float product), div_b, multipliers (:632-644)
  key pass    finite records that pass the field filter against the DOUBLE limits (:677-688);
              ijk = int(floor(x * inverse_leaf) - float(min_b)), id = ijk . multipliers (:690-695)
  order       ascending id; inside a voxel ascending input index (the reference's spreadsort leaves that open, the project
              fixes it: pcl_amd/csrc/voxelgrid.hip)
  sums        the t-th member of every run is added for t = 0, 1, ... (one vectorised float32 addition per rank, so every
              run is a plain sequential float sum in its order; no reduce / reduceat, whose pairwise order differs)
  record      xyz = sum / count, w = 1; with downsample_all_data normal = sum / sqrt((sx*sx + sy*sy) + sz*sz) (0/0 and a NaN
              member give NaN, accumulators.hpp:99-105), curvature = sum / count, every other float 0; without it only xyz1.

`order` selects two deliberately WRONG variants, for tests/test_voxelgrid_restatement.py to prove that its inputs can tell
them apart: "descending" sums every run from its last member to its first, "unstable" breaks ties of equal ids by
descending input index (what an unstable sort may do)."""
import numpy as np

F = np.float32
INT32_MAX = 2147483647
SUM_COLS = (0, 1, 2, 4, 5, 6, 8)   # x y z | normal | curvature of a pcl::PointNormal record, in floats


def _to_int(v, bits):
    """static_cast<intN>(float) as the x86 conversion does it: out of range and NaN give the most negative value"""
    v = float(v)
    lim = 1 << (bits - 1)
    if v != v or v >= lim or v < -lim:
        return -lim
    return int(v)                      # truncation toward zero


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def field_pass(v, lo, hi, negative):
    """:535-553 / :677-688 on an array of field values: True = the record stays.  NaN compares false: it stays in both
    modes; a value exactly on a limit stays in both (only the open interior / the open outside is cut)."""
    with np.errstate(invalid="ignore"):
        if negative:
            return ~((v < hi) & (v > lo))
        return ~((v > hi) | (v < lo))


def sort_bits_of(div_b):
    """(id_bits, sort_bits, passes) of the device's radix sort for a grid: ids < nvox need id_bits, the all-ones key of
    rejected records one more (at most 32), eight bits a pass"""
    nvox = int(div_b[0]) * int(div_b[1]) * int(div_b[2])
    id_bits = 1
    while id_bits < 32 and (1 << id_bits) < nvox:
        id_bits += 1
    sort_bits = id_bits + 1 if id_bits < 32 else 32
    return id_bits, sort_bits, (sort_bits + 7) // 8


def run_sums(values, order, starts, counts, descending=False):
    """float32 sums of values[order[starts[r] : starts[r] + counts[r]]] per run r, member by member in that order (or from
    the last to the first).  values: (n, c) float32.  One vectorised addition per rank t; the runs are visited longest
    first so that the runs that still have a t-th member are a prefix."""
    by_len = np.argsort(-counts, kind="stable")
    st, ct = starts[by_len], counts[by_len]
    acc = np.zeros((len(starts), values.shape[1]), F)
    neg_ct = -ct                                   # ascending, for searchsorted
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(int(ct[0]) if len(ct) else 0):
            m = int(np.searchsorted(neg_ct, -t, side="left"))          # runs with count > t
            pos = st[:m] + (ct[:m] - 1 - t if descending else t)
            acc[:m] = acc[:m] + values[order[pos]]
    out = np.empty_like(acc)
    out[by_len] = acc
    return out


def voxelgrid(cloud, leaf, min_points=0, field=None, limits=None, negative=False, downsample_all_data=True,
              order="stable", with_layout=True, max_layout_cells=1 << 25):
    """cloud: (n, c >= 3) float32; 12 columns and more are PointNormal records and come back as (m, 12), anything else as
    (m, 4).  field: position of the filter field in floats (None: no filter), limits (lo, hi) as doubles.
    -> None when the reference refuses the grid (:624), else a dict:
       out (m, 4 | 12) float32, ids (m,) voxel ids of the kept voxels, counts (m,), nv, nruns, longest, box (False: no
       record passed the box pass -- the reference's grid is undefined then, out is empty and the dims are None),
       min_b, max_b, div_b, mul (int64[3]), layout (int32[ncells], -1 = empty or dropped; None when not asked for, above
       max_layout_cells or without a box), sort_bits, passes."""
    cloud = np.ascontiguousarray(cloud, F)
    n, c = cloud.shape
    wide = c >= 12
    cols = 12 if wide else 4
    leaf = np.asarray(leaf, F)
    if leaf.ndim == 0:
        leaf = np.full(3, leaf, F)
    inv = (F(1.0) / leaf).astype(F)                                                    # voxel_grid.h:279-282
    xyz = cloud[:, :3]
    finite = np.isfinite(xyz).all(1)
    res = dict(out=np.empty((0, cols), F), ids=np.empty(0, np.int64), counts=np.empty(0, np.int64), nv=0, nruns=0,
               longest=0, box=False, min_b=None, max_b=None, div_b=None, mul=None, layout=None, sort_bits=None, passes=None)
    in_box = finite.copy()
    if field is not None:
        lo, hi = float(limits[0]), float(limits[1])
        in_box &= field_pass(cloud[:, field], F(lo), F(hi), negative)                  # :615: limits cast to float
    if not in_box.any():
        return res
    mn = xyz[in_box].min(0)
    mx = xyz[in_box].max(0)
    with np.errstate(over="ignore", invalid="ignore"):
        ext = ((mx - mn).astype(F) * inv).astype(F)                                    # :620-622, float products
        d = [_wrap(_to_int(e, 64) + 1, 64) for e in ext]
        if _wrap(_wrap(d[0] * d[1], 64) * d[2], 64) > INT32_MAX:                       # :624
            return None
        min_b = np.array([_to_int(np.floor((mn[k] * inv[k]).astype(F)), 32) for k in range(3)], np.int64)   # :632-637
        max_b = np.array([_to_int(np.floor((mx[k] * inv[k]).astype(F)), 32) for k in range(3)], np.int64)
    div_b = max_b - min_b + 1
    mul = np.array([1, div_b[0], div_b[0] * div_b[1]], np.int64)
    ncells = int(div_b[0]) * int(div_b[1]) * int(div_b[2])
    id_bits, sort_bits, passes = sort_bits_of(div_b)
    res.update(box=True, min_b=min_b, max_b=max_b, div_b=div_b, mul=mul, sort_bits=sort_bits, passes=passes)
    if with_layout and ncells <= max_layout_cells:
        res["layout"] = np.full(ncells, -1, np.int32)
    valid = finite.copy()
    if field is not None:
        valid &= field_pass(cloud[:, field].astype(np.float64), lo, hi, negative)      # :677-688: double limits
    idx = np.flatnonzero(valid)
    res["nv"] = len(idx)
    if len(idx) == 0:
        return res
    p = xyz[idx]
    ijk = (np.floor((p * inv).astype(F)) - min_b.astype(F)).astype(F).astype(np.int64)  # :690-692
    key = (ijk * mul).sum(1) & 0xFFFFFFFF                                              # :695, as unsigned int
    if order == "unstable":
        perm = np.lexsort((-idx, key))
    else:
        perm = np.argsort(key, kind="stable")
    sk = key[perm]
    order_idx = idx[perm]
    heads = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    counts = np.diff(np.r_[heads, len(sk)])
    res.update(nruns=len(heads), longest=int(counts.max()))
    keep = counts >= min_points                                                         # :742
    heads, counts, ids = heads[keep], counts[keep], sk[heads[keep]]
    m = len(heads)
    out = np.zeros((m, cols), F)
    use = SUM_COLS if (wide and downsample_all_data) else SUM_COLS[:3]
    s = run_sums(np.ascontiguousarray(cloud[:, use]), order_idx, heads, counts, descending=(order == "descending"))
    cnt = counts.astype(F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out[:, :3] = s[:, :3] / cnt[:, None]                                           # accumulators.hpp:81
        out[:, 3] = 1
        if wide and downsample_all_data:
            nsum = s[:, 3:6]
            sq = (nsum * nsum).astype(F)
            length = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F))   # Vector4f::normalized, w = 0
            out[:, 4:7] = nsum / length[:, None]                                       # :105
            out[:, 8] = s[:, 6] / cnt                                                  # :131
    res.update(out=out, ids=ids.astype(np.int64), counts=counts)
    if res["layout"] is not None:
        res["layout"][ids] = np.arange(m, dtype=np.int32)                              # :787
    return res


def same_bytes(a, b):
    """The comparison of every VoxelGrid test: same shape, NaN at the same positions (a NaN's sign and payload are not
    pinned), every other float the same four bytes (so -0.0 is not 0.0)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_difference(a, b):
    """one line for an assertion message"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return "shapes %s / %s" % (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    if not bad.any():
        return "equal"
    r, c = np.argwhere(bad)[0]
    return "%d floats differ in %d rows, first at row %d col %d: %r / %r" % (bad.sum(), bad.any(1).sum(), r, c, a[r, c], b[r, c])
