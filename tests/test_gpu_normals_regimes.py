"""NormalEstimation off the smooth sheet of tests/test_gpu_parity.py (synthetic sheet, gaussian_surface, bunny): exact
planes and lines, coincident points, clouds smaller than k, volumes, ties at the k-th distance that decide the normal,
and float32 subnormal scales -- the clouds on which normals_kernel<8> leaves its fast path (tie redo, REC_CAP overflow,
non-finite k-th distance) and the plane fit of normals_math.hpp leaves its main branch (compute_roots2, the second and
third eigenvector branches, both arms of unit_orthogonal, scale <= FLT_MIN, eig_sum == 0, cos_theta == 0).

Every cloud goes through every entry point that applies: input == surface at k in KS (normals_kernel<8|16|32>,
normals_from_knn_kernel at k = 33), setSearchSurface with nudged queries at k in (8, 33) (normals_at_kernel),
setRadiusSearch at two radii with and without a search surface (normals_radius_kernel<false|true>), and setIndices.

Bars (none is calibrated on the code under test; `rec` is the path record of the oracle's own fit, PLANE_PATH_DTYPE):
 1. NaN mask and nan_count equal the oracle's.
 2. rows on which the oracle took the c0 path (no atan2f / cosf / sinf): normal and curvature bit-equal in the k-NN modes;
    in radius mode on the exact-arithmetic clouds (coordinates in multiples of 1/64 or 1/16: every sum is exact, so the
    kernel's double sums round to the float sums) for queries that coincide with a surface point (the kernel shifts by
    the query, the reference by the first neighbour: the same coordinates there, not for a nudged query).
 3. well-conditioned rows (rec.gap10 >= 0.01, |cos_theta| >= 1e-4 |v|): n . n_ref >= 1 - 1e-5 with the same orientation,
    |curvature - ref| < 1e-5.  The share of finite rows the filter leaves out is capped on the cube (1 %) and the
    clusters (5 %).
 4. every finite row: unit length within 1e-5, and (n^T C n - lambda_0) / trace(C) in float64, C from the reference's
    neighbour list, at most 4 x the largest value the oracle's own float normals reach on the same cloud and k, + 1e-7.
 5. on the wavefront emulation (tests/test_normals_wavesim.py): every finite row of the k-NN modes bit-equal.

Every family asserts ON THE REFERENCE ALONE that it is in the regime it is meant for.

Records (seeds as committed; the reference-alone figures are the same on every machine).
  waves of normals_kernel<8> through the second traversal at k = 8 (an emulation build with -DPCLHIP_NRM_STATS,
  Context.counters()[5]): cube 2 of 32, clusters 7 of 36, lattice3d 8 of 16, coincident 1 of 7, random_at_4096 1 of 7;
  ridge, planes, lines and the subnormal scales 0 (their ties take the redo through TopKReg instead).
  rows bar 3 leaves out, on the reference, over every entry but k = 3 (k-NN, search surface, the four radius entries):
  cube at most 0.83 % (r = 0.08), clusters at most 1.53 % (k = 8 with a search surface); caps 1 % and 5 %.  k = 3: 4.01 % and
  3.23 %, held to 5 % (test_volumes says why).
  the oracle's own excess for bar 4, smallest .. largest over k in KS: cube 9.7e-10 .. 6.5e-8, clusters 5.5e-6 .. 1.3e-3
  (k = 3: three of a cluster's points and its neighbour far away), coincident up to 5.4e-8, lattice3d 3.9e-8, ridge
  1.8e-8, random_at_4096 4.9e-8, small clouds 4.1e-8, planes and lines <= 2.6e-16, the subnormal scales 0.5 .. 0.93 (the
  constant (1, 0, 0) of a covariance that is 0 in float).
  ties that decide the normal on the ridge cloud, rows per k = 3, 7, 8, 9, 16, 17, 32, 33: 30, 499, 536, 2, 734, 193,
  575, 458.
  the reference's own curvature error against float64 on bar 3's rows in radius mode (the guard in check()): at most
  4.7e-6 at the committed radii; 1.8e-5 on the cube at r = 0.15, 5.9e-6 on the clusters at r = 0.01, where the
  device's curvature was 9.2e-6 and 1.04e-5 away from the oracle's (on the clusters' worst row the device was 4.5e-6
  and the oracle 5.9e-6 from the float64 value, on opposite sides).
  the wide radii of test_volumes against float64, input = surface / search surface: cube device 1.77e-5 / 2.07e-5 (oracle
  1.77e-5 / 1.93e-5), clusters device 5.2e-6 / 7.2e-6 (oracle 5.9e-6 / 5.9e-6); the same on the device and the emulation.
  the device's worst values (MI355X), k-NN modes / radius modes: every c0-path row bit-equal; of the trig
  rows about one in eight differs from the oracle in some bit; 1 - n.n_ref <= 2.5e-7 / 2.3e-7 (two float unit vectors
  that agree to the last bit give up to 1.2e-7), |curvature - ref| <= 7.1e-8 / 5.1e-6, | |n| - 1 | <= 1.4e-7,
  bar 4's excess at most 0.25 of its bound.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [3, 7, 8, 9, 16, 17, 32, 33]
KS_AT = [8, 33]
THREADS = 4  # of the oracle per call: the clouds are small, a team per core of a large host costs more than the search


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pcl_oracle
    return pcl_oracle


@pytest.fixture(scope="module")
def emulated(gpu):
    return b"wavesim" in (gpu.lib.pclhip_version() or b"")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the clouds ----------------------------------------------------------------------------------------------------------------
def lattice2(n=24, h=1.0 / 64, tilt=False):
    g = np.arange(n, dtype=np.float32) * np.float32(h)
    x, y = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    return np.ascontiguousarray(np.stack([x, y, x if tilt else np.zeros_like(x)], axis=1), dtype=np.float32)


def line(direction, n=300, h=1.0 / 64):
    t = np.arange(n, dtype=np.float32) * np.float32(h)
    return np.ascontiguousarray(t[:, None] * np.asarray(direction, np.float32)[None, :], dtype=np.float32)


def random_cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def coincident():
    pts = random_cloud(424, 31)
    pts[200:224] = pts[200]  # 24 copies of one point
    return pts


def sprinkle(pts, seed):
    """a few NaN and inf points: NaN rows, nobody's neighbour"""
    rng = np.random.default_rng(seed)
    at = rng.choice(len(pts), 6, replace=False)
    pts[at[0], 0] = np.nan
    pts[at[1], 1] = np.inf
    pts[at[2], 2] = -np.inf
    pts[at[3]] = np.nan
    pts[at[4], 2] = np.nan
    pts[at[5], 0] = np.inf
    return pts


def cube():
    return sprinkle(random_cloud(2000, 41), 42)


def clusters():
    rng = np.random.default_rng(43)
    centres = rng.uniform(0, 100, (40, 3))
    pts = np.concatenate([(centres[:, None, :] + rng.normal(scale=1e-3, size=(40, 50, 3))).reshape(-1, 3),
                          rng.uniform(0, 100, (300, 3))]).astype(np.float32)
    return sprinkle(pts[rng.permutation(len(pts))], 44)


def lattice3(n=10, h=1.0 / 16):
    g = np.arange(n, dtype=np.float32) * np.float32(h)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))


def ridge(n=32, h=1.0 / 16, seed=51):
    """A square lattice folded into a zigzag of 45-degree roofs, two steps per slope (z = |x mod 4h - 2h|), its points in
    a shuffled order.  Lattice neighbours at equal distance lie on different slopes, so which of two tied candidates the
    lower-index rule admits at the k-th distance tilts the fitted plane by degrees."""
    i, j = [a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    z = np.abs(i % 4 - 2)
    pts = (np.stack([i, j, z], axis=1) * h).astype(np.float32)
    return np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))])


def scaled(pts, s, offset=0.0):
    return np.ascontiguousarray((pts.astype(np.float64) * s + offset).astype(np.float32))


# name -> (builder, step = the cloud's length scale (radii and the queries' nudge are multiples of it), the two radii in
# steps, viewpoints, exact arithmetic)
H = 1.0 / 64
FAMILIES = {
    "plane_flat": (lambda: lattice2(), H, (1.5, 2.9), [(0.2, 0.1, 5.0), (3.0, 1.0, 0.0), (0.1, 0.2, -5.0)], True),
    "plane_tilted": (lambda: lattice2(tilt=True), H, (1.5, 2.9), [(0.0, 0.0, 5.0), (2.0, 1.0, 2.0), (0.0, 0.0, -5.0)], True),
    "line_x": (lambda: line((1, 0, 0)), H, (2.5, 6.5), [(0.3, 0.2, 5.0)], True),
    "line_z": (lambda: line((0, 0, 1)), H, (2.5, 6.5), [(0.3, 0.2, 5.0)], True),
    "line_diag": (lambda: line((1, 1, 1)), H, (4.4, 11.3), [(0.3, 0.2, 5.0)], True),
    "coincident": (coincident, 0.05, (3.0, 4.0), [(0.5, 0.5, 9.0)], False),
    "cube": (cube, 0.05, (1.6, 2.0), [(0.5, 0.5, 9.0)], False),
    "clusters": (clusters, 1e-3, (0.8, 1.0), [(50.0, 50.0, 900.0)], False),
    "lattice3d": (lattice3, 1.0 / 16, (1.1, 1.5), [(0.3, 0.2, 5.0)], True),
    "ridge": (ridge, 1.0 / 16, (1.5, 2.3), [(1.0, 1.0, 50.0)], True),
    "plane_1e-19": (lambda: scaled(lattice2(), 1e-19), H * 1e-19, (1.5, 2.9), [(0.0, 0.0, 1e-17)], False),
    "plane_1e-20": (lambda: scaled(lattice2(), 1e-20), H * 1e-20, (1.5, 2.9), [(0.0, 0.0, 1e-18)], False),
    "random_1e-19": (lambda: scaled(random_cloud(400, 61), 1e-19), 0.05e-19, (3.0, 6.0), [(0.0, 0.0, 1e-17)], False),
    "random_1e-20": (lambda: scaled(random_cloud(400, 61), 1e-20), 0.05e-20, (3.0, 6.0), [(0.0, 0.0, 1e-18)], False),
    "random_at_4096": (lambda: scaled(random_cloud(400, 61), 0.01, 4096.0), 5e-4, (2.5, 3.0), [(4096.0, 4096.0, 4200.0)], False),
}
SMALL_N = [2, 3, 5, 9, 17, 63, 64, 65]
FAMILIES.update({"small_%d" % n: (lambda n=n: random_cloud(n, 70 + n), 0.1, (3.0, 4.0) if n >= 17 else (6.0, 9.0),
                                  [(0.5, 0.5, 9.0)], False) for n in SMALL_N})
# One more radius per volume, in steps, with dozens of neighbours (cube: about 28, clusters: the whole cluster of 50): the double
# sums of normals_radius_kernel over long lists.  There the ORACLE's curvature is itself 1.8e-5 (cube) and 5.9e-6 (clusters)
# off the float64 value, so bar 3 has no reference; these runs are held to bars 1 and 4 and to the float64 curvature instead
# (check(..., wide=True)).
WIDE_RADIUS = {"cube": 3.0, "clusters": 10.0}
NUDGE = np.array([0.25, -0.125, 0.5])  # in steps: off every plane and line above


_cache = {}


def family(name):
    if ("cloud", name) not in _cache:
        build, step, radii, vps, exact = FAMILIES[name]
        pts = build()
        qry = np.ascontiguousarray((pts.astype(np.float64) + NUDGE * step).astype(np.float32))
        pts.setflags(write=False)
        qry.setflags(write=False)
        _cache[("cloud", name)] = dict(name=name, pts=pts, qry=qry, step=step, radii=[r * step for r in radii], vps=vps,
                                       exact=exact)
    return _cache[("cloud", name)]


# ---- the reference -------------------------------------------------------------------------------------------------------------
def pad_lists(off, idx, rows):
    width = max(3, int(np.diff(off.astype(np.int64)).max()) if rows else 3)
    out = np.full((rows, width), -1, np.int32)
    for i in range(rows):
        nb = idx[int(off[i]):int(off[i + 1])]
        out[i, :len(nb)] = nb
    return out


def reference(orc, fam, mode, param, vp):
    """mode "knn" | "at" (k = param) | "radius" | "radius_at" (radius = param).  -> dict(want, nan, lists, rec, fit, surface, queries); computed once per key."""
    from oracle import rejectors as rej
    key = (fam["name"], mode, param, tuple(vp))
    if key in _cache:
        return _cache[key]
    pts = fam["pts"]
    if ("tree", fam["name"]) not in _cache:
        _cache[("tree", fam["name"])] = orc.KdTree(pts)
    tree = _cache[("tree", fam["name"])]
    queries = fam["qry"] if mode in ("at", "radius_at") else pts
    if mode == "knn":
        want, lists, nan = tree.normals(pts, param, viewpoint=vp, want_knn=True, nthreads=THREADS)
    elif mode == "at":
        want, nan = tree.normals_at(pts, queries, param, viewpoint=vp, nthreads=THREADS)
        lists, _ = tree.knn(queries, param, nthreads=THREADS)
    else:
        if mode == "radius":
            want, nan = rej.normals_radius(orc, pts, param, viewpoint=vp)
        else:
            want, nan = rej.normals_radius_at(orc, pts, queries, param, viewpoint=vp)
        off, idx, _ = rej.radius_search_bruteforce(pts, queries, param)
        lists = pad_lists(off, idx, len(queries))
    fit, rec = orc.plane_fit_lists(pts, lists)
    ok = ~np.isnan(want[:, 0])
    # the record belongs to the fit the reference made: the same normal up to the viewpoint flip, bit for bit
    assert np.array_equal(np.isnan(fit[:, 0]), ~ok)
    assert np.array_equal(bits(np.abs(fit[ok])), bits(np.abs(want[ok])))
    for a in (want, lists, fit, rec):
        a.setflags(write=False)
    _cache[key] = dict(want=want, nan=int(nan), lists=lists, rec=rec, fit=fit, surface=pts, queries=queries, vp=vp, ok=ok)
    return _cache[key]


def float64_fit(ref):
    """covariance, smallest eigenvalue and trace in float64 of the reference's neighbour list, for every finite row"""
    if "f64" not in ref:
        lists = ref["lists"][ref["ok"]]
        P = ref["surface"].astype(np.float64)[np.maximum(lists, 0), :3]
        w = (lists >= 0).astype(np.float64)[:, :, None]
        cnt = w.sum(axis=1)
        mean = (P * w).sum(axis=1) / cnt
        D = (P - mean[:, None, :]) * w
        Cm = np.einsum("rki,rkj->rij", D, D) / cnt[:, :, None]
        ref["f64"] = (Cm, np.linalg.eigvalsh(Cm)[:, 0], np.trace(Cm, axis1=1, axis2=2))
    return ref["f64"]


def excess(ref, normals):
    """(n^T C n - lambda_0) / trace(C) in float64 for every finite reference row, C the covariance of the reference's
    neighbour list; 0 where trace(C) == 0 (coincident neighbours: every unit vector is a minimiser)."""
    Cm, lam0, tr = float64_fit(ref)
    n = normals[ref["ok"], :3].astype(np.float64)
    q = np.einsum("ri,rij,rj->r", n, Cm, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tr > 0, (q - lam0) / tr, 0.0)


def check(label, got, got_nan, ref, *, knn_mode, bit_equal_c0, emulated, wide=False):
    """bars 1 to 5 of the module's docstring on one run.  wide=True (a radius at which the oracle's own curvature is further
    than half of bar 3 from the float64 value): bars 1 and 4, and the curvature against FLOAT64 on every finite row -- the
    device's largest error at most 4 x the oracle's own largest + 1e-7, the form of bar 4 and for its reason: both are
    evaluations of one float solver on covariances that agree to the last bits."""
    want, ok, rec = ref["want"], ref["ok"], ref["rec"]
    assert got.shape == want.shape, label
    # bar 1
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    assert got_nan == ref["nan"] == int((~ok).sum()), (label, got_nan, ref["nan"])
    if not ok.any():
        return dict(finite=0, left_out=0.0)
    g, w = got[ok], want[ok]
    same = (bits(g) == bits(w)).all(axis=1)
    c0 = rec["roots_path"][ok] == 0
    # bar 2
    if bit_equal_c0:
        assert same[c0].all(), (label, "c0-path rows differ from the oracle", int((~same[c0]).sum()), int(c0.sum()))
    # bar 5
    if emulated and knn_mode:
        assert same.all(), (label, "rows differ from the oracle on the emulation", int((~same).sum()))
    # bar 3
    v = np.asarray(ref["vp"], np.float64) - ref["queries"][ok, :3].astype(np.float64)
    cos = np.einsum("ri,ri->r", v, w[:, :3].astype(np.float64))
    well = (rec["gap10"][ok] >= 0.01) & (np.abs(cos) >= 1e-4 * np.linalg.norm(v, axis=1))
    dots = np.einsum("ri,ri->r", g[:, :3].astype(np.float64), w[:, :3].astype(np.float64))
    dcurv = np.abs(g[:, 3].astype(np.float64) - w[:, 3])
    _, lam0, tr = float64_fit(ref)
    curv64 = np.where(tr > 0, lam0 / np.where(tr > 0, tr, 1), 0.0)
    if not knn_mode and well.any() and not wide:
        # Radius mode: the kernel sums in double what the reference sums in float, so the two fits start from covariances
        # that differ in their last bits, and PCL's closed-form float solver resolves the smallest eigenvalue of a nearly
        # isotropic neighbourhood only coarsely (cube, r = 0.15: the ORACLE's curvature is 1.8e-5 off the float64 one).  The
        # oracle can hold another evaluation to 1e-5 only where it is itself well inside that: the radii of FAMILIES are
        # chosen, on the reference alone, so that it is within half the bar on bar 3's rows.
        own = np.abs(w[:, 3] - curv64)[well].max()
        assert own < 5e-6, (label, "the reference's own curvature error", own)
    worst_dot = float(dots[well].min()) if well.any() else 1.0
    worst_curv = float(dcurv[well].max()) if well.any() else 0.0
    # bar 4
    length = np.abs(np.linalg.norm(g[:, :3].astype(np.float64), axis=1) - 1)
    e_ref = excess(ref, want)
    assert np.isfinite(e_ref).all(), label
    e_got = excess(ref, got)
    bound = 4 * float(e_ref.max()) + 1e-7
    out = dict(finite=int(ok.sum()), c0=int(c0.sum()), differ=int((~same).sum()), left_out=1 - well.sum() / ok.sum(),
               one_minus_dot=1 - worst_dot, dcurv=worst_curv, length=float(length.max()), excess=float(e_got.max()),
               excess_oracle=float(e_ref.max()))
    print("%-46s finite %5d c0 %5d differ %5d left out %.4f  1-dot %.2e dcurv %.2e |len-1| %.2e excess %.2e (oracle %.2e)"
          % (label, out["finite"], out["c0"], out["differ"], out["left_out"], out["one_minus_dot"], out["dcurv"],
             out["length"], out["excess"], out["excess_oracle"]))
    if wide:
        own, dev = float(np.abs(w[:, 3] - curv64).max()), float(np.abs(g[:, 3] - curv64).max())
        print("%-46s curvature against float64: device %.2e, oracle %.2e" % (label, dev, own))
        assert own > 5e-6, (label, "not a wide radius: bar 3 applies", own)
        assert dev <= 4 * own + 1e-7, (label, dev, own)
    else:
        assert worst_dot >= 1 - 1e-5, (label, worst_dot)
        assert worst_curv < 1e-5, (label, worst_curv)
    assert length.max() <= 1e-5, (label, length.max())
    assert e_got.max() <= bound, (label, float(e_got.max()), bound)
    return out


_trees = {}


def run(gpu, cloud, k=0, radius=0.0, vp=(0, 0, 0), surface=None, indices=None, own_tree=False):
    """one NormalEstimation.  Deliberately, the index of a surface is built once and handed over with setSearchMethod (an
    index build per run made up most of the module's time; the arrays of family() live as long as the module, so the tree's
    record of its cloud stays valid) -- the runs of one family therefore share the index and the normals it retains.
    own_tree=True leaves the tree to NormalEstimation itself (its default path): all_entries() does one such run per family
    and its rows must equal the shared tree's."""
    import pcl_amd
    ne = pcl_amd.NormalEstimation(gpu)
    ne.setInputCloud(cloud)
    on = surface if surface is not None else cloud
    if not on.flags.writeable and not own_tree:  # a family's own array
        if id(on) not in _trees:
            _trees[id(on)] = pcl_amd.KdTree(gpu)
        ne.setSearchMethod(_trees[id(on)])
    if surface is not None:
        ne.setSearchSurface(surface)
    if indices is not None:
        ne.setIndices(indices)
    if k:
        ne.setKSearch(k)
    else:
        ne.setRadiusSearch(radius)
    ne.setViewPoint(*vp)
    out = ne.compute()
    return out, ne.nan_count


def all_entries(gpu, orc, name, emulated, ks=KS, ks_at=KS_AT):
    """every entry point on one family; -> {label: figures}"""
    fam = family(name)
    pts, qry = fam["pts"], fam["qry"]
    figures = {}
    for vi, vp in enumerate(fam["vps"]):  # (further viewpoints: the k-NN kernels and one radius, enough for the flip)
        tag = "%s vp=%s" % (name, (vp,))
        for k in ks:
            ref = reference(orc, fam, "knn", k, vp)
            got, nan = run(gpu, pts, k=k, vp=vp)
            figures["knn", k, vp] = check("%s k=%d" % (tag, k), got, nan, ref, knn_mode=True, bit_equal_c0=True, emulated=emulated)
        for k in ks_at if vi == 0 else ():
            ref = reference(orc, fam, "at", k, vp)
            got, nan = run(gpu, qry, k=k, vp=vp, surface=pts)
            figures["at", k, vp] = check("%s at k=%d" % (tag, k), got, nan, ref, knn_mode=True, bit_equal_c0=True, emulated=emulated)
        for r in fam["radii"] if vi == 0 else fam["radii"][:1]:
            ref = reference(orc, fam, "radius", r, vp)
            got, nan = run(gpu, pts, radius=r, vp=vp)
            figures["radius", r, vp] = check("%s r=%g" % (tag, r), got, nan, ref, knn_mode=False, bit_equal_c0=fam["exact"],
                                             emulated=emulated)
            if vi:
                continue
            ref = reference(orc, fam, "radius_at", r, vp)
            got, nan = run(gpu, qry, radius=r, vp=vp, surface=pts)
            figures["radius_at", r, vp] = check("%s at r=%g" % (tag, r), got, nan, ref, knn_mode=False, bit_equal_c0=False,
                                                emulated=emulated)
            if fam["exact"]:  # queries that coincide with the surface's points: the kernel's shift is the reference's
                same = pts.copy()
                got2, nan2 = run(gpu, same, radius=r, vp=vp, surface=pts)
                check("%s same r=%g" % (tag, r), got2, nan2, reference(orc, fam, "radius", r, vp), knn_mode=False,
                      bit_equal_c0=True, emulated=emulated)
    # setIndices: the rows of the full run, a repeated index among them
    vp = fam["vps"][0]
    ind = np.concatenate([np.arange(1, len(pts), 3), [len(pts) - 1, len(pts) - 1, 0]]).astype(np.int32)
    for kw in (dict(k=8), dict(k=33), dict(radius=fam["radii"][0])):
        full, _ = run(gpu, pts, vp=vp, **kw)
        alone, _ = run(gpu, pts, vp=vp, own_tree=True, **kw)   # the index NormalEstimation builds for itself
        assert np.array_equal(bits(alone), bits(full)), (name, kw)
        part, nan = run(gpu, pts, vp=vp, indices=ind, **kw)
        assert np.array_equal(part, full[ind], equal_nan=True), (name, kw)
        assert nan == int(np.isnan(full[ind, 0]).sum()), (name, kw)
    return figures


def paths(orc, name, mode="knn", ks=KS):
    """the path records of the finite rows of one family, per k"""
    fam = family(name)
    out = {}
    for k in ks:
        ref = reference(orc, fam, mode, k, fam["vps"][0])
        out[k] = ref["rec"][ref["ok"]]
    return out


# ---- exact planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane_flat", "plane_tilted"])
def test_exact_planes(gpu, orc, emulated, name):
    fam = family(name)
    above, inplane, below = fam["vps"]
    for mode, params in (("knn", KS), ("at", KS_AT), ("radius", fam["radii"])):
        for p in params:
            for vp in fam["vps"]:
                ref = reference(orc, fam, mode, p, vp)
                assert ref["ok"].all() and (ref["rec"]["roots_path"] == orc.ROOTS_C0).all(), (name, mode, p)
    # the viewpoint in the plane: cos_theta == 0 exactly and the fit's normal stays as it is; below the plane it is turned.
    # (At k = 3 the three nearest points of a lattice can lie in a row: those fits are lines, their normal lies in the plane.)
    for k in KS:
        ref = reference(orc, fam, "knn", k, inplane)
        flat = ref["rec"]["eigvec_branch"] == 1
        assert flat.all() or k == 3, (name, k)
        assert flat.sum() >= 48
        v = np.asarray(inplane, np.float32) - fam["pts"]
        n = ref["fit"]
        cos = (v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) + v[:, 2] * n[:, 2]
        assert (cos[flat] == 0).all(), (name, k)
        assert np.array_equal(bits(ref["want"][flat]), bits(ref["fit"][flat]))
        up, down = reference(orc, fam, "knn", k, above)["want"], reference(orc, fam, "knn", k, below)["want"]
        assert (up[flat, 2] > 0).all() and (down[flat, 2] < 0).all()
        assert np.array_equal(bits(up[flat, :3]), bits(-down[flat, :3]))
        assert np.array_equal(bits(n[flat]), bits(up[flat]))   # the fit itself points up: `below` is the viewpoint that turns it
    all_entries(gpu, orc, name, emulated)


# ---- exact lines -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,arm", [("line_x", 1), ("line_z", 2), ("line_diag", 1)])
def test_exact_lines(gpu, orc, emulated, name, arm):
    """collinear neighbourhoods: the second eigenvector branch; the line along z takes unit_orthogonal's second arm"""
    for k, rec in paths(orc, name).items():
        assert (rec["eigvec_branch"] == 2).all() and (rec["orthogonal_arm"] == arm).all(), (name, k)
        assert (rec["roots_path"] == orc.ROOTS_C0).all(), (name, k)
    all_entries(gpu, orc, name, emulated)


# ---- coincident points -----------------------------------------------------------------------------------------------------
def test_coincident_points(gpu, orc, emulated):
    """24 copies of one point: at k <= 24 their neighbourhoods are the copies (by index, all at distance 0): the constant
    branch with eig_sum == 0, and more than 8 candidates at the 8th distance (the tie redo of normals_kernel<8>)"""
    fam = family("coincident")
    copies = np.arange(200, 224)
    for k in [k for k in KS if k <= 17]:
        ref = reference(orc, fam, "knn", k, fam["vps"][0])
        assert (ref["rec"]["eigvec_branch"][copies] == 3).all() and (ref["rec"]["eig_sum_zero"][copies] == 1).all()
        assert (ref["lists"][copies] == np.arange(200, 200 + k)[None, :]).all()   # ties go to the lower index
        assert np.array_equal(ref["fit"][copies], np.tile(np.float32([1, 0, 0, 0]), (24, 1)))
    all_entries(gpu, orc, "coincident", emulated)


# ---- small clouds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL_N)
def test_small_clouds(gpu, orc, emulated, n):
    """n < k: the k-th distance of normals_kernel<8> is not finite; partial last groups; k = 1 and 2: every row NaN"""
    name = "small_%d" % n
    fam = family(name)
    for k in (1, 2):
        got, nan = run(gpu, fam["pts"], k=k)
        assert np.isnan(got).all() and nan == n
        ref = reference(orc, fam, "knn", k, fam["vps"][0])
        assert ref["nan"] == n
    if n == 2:
        assert reference(orc, fam, "knn", 8, fam["vps"][0])["nan"] == 2
    all_entries(gpu, orc, name, emulated)


# ---- volumes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cap", [("cube", 0.01), ("clusters", 0.05)])
def test_volumes(gpu, orc, emulated, name, cap):
    """the clouds on which lanes of normals_kernel<8> record more than REC_CAP leaves (counts in the module's docstring)"""
    fam = family(name)
    bad = ~np.isfinite(fam["pts"]).all(axis=1)
    assert bad.sum() == 6
    for k in KS:
        ref = reference(orc, fam, "knn", k, fam["vps"][0])
        assert np.array_equal(~ref["ok"], bad) and not np.isin(ref["lists"], np.nonzero(bad)[0]).any()
    figures = all_entries(gpu, orc, name, emulated)
    # the share of finite rows bar 3 leaves out, on EVERY entry (k-NN, search surface, both radii with and without a
    # surface).  The one exception is k = 3: three points always span a plane exactly, and gap10 < 0.01 then says no more
    # than that the triangle is a sliver (its height under a tenth of its base), which the three nearest points of a
    # volume are in a few rows of a hundred -- measured on the reference 4.01 % on the cube and 3.23 % on the clusters;
    # k = 3 is held to 5 % on both.
    for key, f in figures.items():
        limit = 0.05 if key[:2] == ("knn", 3) else cap
        assert f["left_out"] <= limit, (name, key, f["left_out"], limit)
    # the wide radius (WIDE_RADIUS): long neighbour lists, judged against float64
    vp, r = fam["vps"][0], WIDE_RADIUS[name] * fam["step"]
    for mode, cloud in (("radius", fam["pts"]), ("radius_at", fam["qry"])):
        ref = reference(orc, fam, mode, r, vp)
        assert np.median((ref["lists"][ref["ok"]] >= 0).sum(axis=1)) >= 24, (name, mode)
        got, nan = run(gpu, cloud, radius=r, vp=vp, surface=fam["pts"] if mode == "radius_at" else None)
        check("%s wide %s r=%g" % (name, mode, r), got, nan, ref, knn_mode=False, bit_equal_c0=False, emulated=emulated, wide=True)


# ---- ties that decide the normal -------------------------------------------------------------------------------------------
def tie_rows(orc, fam, k):
    """rows whose k-th and (k+1)-th reference distances are equal, whose fit is well conditioned, and whose float64 normal
    turns by more than 1e-2 rad when the (k+1)-th neighbour takes the k-th's place"""
    pts = fam["pts"]
    ref = reference(orc, fam, "knn", k, fam["vps"][0])
    idx, d2 = _cache[("tree", fam["name"])].knn(pts, k + 1, nthreads=THREADS)
    assert np.array_equal(idx[:, :k], ref["lists"])
    tied = (d2[:, k - 1] == d2[:, k]) & (ref["rec"]["gap10"] >= 0.01)
    assert (idx[tied, k - 1] < idx[tied, k]).all()    # the lower index is the one inside

    def normal64(lists):
        P = pts.astype(np.float64)[lists]
        D = P - P.mean(axis=1, keepdims=True)
        return np.linalg.eigh(np.einsum("rki,rkj->rij", D, D))[1][:, :, 0]

    swapped = idx[:, :k].copy()
    swapped[:, k - 1] = idx[:, k]
    cosang = np.abs(np.einsum("ri,ri->r", normal64(idx[:, :k]), normal64(swapped)))
    return tied & (np.arccos(np.minimum(cosang, 1.0)) > 1e-2), tied


def test_mass_ties_on_a_lattice(gpu, orc, emulated):
    fam = family("lattice3d")
    for k in KS:
        reference(orc, fam, "knn", k, fam["vps"][0])
        _, d2 = _cache[("tree", "lattice3d")].knn(fam["pts"], k + 1, nthreads=THREADS)
        assert (d2[:, k - 1] == d2[:, k]).mean() > (0.9 if k == 8 else 0.3), k
    all_entries(gpu, orc, "lattice3d", emulated)


def test_ties_that_decide_the_normal(gpu, orc, emulated):
    """at least 50 rows on which the device's choice among tied candidates shows in the normal, at a k of every kernel: such
    a row is in bar 3's set (gap >= 0.01) and 1 - cos(1e-2) = 5e-5 is five times that bar.  (The lattice's shells end at
    3 and 9 points for most rows: few ties there.)"""
    fam = family("ridge")
    for k in KS:
        deciding, tied = tie_rows(orc, fam, k)
        print("ridge k=%d: %d rows tied at the k-th distance, %d decide the normal" % (k, tied.sum(), deciding.sum()))
        assert deciding.sum() >= 50 or k in (3, 9), (k, int(deciding.sum()))
    all_entries(gpu, orc, "ridge", emulated)


# ---- scale edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane_1e-19", "plane_1e-20", "random_1e-19", "random_1e-20"])
def test_subnormal_scales(gpu, orc, emulated, name):
    """squared distances and covariances are subnormal in float32 or 0: scale <= FLT_MIN on every fit, ties by index"""
    fam = family(name)
    tiny = np.finfo(np.float32).tiny
    for k in KS:
        ref = reference(orc, fam, "knn", k, fam["vps"][0])
        assert ref["ok"].all() and (ref["rec"]["scale_small"] == 1).all(), (name, k)
        _, d2 = _cache[("tree", name)].knn(fam["pts"], k, nthreads=THREADS)
        assert (d2 < tiny).all()
        if name == "plane_1e-20":  # (h * 1e-20)^2 is 17 units of the smallest subnormal: the lattice's ties survive the scaling
            assert (d2[:, 1] == d2[:, 2]).all()
    all_entries(gpu, orc, name, emulated)


def test_small_cloud_far_from_the_origin(gpu, orc, emulated):
    """extent 0.01 at offset 4096 (the floats' spacing there is 4.9e-4): few distinct coordinates, duplicates and ties"""
    fam = family("random_at_4096")
    assert len(np.unique(fam["pts"][:, 0])) < 40
    all_entries(gpu, orc, "random_at_4096", emulated)
