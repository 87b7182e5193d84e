"""NormalDistributionsTransform off the path of tests/test_gpu_ndt.py (the sheet at resolution 0.05, the bunny, the
identity guess): the branches of nf::cell_from_sums that the sheet never takes, the voxel Gaussians at map coordinates,
the derivative pass at the class's default resolution and on both sides of the small-angle switch, a point that meets
all 27 cells around it, and More-Thuente line searches that take other cases than the first.

Every test first asserts ON THE RESTATEMENT (tests/ndt_restatement.py) that its input takes the branch it is meant for:
that is a condition on the input, so a later change of an input cannot quietly empty a test.

The voxel Gaussians are judged against a high-precision evaluation (mpmath at 50 digits; np.longdouble, 64-bit mantissa
on x86, where mpmath is missing) of filters/include/pcl/filters/impl/voxel_grid_covariance.hpp:329-356 applied to the raw
covariance of :326, which is bitwise the restatement's, read through its lower triangle as Eigen's SelfAdjointEigenSolver
reads it."""
import numpy as np
import pytest

import ndt_restatement as rs
from test_gpu_ndt import BUNNY, SYNTH, check_cells, check_evaluation, make_ndt, rs_params, stable_prefix, xyz1

pytestmark = pytest.mark.gpu

try:
    import mpmath
except ImportError:  # the long-double path: no test disappears
    mpmath = None

N_SHEET = 1 << 15


@pytest.fixture(scope="module")
def gpu():
    from conftest import make_context
    return make_context(0)


@pytest.fixture(scope="module")
def sheet():
    import pcl_amd
    return pcl_amd.synth.icp_pair(N_SHEET)


# ---- the high-precision voxel Gaussian -----------------------------------------------------------------------------
class _Num:
    """The scalar type of the reference: mpmath.mpf at 50 digits, or np.longdouble."""

    def __init__(self):
        if mpmath is not None:
            self.mp = mpmath.mp.clone()
            self.mp.dps = 50
            self.num, self.sqrt, self.tol, self.name = self.mp.mpf, self.mp.sqrt, self.mp.mpf(10) ** -110, "mpmath, 50 digits"
        else:
            self.num, self.sqrt, self.tol, self.name = np.longdouble, np.sqrt, np.longdouble(1e-44), "np.longdouble"


NUM = _Num()


def hp_eig3_lower(cov):
    """Eigenvalues (ascending) and eigenvectors (columns) of the symmetric matrix whose lower triangle is cov's: cyclic
    Jacobi in the high-precision type, started from numpy's double eigenvectors (two or three sweeps then suffice)."""
    num, sqrt = NUM.num, NUM.sqrt
    L = np.tril(cov) + np.tril(cov, -1).T
    _, V0 = np.linalg.eigh(L)
    S = [[num(float(L[i, j])) for j in range(3)] for i in range(3)]
    U = [[num(float(V0[i, j])) for j in range(3)] for i in range(3)]
    # Gram-Schmidt in the high-precision type: U orthogonal to working precision, not to 1e-16
    for c in range(3):
        for b in range(c):
            d = sum(U[k][c] * U[k][b] for k in range(3))
            for k in range(3):
                U[k][c] -= d * U[k][b]
        nrm = sqrt(sum(U[k][c] * U[k][c] for k in range(3)))
        for k in range(3):
            U[k][c] /= nrm
    SU = [[sum(S[i][k] * U[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    A = [[sum(U[k][i] * SU[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(i):
            A[i][j] = A[j][i] = (A[i][j] + A[j][i]) / 2
    one = num(1)
    for _ in range(60):
        off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2]
        diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2]
        if off == 0 or off <= NUM.tol * diag:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if A[p][q] == 0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2 * A[p][q])
                t = (one if theta >= 0 else -one) / (abs(theta) + sqrt(theta * theta + 1))
                c = one / sqrt(t * t + 1)
                s = t * c
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
                for k in range(3):
                    ukp, ukq = U[k][p], U[k][q]
                    U[k][p], U[k][q] = c * ukp - s * ukq, s * ukp + c * ukq
    o = sorted(range(3), key=lambda k: A[k][k])
    return [A[k][k] for k in o], [[U[r][k] for k in o] for r in range(3)]


def hp_inverse3(C):
    a, b, c, d, e, f, g, h, i = C[0][0], C[0][1], C[0][2], C[1][0], C[1][1], C[1][2], C[2][0], C[2][1], C[2][2]
    co = [[e * i - f * h, c * h - b * i, b * f - c * e],
          [f * g - d * i, a * i - c * g, c * d - a * f],
          [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * co[0][0] + b * co[1][0] + c * co[2][0]
    return [[co[r][k] / det for k in range(3)] for r in range(3)]


def hp_cell(cov, mult):
    """voxel_grid_covariance.hpp:329-356 from a raw covariance: (valid, icov as float64 (zero if not valid), the
    eigenvalues as floats, how many eigenvalues were inflated)."""
    num = NUM.num
    w, V = hp_eig3_lower(cov)
    wf = [float(x) for x in w]
    if w[0] < num(-1e-12) or w[1] < num(-1e-12) or w[2] <= 0:
        return False, np.zeros((3, 3)), wf, 0
    C = [[num(float(cov[r, c])) for c in range(3)] for r in range(3)]
    floor_ = num(float(mult)) * w[2]
    inflated = 0
    if w[0] < floor_:
        w = list(w)
        w[0] = floor_
        inflated = 1
        if w[1] < floor_:
            w[1] = floor_
            inflated = 2
        C = [[sum(V[r][k] * w[k] * V[c][k] for k in range(3)) for c in range(3)] for r in range(3)]
    inv = hp_inverse3(C)
    return True, np.array([[float(inv[r][c]) for c in range(3)] for r in range(3)]), wf, inflated


def near_threshold(w):
    """The eigenvalue tests `w0 < -1e-12 || w1 < -1e-12 || w2 <= 0` decided within 1e-3 relative of their threshold (for
    the last one: of the scale 1e-12 of the other two)."""
    return abs(w[0] + 1e-12) <= 1e-15 or abs(w[1] + 1e-12) <= 1e-15 or abs(w[2]) <= 1e-15


SHARP_FACTOR = 8


def check_cells_sharp(got, want, mult=0.01, excused_share=0.0, label=""):
    """The bitwise parts of check_cells, the validity flags, and icov per cell within the larger of
    1e-13 * max|icov| and SHARP_FACTOR times the restatement's own distance from the high-precision value of the same
    cell ("another double eigen-solver on the same matrix").  A cell whose high-precision eigenvalues decide a validity
    test within 1e-3 relative of its threshold may differ in its flag; at most `excused_share` of the cells may.
    The library keeps the 6 distinct entries of icov (DEVIATIONS in pcl_amd/csrc/ndt_forms.hpp), so its value is compared
    with the symmetric part of the high-precision one; the restatement's full matrix with the full one.  The part left
    out (a cell that keeps its eigenvalues inverts the raw, not quite symmetric covariance) is printed.
    Returns dict(inflated = cells by number of inflated eigenvalues, ...) computed from the high-precision eigenvalues.

    SHARP_FACTOR: on the wavefront emulation no cell of any input of this module is over the floor of 1e-13 (worst
    device error 1.6e-14), so the factor decides nothing there and no measurement supports a smaller or a larger one: 8
    stays.  Below the floor the ratio says more about the restatement's luck than about the library: among the cells with
    a device error over 1e-14 it is 6 to 44 (far-field cells on which LAPACK lands 3e-16 from the value)."""
    n = len(want["npoints"])
    assert len(got["npoints"]) == n > 0
    assert np.array_equal(got["voxel_ids"], want["voxel_ids"]) and np.all(np.diff(got["voxel_ids"]) > 0)
    assert np.array_equal(got["npoints"], want["npoints"])
    assert np.array_equal(got["centroids"].view(np.uint32), want["centroids"].view(np.uint32))
    assert np.array_equal(got["means"].view(np.uint64), want["means"].view(np.uint64))
    assert np.array_equal(got["cov"].view(np.uint64), want["cov"].view(np.uint64))
    assert np.array_equal(got["icov"], np.transpose(got["icov"], (0, 2, 1)))
    inflated = np.zeros(3, np.int64)
    excused = flag_diff_dev = flag_diff_rs = 0
    worst = worst_rs = worst_ratio = ratio_14 = anti = 0.0
    over_floor = 0
    bad = []
    for k in range(n):
        valid, icov, w, infl = hp_cell(want["cov"][k], mult)
        if near_threshold(w):
            excused += 1
            continue
        flag_diff_rs += int(bool(want["valid"][k]) != valid)
        if bool(got["valid"][k]) != valid:
            flag_diff_dev += 1
            continue
        if not valid:
            assert not got["icov"][k].any()
            continue
        inflated[infl] += 1
        scale = np.abs(icov).max()
        if not np.isfinite(scale):
            continue
        anti = max(anti, np.abs(icov - icov.T).max() / 2 / scale)
        e_dev = np.abs(got["icov"][k] - (icov + icov.T) / 2).max() / scale
        e_rs = np.abs(want["icov"][k] - icov).max() / scale
        worst, worst_rs = max(worst, e_dev), max(worst_rs, e_rs)
        if e_dev > 1e-14 and e_rs > 0:
            ratio_14 = max(ratio_14, e_dev / e_rs)
        if e_dev > 1e-13:
            over_floor += 1
            worst_ratio = max(worst_ratio, e_dev / e_rs if e_rs > 0 else np.inf)
        if e_dev > max(1e-13, SHARP_FACTOR * e_rs):
            bad.append((k, e_dev, e_rs))
    print("%s: %d cells (%d invalid), inflated 0 / 1 / 2 eigenvalues: %d / %d / %d, flags differing from the %s value: "
          "device %d, restatement %d, excused %d; worst icov error device %.3g, restatement %.3g; %d cells over 1e-13, "
          "worst device / restatement there %.3g (over 1e-14: %.3g); antisymmetric part of the reference value up to %.3g" %
          (label, n, int((~want["valid"]).sum()), inflated[0], inflated[1], inflated[2], NUM.name, flag_diff_dev,
           flag_diff_rs, excused, worst, worst_rs, over_floor, worst_ratio, ratio_14, anti))
    assert excused <= excused_share * n, (excused, n)
    assert flag_diff_rs == 0, flag_diff_rs  # the restatement reads the matrix as the high-precision evaluation does
    assert flag_diff_dev == 0, "validity flags of %d cells differ from the lower-triangle reading" % flag_diff_dev
    assert not bad, bad[:5]
    return dict(inflated=inflated, worst=worst, excused=excused)


# ---- cell regimes ---------------------------------------------------------------------------------------------------------
def cube_cloud(n, half=1.0, seed=21):
    return xyz1(np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(np.float32))


def lines_cloud():
    """Axis-parallel segments through [-1, 1]^3 with 1e-5 of noise across: most of their cells are needles (two
    eigenvalues under the floor), the crossings are not."""
    rng = np.random.default_rng(22)
    parts = []
    for axis in range(3):
        for _ in range(40):
            p = np.empty((400, 3))
            p[:] = rng.uniform(-1, 1, 3)
            p[:, axis] = rng.uniform(-1, 1, 400)
            parts.append(p + rng.normal(0, 1e-5, p.shape))
    return xyz1(np.concatenate(parts).astype(np.float32))


def plane_cloud():
    rng = np.random.default_rng(23)
    p = rng.uniform(-1, 1, (20000, 3)).astype(np.float32)
    p[:, 2] = np.float32(0.375)
    return xyz1(p)


def run_cells(gpu, tgt, resolution, label, min_points=None, mult=None, excused_share=0.0, flat=True):
    src = np.ascontiguousarray(tgt[:64, :4])
    reg = make_ndt(gpu, tgt, src, setResolution=resolution)
    kw = {}
    if min_points is not None:
        reg.setMinPointPerVoxel(min_points)
        kw["min_points"] = min_points
    if mult is not None:
        reg.p.min_covar_eigvalue_mult = mult
        kw["mult"] = mult
    got = reg.cells()
    want = rs.voxel_cells(tgt, resolution, **kw)
    if flat:
        check_cells(got, want)
    return check_cells_sharp(got, want, 0.01 if mult is None else mult, excused_share, label), got, want, reg


def test_ndt_cells_cube_plain_inverse(gpu):
    """The first input on which nf::cell_from_sums takes `icov = cov^-1` of the raw covariance (no eigenvalue under
    0.01 w2: the cofactor inverse alone), with negative voxel coordinates.  Uniform cube, 60000 points, resolution 0.25.
    Emulation: 512 cells, 512 / 0 / 0 inflated, worst icov error device 4.8e-16, restatement 3.4e-16, no cell over 1e-13."""
    r, got, want, _ = run_cells(gpu, cube_cloud(60000), 0.25, "cube")
    assert len(want["npoints"]) == 512 and r["inflated"][0] == 512
    assert (np.floor(want["centroids"] / np.float32(0.25)) < 0).any()


def test_ndt_cells_lines_two_inflated(gpu):
    """The first input with cells whose two smallest eigenvalues are both replaced (needles: w0 / w2 under 1e-8), next
    to cells with one and with none (where segments cross).  Emulation: 397 cells, 201 / 62 / 134 inflated, worst icov error
    device 5.1e-15, restatement 6.6e-15, no cell over 1e-13.  The cells that keep their eigenvalues are 0.3 wide and up to
    1 from the origin: the reference value's antisymmetric part, which the library's six entries cannot hold, reaches
    1.4e-13 * max|icov| there (printed).  With the symmetrised matrix that nf::eig3_sym read before, 4 cells of this input
    were 1.1e-13 to 1.5e-13 away: this test fails there too."""
    r, got, want, _ = run_cells(gpu, lines_cloud(), 0.3, "lines")
    assert r["inflated"][2] >= 100 and r["inflated"][1] >= 10 and r["inflated"][0] >= 10
    w = np.linalg.eigvalsh(want["cov"][want["valid"]])
    assert (w[:, 0] / w[:, 2]).min() < 1e-8


def test_ndt_cells_exact_plane(gpu):
    """An exactly singular covariance of non-identical points: z = 0.375 for every point, so the zz sum cancels to 0 and
    w0 is 0 or a rounding-level negative: valid (w0 >= -1e-12), one eigenvalue inflated, and nf::eig3_sym meets exact
    zeros off the diagonal.  Emulation: 100 cells, 0 / 100 / 0 inflated, worst icov error device 5.2e-16."""
    r, got, want, _ = run_cells(gpu, plane_cloud(), 0.2, "plane")
    assert want["valid"].all() and r["inflated"][1] == len(want["npoints"]) >= 100
    assert np.all(want["cov"][:, 2, 2] == 0.0)
    w0 = np.linalg.eigvalsh(want["cov"])[:, 0]
    assert np.all(w0 <= 1e-20) and np.all(w0 > -1e-12)


@pytest.mark.parametrize("min_points", [1, 3, 6, 12])
def test_ndt_cells_min_points(gpu, min_points):
    """min_points_per_voxel other than the default (1 is raised to 3: voxel_grid_covariance.h:214-225): the cells kept
    are the restatement's.  Cube of 4000 points at resolution 0.25: its voxels hold fewer than 3 to more than 12 points, so
    every value keeps another set of cells (asserted)."""
    tgt = cube_cloud(4000, seed=24)
    r, got, want, _ = run_cells(gpu, tgt, 0.25, "min_points %d" % min_points, min_points=min_points)
    assert want["npoints"].min() == max(3, min_points)
    sizes = [len(rs.voxel_cells(tgt, 0.25, min_points=m)["npoints"]) for m in (1, 3, 6, 12)]
    assert sizes[0] == sizes[1] > sizes[2] > sizes[3] > 0
    assert len(got["npoints"]) == sizes[(1, 3, 6, 12).index(min_points)]


@pytest.mark.parametrize("mult", [0.001, 0.1])
def test_ndt_cells_eigenvalue_floor(gpu, mult):
    """min_covar_eigvalue_mult other than 0.01: the floor decides which cells are inflated and by how much.  The same
    cube: at 0.1 some sixty cells have one eigenvalue floored, at 0.001 none, at the default one."""
    tgt = cube_cloud(4000, seed=24)
    r, got, want, _ = run_cells(gpu, tgt, 0.25, "mult %g" % mult, mult=mult)
    assert not np.array_equal(rs.voxel_cells(tgt, 0.25, mult=0.01 if mult == 0.1 else 0.1)["icov"], want["icov"])
    if mult == 0.1:
        assert r["inflated"][1] >= 50 and r["inflated"][0] >= 50
    else:
        assert r["inflated"][0] == len(want["npoints"])


def test_ndt_cells_nonfinite_target_rows(gpu):
    """Target rows with NaN or Inf are dropped before the grid's bounds are taken (voxel_grid_covariance.hpp:100-118):
    the cells are those of the finite rows."""
    tgt = cube_cloud(20000, seed=25)
    clean = tgt.copy()
    tgt[[5, 700, 701]] = np.nan
    tgt[900, 1] = np.inf
    tgt[1500, 0] = -np.inf
    tgt[19999, 2] = np.nan
    r, got, want, _ = run_cells(gpu, tgt, 0.25, "non-finite rows")
    kept = rs.voxel_cells(np.delete(clean, [5, 700, 701, 900, 1500, 19999], axis=0), 0.25)
    assert np.array_equal(kept["cov"], want["cov"]) and int(want["npoints"].sum()) <= 20000 - 6


def test_ndt_cells_point_normal_stride(gpu):
    """A target of 48-byte records (pcl::PointNormal's layout): the cells are those of its xyz columns."""
    tgt = cube_cloud(20000, seed=26)
    wide = np.random.default_rng(27).uniform(-5, 5, (len(tgt), 12)).astype(np.float32)
    wide[:, :3] = tgt[:, :3]
    reg = make_ndt(gpu, wide, tgt[:64], setResolution=0.25)
    want = rs.voxel_cells(tgt, 0.25)
    got = reg.cells()
    check_cells(got, want)
    check_cells_sharp(got, want, label="48-byte records")


# ---- far field ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,resolution", [(1.0, 0.05), (20.0, 1.0)])
@pytest.mark.parametrize("o", [1e2, 1e3, 1e4, 3e4])
def test_ndt_cells_far_field(gpu, sheet, o, scale, resolution):
    """The voxel Gaussians at map coordinates: the sheet moved to (o, -o, o).  The single-pass covariance of :326 cancels
    there, and its two triangles differ (pt_sum[r] * mean[c] against pt_sum[c] * mean[r]) by up to 2e-7 at o = 3e4; the
    reference's eigen-solver reads the lower one.  The first test that tells which triangle nf::eig3_sym reads.

    Emulation, with the symmetrised matrix that nf::eig3_sym read before -> reading the lower triangle (all 8 cases failed
    before, all pass now):
      validity flags differing from the high-precision value: sheet, o = 1e4: 2 of 1912 -> 0; o = 3e4: 4 of 1922 -> 0;
        sheet * 20 at resolution 1.0, o = 3e4: 1 of 1920 -> 0; none at the other offsets;
      worst icov error / max|icov|: sheet 1.2e-7, 7.5e-6, 1.4e-3, 2.4e-2 at o = 1e2, 1e3, 1e4, 3e4 -> <= 1.3e-14;
        sheet * 20: 1.6e-10, 3.2e-8, 4.3e-6, 3.7e-5 -> <= 1.6e-14 (the restatement: <= 9.8e-15 throughout).
    The excuse for eigenvalues at a threshold (<= 0.5 % of the cells) was used by no cell of any case."""
    tgt = sheet[0].copy()
    off = np.float32([o, -o, o])
    tgt[:, :3] = tgt[:, :3] * np.float32(scale) + off
    r, got, want, _ = run_cells(gpu, tgt, resolution, "far field o = %g, scale %g" % (o, scale), excused_share=0.005, flat=False)
    assert len(want["npoints"]) > 1000
    asym = np.abs(want["cov"] - np.transpose(want["cov"], (0, 2, 1))).max()
    print("max asymmetry of the raw covariance %.3g" % asym)
    if o >= 1e4 and scale == 1.0:
        assert asym > 1e-9  # the two triangles do differ on this input


# ---- evaluation regimes -----------------------------------------------------------------------------------------------------
EVAL_STATES = [np.zeros(6),
               np.array([0.1, -0.2, 0.05, 0.7, -1.1, 2.0]),
               np.array([0.3, 0.1, -0.2, -3.0, 1.5, 0.4]),
               # nf::angle_tables takes cos = 1, sin = 0 for |angle| < 10e-5: two angles at the bound (not below it), one
               # under it; then one under it, one just past it, one at it
               np.array([0.05, -0.02, 0.03, 1e-4, -1e-4, 9.9e-5]),
               np.array([-0.05, 0.02, 0.03, -9.9e-5, 1.0000001e-4, -1e-4])]


@pytest.mark.parametrize("resolution,outlier_ratio", [(1.0, 0.55), (1.0, 0.1), (2.5, 0.55)])
def test_ndt_evaluation_default_resolution(gpu, resolution, outlier_ratio):
    """ndt_eval_kernel at the class's default resolution 1.0 (the suite evaluates at 0.025 and 0.05 only, where d2 is 1 to
    three digits and d1 about -1e-3), at another outlier ratio and at 2.5; rotations of up to 3 rad; and the first states
    on both sides of the small-angle switch of nf::angle_tables.  check_evaluation's bar as it is: 1e-12 of the sum of the
    terms' magnitudes.  Emulation: score / gradient / Hessian errors <= 5.3e-15 over the 15 evaluations."""
    tgt = cube_cloud(40000, half=2.0, seed=31)
    src = xyz1(np.random.default_rng(32).uniform(-1.6, 1.6, (3000, 3)).astype(np.float32))
    reg = make_ndt(gpu, tgt, src)
    assert reg.getResolution() == 1.0 and reg.getOutlierRatio() == 0.55  # the defaults, untouched
    if resolution != 1.0:
        reg.setResolution(resolution)
    if outlier_ratio != 0.55:
        reg.setOutlierRatio(outlier_ratio)
    d1, d2 = rs.gauss_constants(resolution, outlier_ratio)
    print("resolution %g, outlier ratio %g: d1 = %.6g, d2 = %.6g" % (resolution, outlier_ratio, d1, d2))
    assert abs(d1) > 0.1  # not the regime of the fine grids
    cells = reg.cells()
    assert cells["valid"].all() and len(cells["valid"]) >= 8
    aj0, _ = rs.angle_tables(EVAL_STATES[3])
    assert aj0[5, 0] == 0.0 and aj0[3, 2] != 0.0  # rows -cy sz and sx sy: sz switched to 0, sx and sy not
    for x in EVAL_STATES:
        check_evaluation(reg, cells, src, resolution, x)


def block27_cloud():
    """The 27 voxels of a 3 x 3 x 3 block at resolution 1.0, 8 points each within 0.03 of the voxel's point nearest to the
    centre of the middle voxel: every centroid is within 0.54 * sqrt(3) + 0.03 < 1 of that centre."""
    rng = np.random.default_rng(41)
    near = {-1: -0.04, 0: 0.5, 1: 1.04}
    parts = [np.array([near[i], near[j], near[k]]) + rng.uniform(-0.03, 0.03, (8, 3))
             for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    return xyz1(np.concatenate(parts).astype(np.float32))


def test_ndt_evaluation_27_cells_per_point(gpu):
    """The geometric maximum that NdtCollect's 32-slot column is sized for: queries at the centre of a 3 x 3 x 3 block of
    occupied voxels meet all 27 cells (the suite's inputs reach about 9).  The pair count and the sums agree with the
    restatement and the overflow error does not fire.  Nothing here tries to exceed the 32 slots."""
    tgt = block27_cloud()
    src = xyz1(np.float32([[0.5, 0.5, 0.5], [0.51, 0.5, 0.49], [0.49, 0.51, 0.5], [0.5, 0.49, 0.51]]))
    reg = make_ndt(gpu, tgt, src)
    cells = reg.cells()
    assert len(cells["npoints"]) == 27 and np.all(cells["npoints"] == 8)
    search = rs.CellSearch(cells["centroids"], 1.0)
    for x in (np.zeros(6), np.array([0.004, -0.003, 0.002, 0.01, -0.02, 0.015])):
        pi, ci = search.pairs(rs.transform_se3(rs.convert_transform(x), src[:, :3]))
        assert np.array_equal(np.bincount(pi, minlength=4), [27] * 4) and len(pi) == 108
        assert reg.evaluate(x)[3] == 108
        check_evaluation(reg, cells, src, 1.0, x, need_gradient=False)


# ---- More-Thuente branches ---------------------------------------------------------------------------------------------------
def mt_coverage(want, prefix):
    cases = [c for m in want["mt"][:prefix] for c in m["cases"]]
    return ({c: cases.count(c) for c in (1, 2, 3, 4)}, sum(m["closed"] for m in want["mt"][:prefix]),
            sum(m["flipped"] for m in want["mt"][:prefix]), max(want["trials"][:prefix], default=0))


def loop_parity(gpu, tgt, src, params, guess, t_bar, label):
    reg = make_ndt(gpu, tgt, src, **params)
    reg.align(guess)
    want, prefix = stable_prefix(tgt, src, rs_params(params), guess)
    got = [t["line_search_trials"] for t in reg.trace]
    cases, closed, flipped, longest = mt_coverage(want, prefix)
    T = reg.getFinalTransformation().astype(np.float64)
    err = np.abs(T - want["T"].astype(np.float64)).max()
    print("%s: outer iterations %d (restated %d), trials %s (restated %s), stable prefix %d; inside it trial_value cases %s, "
          "interval closed %d times, direction flipped %d times, longest line search %d trials; |T - T_restated|_max %.3g" %
          (label, reg.nr_iterations_, want["nr_iterations"], got, want["trials"], prefix, cases, closed, flipped, longest, err))
    assert got[:prefix] == want["trials"][:prefix]
    for k in range(prefix):
        assert abs(reg.trace[k]["step_length"] - want["steps"][k]) <= 1e-9 * want["steps"][k]
    if prefix == len(want["trials"]):
        assert reg.nr_iterations_ == want["nr_iterations"] and reg.hasConverged() == want["converged"]
    assert err < t_bar, err
    return cases, closed, flipped, longest


def test_ndt_more_thuente_coarse_grid(gpu, sheet):
    """nf::mt_trial_value's case 4 (the trial is farther from a_l than a_t allows: the cubic through the upper end) and
    line searches whose interval closes (the switch from psi to phi in the step-length loop): the sheet at resolution 0.2.
    The suite's three alignments take case 1 nineteen times, case 2 once and close the interval once."""
    tgt, src, _ = sheet
    cases, closed, _, _ = loop_parity(gpu, tgt, src, dict(SYNTH, setResolution=0.2), None, 1e-5, "sheet at resolution 0.2")
    assert cases[4] >= 1 and closed >= 3


def test_ndt_more_thuente_from_a_guess(gpu, sheet):
    """Cases 1 and 2 and two closed intervals inside the stable prefix, from a guess 0.2 rad and 0.1 away.  The whole run
    of the restatement (13 outer iterations) also takes case 4 and a line search of three trials at its 11th iteration;
    the stable prefix ends at 10, so they are printed, not asserted (the emulation follows the restatement through all
    13: trials [0, 0, 1, 0, 2, 0, 0, 1, 1, 0, 3, 0, 0] on both sides, the same final transformation bit for bit)."""
    tgt, src, _ = sheet
    guess = rs.convert_transform([0.08, -0.06, 0.05, 0.2, -0.15, 0.1])
    cases, closed, flipped, _ = loop_parity(gpu, tgt, src, SYNTH, guess, 1e-5, "sheet from a guess")
    assert cases[1] >= 1 and cases[2] >= 1 and closed >= 2 and flipped >= 1


def test_ndt_more_thuente_long_steps_bunny(gpu, bunny):
    """The bunny with step size 0.5 (ten times the reference test's): the first trial overshoots again and again.  Inside
    the stable prefix (9 of 23 outer iterations): cases 1 and 4, the interval closes three times.  Beyond it the
    restatement takes case 2 and closes two more (emulation: the same trials on both sides through all 23)."""
    tgt, src = xyz1(bunny["bun4"]), xyz1(bunny["bun0"])
    cases, closed, _, _ = loop_parity(gpu, tgt, src, dict(BUNNY, setStepSize=0.5), None, 1e-3, "bunny, step size 0.5")
    assert cases[1] >= 1 and cases[4] >= 1 and closed >= 3
