// ndt_forms.hpp -- the closed forms of NormalDistributionsTransform, written once for the host driver, the kernels of
// ndt.hpp / ndt_cells.hpp and the wavefront emulation of the test tier (the tests' numpy restatement follows the same
// operation order):
//   * the Gaussian constants d1, d2                      (registration/include/pcl/registration/impl/ndt.hpp:92-99)
//   * convertTransform in float                          (registration/include/pcl/registration/ndt.h:293-313)
//   * the Euler extraction of the guess                  (impl/ndt.hpp:113-125, Eigen's eulerAngles(0, 1, 2))
//   * computeAngleDerivatives                            (impl/ndt.hpp:306-389)
//   * a voxel Gaussian from its sums                     (filters/include/pcl/filters/impl/voxel_grid_covariance.hpp:281-361)
//   * computePointDerivatives + updateDerivatives / updateHessian for one (point, cell) pair
//                                                        (impl/ndt.hpp:391-437, 448-495, 573-608)
//   * the Newton direction: 6x6 one-sided Jacobi SVD     (impl/ndt.hpp:139-151)
//   * More-Thuente: trial value, interval update          (impl/ndt.hpp:620-776)
// Everything is IEEE double (float where the reference is float) in the reference's operation order, -ffp-contract=off.
// DEVIATIONS (all at the rounding level of the quantity named):
//   * sin / cos / atan2 of float angles are taken in double and rounded to float (as gicp_forms.hpp does): host, device
//     and numpy then agree on the float; the reference's float libm may differ by an ulp of a rotation entry;
//   * the cell's inverse covariance is kept as its 6 distinct entries, (i, j) from the upper triangle of cov^-1 computed
//     by the symmetric cofactor form: the reference's full inverse of V L V^-1 is asymmetric by a few ulp
//     (<= 1e-15 * max|icov|, cond <= 100 after the inflation);  V^-1 is taken as V^T (V orthogonal to 1e-16);
//   * a cell that keeps its eigenvalues inverts the raw covariance of :326, which is not symmetric (see eig3_sym): the
//     reference's inverse is then not symmetric either, and the 6 entries kept here are those of the inverse of the
//     symmetrised matrix, its symmetric part to first order.  The part left out is eps * |mean|^2 / variance * cond:
//     up to 2.9e-13 * max|icov| on cells 0.3 wide inside [-1, 1]^3, 1e-3 on a cell at 3e4.  x' C x does not see it;
//     x' C J_i does (the gradient and Hessian terms of such a pair, by that relative amount);
//   * the pair Hessian is accumulated for i <= j and mirrored: the reference's (i, j) and (j, i) differ only by the
//     association of (-d2 a_i) a_j, one ulp of that term.
#pragma once

#include <cmath>

#include "closed_forms.hpp"

namespace pclhip {
namespace nf {

constexpr int kNdtSums = 29;         // score, g[6], the 21 upper-triangle entries of H (row-major), the pair count
constexpr int kNdtCellDoubles = 9;   // mean[3], icov: c00 c01 c02 c11 c12 c22

struct NdtAngles {   // angular_jacobian_ (8 rows) and angular_hessian_ (15 rows), xyz columns
  double j[8][3];
  double h[15][3];
};

// position of (i, j), i <= j, among the 21 upper-triangle entries in row-major order
PCLHIP_HD constexpr int tri21(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

PCLHIP_HD void gauss_constants(float resolution, double outlier_ratio, double* d1, double* d2) {
  const double c1 = 10 * (1 - outlier_ratio);
  const double c2 = outlier_ratio / pow(double(resolution), 3);
  const double d3 = -log(c2);
  *d1 = -log(c1 + c2) - d3;
  *d2 = -2 * log((-log(c1 * exp(-0.5) + c2) - d3) / *d1);
}

// float 3x3 product in Eigen's coefficient order: (a0 b0 + a1 b1) + a2 b2
PCLHIP_HD void mul3f(const float* A, const float* B, float* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// AngleAxis<float>(angle, unit axis `ax`)::toRotationMatrix (Eigen/src/Geometry/AngleAxis.h)
PCLHIP_HD void angle_axis_matrix(float angle, int ax, float* R) {
  const float s = float(sin(double(angle))), c = float(cos(double(angle)));
  const float d = (1.0f - c) * 1.0f * 1.0f + c;  // cos1_axis * axis + c on the axis' own diagonal entry
  const int u = (ax + 1) % 3, v = (ax + 2) % 3;
  for (int k = 0; k < 9; ++k) R[k] = 0.0f;
  R[4 * ax] = d;
  R[4 * u] = c;
  R[4 * v] = c;
  R[3 * u + v] = -s;
  R[3 * v + u] = s;
}

// Translation * AngleAxis(x[3], X) * AngleAxis(x[4], Y) * AngleAxis(x[5], Z) in float, row-major 4x4
PCLHIP_HD void convert_transform(const double x[6], float T[16]) {
  float Rx[9], Ry[9], Rz[9], A[9], R[9];
  angle_axis_matrix(float(x[3]), 0, Rx);
  angle_axis_matrix(float(x[4]), 1, Ry);
  angle_axis_matrix(float(x[5]), 2, Rz);
  mul3f(Rx, Ry, A);
  mul3f(A, Rz, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
    T[4 * r + 3] = float(x[r]);
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}

// transform << translation, rotation().eulerAngles(0, 1, 2) of a float transform (Eigen/src/Geometry/EulerAngles.h with
// i = 0, j = 1, k = 2, "even" permutation), the angles rounded to float as the reference's Vector3f holds them
PCLHIP_HD void euler_from(const float T[16], double x[6]) {
  const double kPi = 3.14159265358979323846;
  auto m = [&](int r, int c) { return double(T[4 * r + c]); };
  double r0 = atan2(m(1, 2), m(2, 2));
  const double c2 = double(float(sqrt(double(T[0] * T[0] + T[1] * T[1]))));
  double r1;
  if (r0 > 0.0) {
    r0 -= kPi;
    r1 = atan2(-m(0, 2), -c2);
  } else {
    r1 = atan2(-m(0, 2), c2);
  }
  r0 = double(float(r0));
  const double s1 = double(float(sin(r0))), c1 = double(float(cos(r0)));
  const double r2 = atan2(s1 * m(2, 0) - c1 * m(1, 0), c1 * m(1, 1) - s1 * m(2, 1));
  x[0] = double(T[3]);
  x[1] = double(T[7]);
  x[2] = double(T[11]);
  x[3] = double(float(-r0));
  x[4] = double(float(-r1));
  x[5] = double(float(-r2));
}

PCLHIP_HD void angle_tables(const double x[6], NdtAngles& A) {
  double cx, cy, cz, sx, sy, sz;
  if (fabs(x[3]) < 10e-5) { cx = 1.0; sx = 0.0; } else { cx = cos(x[3]); sx = sin(x[3]); }
  if (fabs(x[4]) < 10e-5) { cy = 1.0; sy = 0.0; } else { cy = cos(x[4]); sy = sin(x[4]); }
  if (fabs(x[5]) < 10e-5) { cz = 1.0; sz = 0.0; } else { cz = cos(x[5]); sz = sin(x[5]); }
  const double J[8][3] = {{-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy},
                          {cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy},
                          {-sy * cz, sy * sz, cy},
                          {sx * cy * cz, -sx * cy * sz, sx * sy},
                          {-cx * cy * cz, cx * cy * sz, -cx * sy},
                          {-cy * sz, -cy * cz, 0},
                          {cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0},
                          {sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0}};
  const double H[15][3] = {{-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, sx * cy},
                           {-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, -cx * cy},
                           {cx * cy * cz, -cx * cy * sz, cx * sy},
                           {sx * cy * cz, -sx * cy * sz, sx * sy},
                           {-sx * cz - cx * sy * sz, sx * sz - cx * sy * cz, 0},
                           {cx * cz - sx * sy * sz, -sx * sy * cz - cx * sz, 0},
                           {-cy * cz, cy * sz, -sy},
                           {-sx * sy * cz, sx * sy * sz, sx * cy},
                           {cx * sy * cz, -cx * sy * sz, -cx * cy},
                           {sy * sz, sy * cz, 0},
                           {-sx * cy * sz, -sx * cy * cz, 0},
                           {cx * cy * sz, cx * cy * cz, 0},
                           {-cy * cz, cy * sz, 0},
                           {-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, 0},
                           {-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, 0}};
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 3; ++c) A.j[r][c] = J[r][c];
  for (int r = 0; r < 15; ++r)
    for (int c = 0; c < 3; ++c) A.h[r][c] = H[r][c];
}

// Eigenvalues (ascending) and eigenvectors (columns of V, row-major) of a symmetric 3x3: cyclic Jacobi in double.  Only
// the lower triangle of Ain is read, as Eigen's SelfAdjointEigenSolver does (voxel_grid_covariance.hpp:329): the raw
// covariance of :326 is not symmetric (pt_sum[r] * mean[c] against pt_sum[c] * mean[r]), and far from the origin the
// two triangles decide the eigenvalue tests of a thin cell differently (sheet at (1e4, -1e4, 1e4), resolution 0.05: 2 of
// 1912 validity flags; at 3e4: 4 of 1922).
PCLHIP_HD void eig3_sym(const double Ain[9], double w[3], double V[9]) {
  double A[3][3], U[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      A[i][j] = i >= j ? Ain[3 * i + j] : Ain[3 * j + i];
      U[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 40; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off == 0.0 || off <= 1e-40 * diag) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double ukp = U[k][p], ukq = U[k][q];
          U[k][p] = c * ukp - s * ukq;
          U[k][q] = s * ukp + c * ukq;
        }
      }
  }
  int o[3] = {0, 1, 2};
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2 - a; ++b)
      if (A[o[b]][o[b]] > A[o[b + 1]][o[b + 1]]) {
        const int t = o[b];
        o[b] = o[b + 1];
        o[b + 1] = t;
      }
  for (int c = 0; c < 3; ++c) {
    w[c] = A[o[c]][o[c]];
    for (int r = 0; r < 3; ++r) V[3 * r + c] = U[r][o[c]];
  }
}

// A voxel's Gaussian from its sequential sums (voxel_grid_covariance.hpp:285-361): mean, the raw covariance of :326
// (row-major 3x3), the inverse covariance (6 entries; zero for a cell that fails the eigenvalue test, as the Leaf
// constructor leaves it).  Returns the cell's validity (nr_points != -1).
PCLHIP_HD bool cell_from_sums(uint32_t n, const double pt_sum[3], const double cov_sum[9], double mult, double mean[3],
                              double cov[9], double icov[6]) {
  for (int k = 0; k < 3; ++k) mean[k] = pt_sum[k] / double(n);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) cov[3 * r + c] = (cov_sum[3 * r + c] - pt_sum[r] * mean[c]) / (double(n) - 1.0);
  for (int k = 0; k < 6; ++k) icov[k] = 0.0;
  double w[3], V[9];
  eig3_sym(cov, w, V);
  if (w[0] < -1e-12 || w[1] < -1e-12 || w[2] <= 0) return false;  // NumTraits<double>::dummy_precision()
  double C[9];
  for (int k = 0; k < 9; ++k) C[k] = cov[k];
  const double floor_ = mult * w[2];
  if (w[0] < floor_) {
    w[0] = floor_;
    if (w[1] < floor_) w[1] = floor_;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        C[3 * r + c] = (V[3 * r] * w[0] * V[3 * c] + V[3 * r + 1] * w[1] * V[3 * c + 1]) + V[3 * r + 2] * w[2] * V[3 * c + 2];
  }
  // cov^-1 by cofactors of the symmetrised matrix
  const double a = C[0], b = 0.5 * (C[1] + C[3]), c = 0.5 * (C[2] + C[6]), d = C[4], e = 0.5 * (C[5] + C[7]), f = C[8];
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  icov[0] = c00 / det;
  icov[1] = c01 / det;
  icov[2] = c02 / det;
  icov[3] = (a * f - c * c) / det;
  icov[4] = (b * c - a * e) / det;
  icov[5] = (a * d - b * b) / det;
  bool ok = true;
  for (int k = 0; k < 6; ++k)
    if (icov[k] == double(__builtin_inff()) || icov[k] == -double(__builtin_inff())) ok = false;
  return ok;
}

PCLHIP_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// c_inv * v with the symmetric 6-entry matrix
PCLHIP_HD void symv(const double* C, const double* v, double* o) {
  o[0] = (C[0] * v[0] + C[1] * v[1]) + C[2] * v[2];
  o[1] = (C[1] * v[0] + C[3] * v[1]) + C[4] * v[2];
  o[2] = (C[2] * v[0] + C[4] * v[1]) + C[5] * v[2];
}

// One (point, cell) pair: x the original point, xt = T x - mean, C the cell's inverse covariance.  Adds the pair's score
// to acc[0], its gradient to acc[1..6] (WITH_G) and the upper triangle of its Hessian to acc[7..27] (WITH_H).  A pair
// whose d2 * e is > 1, < 0 or NaN adds nothing (impl/ndt.hpp:467-469).  Every index is a compile-time constant after
// unrolling: acc stays in registers.
template <bool WITH_G, bool WITH_H>
PCLHIP_HD void pair_terms(const double x[3], const double xt[3], const double C[6], const NdtAngles& A, double d1, double d2,
                          double* acc) {
  double cx[3];
  symv(C, xt, cx);
  const double e = exp(-d2 * dot3(xt, cx) / 2);
  const double score_inc = -d1 * e;
  double e3 = d2 * e;
  if (e3 > 1 || e3 < 0 || e3 != e3) return;
  e3 *= d1;
  if (WITH_G) acc[0] += score_inc;
  // point_jacobian (3 x 6): unit columns, then the angular rows
  double paj[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) paj[r] = (A.j[r][0] * x[0] + A.j[r][1] * x[1]) + A.j[r][2] * x[2];
  const double J[6][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, paj[0], paj[1]}, {paj[2], paj[3], paj[4]}, {paj[5], paj[6], paj[7]}};
  double CJ[6][3], a[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    symv(C, J[i], CJ[i]);
    a[i] = dot3(xt, CJ[i]);
    if (WITH_G) acc[1 + i] += a[i] * e3;
  }
  if (WITH_H) {
    double pah[15];
#pragma unroll
    for (int r = 0; r < 15; ++r) pah[r] = (A.h[r][0] * x[0] + A.h[r][1] * x[1]) + A.h[r][2] * x[2];
    // point_hessian blocks (3 + i, 3 + j): a b c / b d e / c e f
    const double ph[6][3] = {{0, pah[0], pah[1]}, {0, pah[2], pah[3]}, {0, pah[4], pah[5]},
                             {pah[6], pah[7], pah[8]}, {pah[9], pah[10], pah[11]}, {pah[12], pah[13], pah[14]}};
    double xch[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double t[3];
      symv(C, ph[k], t);
      xch[k] = dot3(xt, t);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        double second = 0.0;
        if (i >= 3) second = xch[i == 3 ? (j - 3) : (i == 4 ? (j - 1) : 5)];
        acc[7 + tri21(i, j)] += e3 * ((-d2 * a[i] * a[j] + second) + dot3(J[j], CJ[i]));
      }
  }
}

// ---- the serial step (host) -----------------------------------------------------------------------------------------

// delta = JacobiSVD(H).solve(b): one-sided Jacobi on the columns of H (double), singular values at or below
// 6 eps * the largest are dropped as Eigen's rank() does
inline void svd_solve6(const double H[36], const double b[6], double delta[6]) {
  double U[6][6], V[6][6];
  bool finite = true;
  for (int i = 0; i < 6; ++i) {
    finite = finite && std::isfinite(b[i]);
    for (int j = 0; j < 6; ++j) {
      U[i][j] = H[6 * i + j];
      V[i][j] = i == j ? 1.0 : 0.0;
      finite = finite && std::isfinite(U[i][j]);
    }
  }
  if (!finite) {  // the reference's delta is NaN then: its isnan(delta_norm) exit takes it
    for (int r = 0; r < 6; ++r) delta[r] = std::nan("");
    return;
  }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int k = 0; k < 6; ++k) {
          al += U[k][p] * U[k][p];
          be += U[k][q] * U[k][q];
          ga += U[k][p] * U[k][q];
        }
        if (ga == 0.0 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 6; ++k) {
          const double up = U[k][p], uq = U[k][q];
          U[k][p] = c * up - s * uq;
          U[k][q] = s * up + c * uq;
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  double sv[6], smax = 0.0;
  for (int j = 0; j < 6; ++j) {
    double s = 0;
    for (int k = 0; k < 6; ++k) s += U[k][j] * U[k][j];
    sv[j] = sqrt(s);
    if (sv[j] > smax) smax = sv[j];
  }
  const double thr = smax * 6.0 * 2.220446049250313e-16;
  double y[6];
  for (int j = 0; j < 6; ++j) {
    y[j] = 0.0;
    if (!(sv[j] > thr) || sv[j] < 2.2250738585072014e-308) continue;
    double s = 0;
    for (int k = 0; k < 6; ++k) s += U[k][j] * b[k];
    y[j] = s / (sv[j] * sv[j]);  // (u_j . b) / sigma_j with u_j = U[:, j] / sigma_j
  }
  for (int r = 0; r < 6; ++r) {
    double s = 0;
    for (int j = 0; j < 6; ++j) s += V[r][j] * y[j];
    delta[r] = s;
  }
}

struct MtInterval {
  double a_l, f_l, g_l, a_u, f_u, g_u;
};

// updateIntervalMT (impl/ndt.hpp:620-663)
inline bool mt_update_interval(MtInterval& I, double a_t, double f_t, double g_t) {
  if (f_t > I.f_l) {
    I.a_u = a_t;
    I.f_u = f_t;
    I.g_u = g_t;
    return false;
  }
  if (g_t * (I.a_l - a_t) > 0) {
    I.a_l = a_t;
    I.f_l = f_t;
    I.g_l = g_t;
    return false;
  }
  if (g_t * (I.a_l - a_t) < 0) {
    I.a_u = I.a_l;
    I.f_u = I.f_l;
    I.g_u = I.g_l;
    I.a_l = a_t;
    I.f_l = f_t;
    I.g_l = g_t;
    return false;
  }
  return true;
}

// trialValueSelectionMT (impl/ndt.hpp:665-776)
inline double mt_trial_value(const MtInterval& I, double a_t, double f_t, double g_t) {
  const double a_l = I.a_l, f_l = I.f_l, g_l = I.g_l, a_u = I.a_u, f_u = I.f_u, g_u = I.g_u;
  if (a_t == a_l && a_t == a_u) return a_t;
  int cond;
  if (a_t == a_l) cond = 4;
  else if (f_t > f_l) cond = 1;
  else if (g_t * g_l < 0) cond = 2;
  else if (std::fabs(g_t) <= std::fabs(g_l)) cond = 3;
  else cond = 4;
  if (cond != 4) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    if (cond == 1) {
      const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
      if (std::fabs(a_c - a_l) < std::fabs(a_q - a_l)) return a_c;
      return 0.5 * (a_q + a_c);
    }
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    if (cond == 2) return std::fabs(a_c - a_t) >= std::fabs(a_s - a_t) ? a_c : a_s;
    const double next = std::fabs(a_c - a_t) < std::fabs(a_s - a_t) ? a_c : a_s;
    const double lim = a_t + 0.66 * (a_u - a_t);
    if (a_t > a_l) return next < lim ? next : lim;  // std::min(lim, next)
    return lim < next ? next : lim;                 // std::max(lim, next)
  }
  const double z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u;
  const double w = std::sqrt(z * z - g_t * g_u);
  return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w);
}

}  // namespace nf
}  // namespace pclhip
