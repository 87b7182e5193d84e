// gicp_forms.hpp -- the closed forms of GeneralizedIterativeClosestPoint's Newton solver, written once for both sides
// (the host drives the solver; the kernels of gicp.hpp and the tests' restatement use the same definitions):
//   * applyState in float (registration/include/pcl/registration/impl/gicp.hpp:916-933)
//   * getRDerivatives / getR2ndDerivatives / computeRDerivative (impl/gicp.hpp:153-290)
//   * the assembly of dfddf's gradient and Hessian from the per-pair sums (impl/gicp.hpp:612-750)
//   * invert3x3SymMatrix (common/include/pcl/common/impl/eigen.hpp:434-466)
//   * the Newton step of estimateRigidTransformationNewton (impl/gicp.hpp:418-434) with a cyclic Jacobi eigen-solve
//
// The per-pair sums: the 60 that depend only on the pairs and their Mahalanobis matrices M (fixed for an outer
// iteration, summed ONCE by the pack pass) and the 12 + 1 that change with x (summed by the evaluation passes).
// Layout of the cached record (kGicpCached doubles):
//   [0]        number of pairs m
//   [1..6]     sum M                     (m00 m01 m02 m11 m12 m22)
//   [7..24]    sum p_c * M, c = 0,1,2    (dCost_dR_T{1,2,3}b, 6 each, same order)
//   [25..60]   hessian_rot_tmp: sum p_a p_b * M over the 6 products (aa ab ac bb bc cc) x the 6 entries of M
// Layout of the x-dependent record (kGicpEval doubles): [0] f = sum d'Md, [1..3] sum Md, [4..12] sum p (Md)' row-major.
#pragma once

#include <cmath>

#include "closed_forms.hpp"

namespace pclhip {
namespace gf {

constexpr int kGicpCached = 61;
constexpr int kGicpEval = 13;
constexpr int kGicpCandidates = 10;  // line-search tries of impl/gicp.hpp:437 (alpha = 1, 1/2, ...)

// index of (r, c) of a symmetric 3x3 in the 6-entry layout m00 m01 m02 m11 m12 m22
PCLHIP_HD int sym6(int r, int c) {
  const int a = r < c ? r : c, b = r < c ? c : r;
  return a == 0 ? b : (a == 1 ? 2 + b : 5);
}

// Eigen::AngleAxis<float> -> Quaternion (Geometry/Quaternion.h: w = cos(a/2), vec = sin(a/2) axis), the product
// AngleAxis(z) * AngleAxis(y) * AngleAxis(x), then toRotationMatrix (Geometry/Quaternion.h), in the reference's float
// operation order.  DEVIATION: the reference takes std::sin / std::cos of the float half angle in float; here they are
// taken in double and rounded to float, so that the host, the device and the tests' numpy restatement get the same float
// (libm float sin / cos differ between implementations in the last ulp).  The result differs from the reference's by at
// most an ulp of the rotation entries.
PCLHIP_HD void apply_state(const double x[6], float T[16]) {
  float q[3][4];  // (w, x, y, z) of the rotations about z, y, x
  for (int a = 0; a < 3; ++a) {
    const float ang = float(x[5 - a]);
    const float ha = 0.5f * ang;
    const float c = float(cos(double(ha))), s = float(sin(double(ha)));
    q[a][0] = c;
    q[a][1] = a == 2 ? s : 0.0f;
    q[a][2] = a == 1 ? s : 0.0f;
    q[a][3] = a == 0 ? s : 0.0f;
  }
  float r[4] = {q[0][0], q[0][1], q[0][2], q[0][3]};
  for (int a = 1; a < 3; ++a) {
    const float* b = q[a];
    float o[4];
    o[0] = r[0] * b[0] - r[1] * b[1] - r[2] * b[2] - r[3] * b[3];
    o[1] = r[0] * b[1] + r[1] * b[0] + r[2] * b[3] - r[3] * b[2];
    o[2] = r[0] * b[2] + r[2] * b[0] + r[3] * b[1] - r[1] * b[3];
    o[3] = r[0] * b[3] + r[3] * b[0] + r[1] * b[2] - r[2] * b[1];
    for (int k = 0; k < 4; ++k) r[k] = o[k];
  }
  const float w = r[0], qx = r[1], qy = r[2], qz = r[3];
  const float tx = 2.0f * qx, ty = 2.0f * qy, tz = 2.0f * qz;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const float tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  T[0] = 1.0f - (tyy + tzz);
  T[1] = txy - twz;
  T[2] = txz + twy;
  T[4] = txy + twz;
  T[5] = 1.0f - (txx + tzz);
  T[6] = tyz - twx;
  T[8] = txz - twy;
  T[9] = tyz + twx;
  T[10] = 1.0f - (txx + tyy);
  T[3] = float(x[0]);
  T[7] = float(x[1]);
  T[11] = float(x[2]);
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}

// x from a float transform (impl/gicp.hpp:391-401).  DEVIATION: the reference's atan2 takes the float entries and
// returns float (std::atan2(float, float)); here it is evaluated in double (asin is double in both), for the same
// reason as apply_state's sin / cos: a difference at the ulp level of a float angle.
PCLHIP_HD void state_from(const float T[16], double x[6]) {
  x[0] = T[3];
  x[1] = T[7];
  x[2] = T[11];
  x[3] = atan2(double(T[9]), double(T[10]));
  double s = -double(T[8]);
  s = s > 1.0 ? 1.0 : (s < -1.0 ? -1.0 : s);
  x[4] = asin(s);
  x[5] = atan2(double(T[4]), double(T[0]));
}

// dR/dphi, dR/dtheta, dR/dpsi (impl/gicp.hpp:153-199), row-major 3x3 each
PCLHIP_HD void r_derivatives(double phi, double theta, double psi, double d[3][9]) {
  const double cphi = cos(phi), sphi = sin(phi), ctheta = cos(theta), stheta = sin(theta), cpsi = cos(psi), spsi = sin(psi);
  double* a = d[0];
  a[0] = 0.; a[3] = 0.; a[6] = 0.;
  a[1] = sphi * spsi + cphi * cpsi * stheta; a[4] = -cpsi * sphi + cphi * spsi * stheta; a[7] = cphi * ctheta;
  a[2] = cphi * spsi - cpsi * sphi * stheta; a[5] = -cphi * cpsi - sphi * spsi * stheta; a[8] = -ctheta * sphi;
  double* b = d[1];
  b[0] = -cpsi * stheta; b[3] = -spsi * stheta; b[6] = -ctheta;
  b[1] = cpsi * ctheta * sphi; b[4] = ctheta * sphi * spsi; b[7] = -sphi * stheta;
  b[2] = cphi * cpsi * ctheta; b[5] = cphi * ctheta * spsi; b[8] = -cphi * stheta;
  double* c = d[2];
  c[0] = -ctheta * spsi; c[3] = cpsi * ctheta; c[6] = 0.;
  c[1] = -cphi * cpsi - sphi * spsi * stheta; c[4] = -cphi * spsi + cpsi * sphi * stheta; c[7] = 0.;
  c[2] = cpsi * sphi - cphi * spsi * stheta; c[5] = sphi * spsi + cphi * cpsi * stheta; c[8] = 0.;
}

// second derivatives (impl/gicp.hpp:214-290): pp, pt, ps, tt, ts, ss (phi, theta, psi)
PCLHIP_HD void r_2nd_derivatives(double phi, double theta, double psi, double d[6][9]) {
  const double sphi = sin(phi), stheta = sin(theta), spsi = sin(psi), cphi = cos(phi), ctheta = cos(theta), cpsi = cos(psi);
  double* a = d[0];
  a[0] = 0.0; a[3] = 0.0; a[6] = 0.0;
  a[1] = -cpsi * stheta * sphi + spsi * cphi; a[4] = -cpsi * cphi - spsi * stheta * sphi; a[7] = -ctheta * sphi;
  a[2] = -spsi * sphi - cpsi * stheta * cphi; a[5] = -spsi * stheta * cphi + cpsi * sphi; a[8] = -ctheta * cphi;
  double* b = d[1];
  b[0] = 0.0; b[3] = 0.0; b[6] = 0.0;
  b[1] = cpsi * ctheta * cphi; b[4] = spsi * ctheta * cphi; b[7] = -stheta * cphi;
  b[2] = -cpsi * ctheta * sphi; b[5] = -spsi * ctheta * sphi; b[8] = stheta * sphi;
  double* c = d[2];
  c[0] = 0.0; c[3] = 0.0; c[6] = 0.0;
  c[1] = -spsi * stheta * cphi + cpsi * sphi; c[4] = spsi * sphi + cpsi * stheta * cphi; c[7] = 0.0;
  c[2] = cpsi * cphi + spsi * stheta * sphi; c[5] = -cpsi * stheta * sphi + spsi * cphi; c[8] = 0.0;
  double* e = d[3];
  e[0] = -cpsi * ctheta; e[3] = -spsi * ctheta; e[6] = stheta;
  e[1] = -cpsi * stheta * sphi; e[4] = -spsi * stheta * sphi; e[7] = -ctheta * sphi;
  e[2] = -cpsi * stheta * cphi; e[5] = -spsi * stheta * cphi; e[8] = -ctheta * cphi;
  double* f = d[4];
  f[0] = spsi * stheta; f[3] = -cpsi * stheta; f[6] = 0.0;
  f[1] = -spsi * ctheta * sphi; f[4] = cpsi * ctheta * sphi; f[7] = 0.0;
  f[2] = -spsi * ctheta * cphi; f[5] = cpsi * ctheta * cphi; f[8] = 0.0;
  double* g = d[5];
  g[0] = -cpsi * ctheta; g[3] = -spsi * ctheta; g[6] = 0.0;
  g[1] = -cpsi * stheta * sphi + spsi * cphi; g[4] = -cpsi * cphi - spsi * stheta * sphi; g[7] = 0.0;
  g[2] = -spsi * sphi - cpsi * stheta * cphi; g[5] = -spsi * stheta * cphi + cpsi * sphi; g[8] = 0.0;
}

// trace(A * B) of row-major 3x3
PCLHIP_HD double trace_ab(const double* A, const double* B) {
  double t = 0.0;
  for (int i = 0; i < 3; ++i) {
    double s = 0.0;
    for (int k = 0; k < 3; ++k) s += A[3 * i + k] * B[3 * k + i];
    t += s;
  }
  return t;
}

// OptimizationFunctorWithIndices::dfddf (impl/gicp.hpp:612-750) from the cached record C and the x-dependent record E:
// f (= operator(), divided by m), gradient g[6], Hessian H[36] row-major
PCLHIP_HD void assemble(const double* C, const double* E, const double x[6], double* f, double g[6], double H[36]) {
  const double m = C[0];
  const double s = 2.0 / m;
  double dR[3][9], ddR[6][9];
  r_derivatives(x[3], x[4], x[5], dR);
  r_2nd_derivatives(x[3], x[4], x[5], ddR);
  *f = E[0] / m;
  for (int i = 0; i < 36; ++i) H[i] = 0.0;
  for (int r = 0; r < 3; ++r) g[r] = E[1 + r] * s;
  double dCost_dR_T[9];
  for (int i = 0; i < 9; ++i) dCost_dR_T[i] = E[4 + i] * s;
  for (int a = 0; a < 3; ++a) g[3 + a] = trace_ab(dR[a], dCost_dR_T);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) H[6 * r + c] = C[1 + sym6(r, c)] * s;
  // dCost_dR_T{1,2,3}: row r of T_k = column k of dCost_dR_T{r+1}b = (p_r M)(., k): element (r, c) = sum p_r M(c, k)
  double T3[3][9];
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) T3[k][3 * r + c] = C[7 + 6 * r + sym6(c, k)] * s;
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) {
      H[6 * (3 + a) + k] = trace_ab(dR[a], T3[k]);
      H[6 * k + 3 + a] = H[6 * (3 + a) + k];
    }
  // rotation-rotation: hessian_rot_tmp(3j + i, l') = sum M(i, j) * pp[l'] (M stored column-major in the reference; M symmetric)
  const int lookup[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  double hrot[3][9];  // phi, theta, psi: (i, l) row-major
  for (int l = 0; l < 3; ++l)
    for (int i = 0; i < 3; ++i) {
      double acc[3] = {0.0, 0.0, 0.0};
      for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) {
          const double h = C[25 + 6 * lookup[l][k] + sym6(i, j)];
          for (int a = 0; a < 3; ++a) acc[a] += h * dR[a][3 * j + k];
        }
      for (int a = 0; a < 3; ++a) hrot[a][3 * i + l] = acc[a] * s;
    }
  // trace(dR_a^T * hrot_b) = sum_ij dR_a(i, j) hrot_b(i, j)
  auto tr_t = [&](int a, int b) {
    double t = 0.0;
    for (int i = 0; i < 3; ++i) {
      double u = 0.0;
      for (int k = 0; k < 3; ++k) u += dR[a][3 * k + i] * hrot[b][3 * k + i];
      t += u;
    }
    return t;
  };
  const int pair_of[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) {
      const double v = tr_t(a, b) + trace_ab(ddR[pair_of[a][b]], dCost_dR_T);
      H[6 * (3 + a) + 3 + b] = v;
      H[6 * (3 + b) + 3 + a] = v;
    }
}

// invert3x3SymMatrix (common/include/pcl/common/impl/eigen.hpp:434-466) on a 3x3 given row-major; the reference reads
// Eigen's column-major coefficients: coeff(k) = A(k % 3, k / 3).  Returns det; out (6 entries) is written when det != 0.
PCLHIP_HD double invert3x3_sym(const double A[9], double out[6]) {
  auto cf_ = [&](int k) { return A[3 * (k % 3) + k / 3]; };
  const double fd_ee = cf_(4) * cf_(8) - cf_(7) * cf_(5);
  const double ce_bf = cf_(2) * cf_(5) - cf_(1) * cf_(8);
  const double be_cd = cf_(1) * cf_(5) - cf_(2) * cf_(4);
  const double det = cf_(0) * fd_ee + cf_(1) * ce_bf + cf_(2) * be_cd;
  if (det != 0) {
    out[0] = fd_ee / det;                                 // (0,0)
    out[1] = ce_bf / det;                                 // (0,1)
    out[2] = be_cd / det;                                 // (0,2)
    out[3] = (cf_(0) * cf_(8) - cf_(2) * cf_(2)) / det;   // (1,1)
    out[4] = (cf_(1) * cf_(2) - cf_(0) * cf_(5)) / det;   // (1,2)
    out[5] = (cf_(0) * cf_(4) - cf_(1) * cf_(1)) / det;   // (2,2)
  }
  return det;
}

// The Newton direction of impl/gicp.hpp:418-434: delta = V diag(1/ev') V^T g, ev' = ev, or 1/largest eigenvalue where ev
// is negative.  Cyclic Jacobi on the symmetric 6x6 (fp64, converged to the rounding level).
PCLHIP_HD void newton_step(const double H[36], const double g[6], double delta[6]) {
  double A[6][6], V[6][6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      A[i][j] = H[6 * i + j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < 6; ++p) {
      diag += A[p][p] * A[p][p];
      for (int q = p + 1; q < 6; ++q) off += A[p][q] * A[p][q];
    }
    if (off <= 1e-36 * diag || off == 0.0) break;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 6; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - sn * akq;
          A[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - sn * aqk;
          A[q][k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < 6; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - sn * vkq;
          V[k][q] = sn * vkp + c * vkq;
        }
      }
  }
  double largest = A[0][0];
  for (int i = 1; i < 6; ++i) largest = A[i][i] > largest ? A[i][i] : largest;
  double inv[6], vg[6];
  for (int i = 0; i < 6; ++i) {
    inv[i] = A[i][i] < 0 ? 1.0 / largest : 1.0 / A[i][i];
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += V[k][i] * g[k];
    vg[i] = s * inv[i];
  }
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
    for (int i = 0; i < 6; ++i) s += V[r][i] * vg[i];
    delta[r] = s;
  }
}

}  // namespace gf
}  // namespace pclhip
