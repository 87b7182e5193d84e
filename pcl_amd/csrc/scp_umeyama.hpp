// scp_umeyama.hpp -- pcl::umeyama without scaling (common/include/pcl/common/impl/eigen.hpp:675-738) for the few pairs of a
// sample, in double, written once for SampleConsensusPrerejective's hypotheses (scp.hpp) and for the registration model of
// CorrespondenceRejectorSampleConsensus (rejector_sac.hpp).
#pragma once

#include <cmath>

#include "closed_forms.hpp"

namespace pclhip {

// The rotation of umeyama (eigen.hpp:700-724), R = U S V^T with S = diag(1, 1, det(U) det(V)), for the sigma of a few pairs.
// Three pairs give a sigma of rank two and two pairs one of rank one: the last singular directions carry no information,
// and U S V^T is u0 v0^T + u1 v1^T + (u0 x u1)(v0 x v1)^T whatever their signs.  V and the singular values come from the
// Jacobi eigen-decomposition of sigma^T sigma (cf::jacobi_eig3), u_i = sigma v_i / |sigma v_i|; a second singular value
// below 1e-7 of the first (the noise floor of a square root of an eigenvalue) counts as zero and u1 is any unit vector
// orthogonal to u0.
PCLHIP_HD void scp_rotation(const double sigma[3][3], double R[3][3]) {
  double AtA[3][3], V[3][3], w[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double a = 0;
      for (int k = 0; k < 3; ++k) a += sigma[k][i] * sigma[k][j];
      AtA[i][j] = a;
    }
  cf::jacobi_eig3(AtA, V, w);
  int i0 = 0, i1 = 1, i2 = 2;  // descending eigenvalues
  if (w[i1] > w[i0]) cf::swap_(i0, i1);
  if (w[i2] > w[i0]) cf::swap_(i0, i2);
  if (w[i2] > w[i1]) cf::swap_(i1, i2);
  double v0[3], v1[3], v2[3], u0[3], u1[3], u2[3];
  for (int r = 0; r < 3; ++r) {
    v0[r] = V[r][i0];
    v1[r] = V[r][i1];
  }
  cf::cross3(v0, v1, v2);
  double n0 = 0, n1 = 0;
  for (int r = 0; r < 3; ++r) {
    u0[r] = sigma[r][0] * v0[0] + sigma[r][1] * v0[1] + sigma[r][2] * v0[2];
    u1[r] = sigma[r][0] * v1[0] + sigma[r][1] * v1[1] + sigma[r][2] * v1[2];
    n0 += u0[r] * u0[r];
    n1 += u1[r] * u1[r];
  }
  n0 = sqrt(n0);
  n1 = sqrt(n1);
  if (!(n0 > 0)) {  // sigma == 0 (coincident points): the identity
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
    return;
  }
  for (int r = 0; r < 3; ++r) u0[r] /= n0;
  if (n1 > 1e-7 * n0) {
    double d = 0, n = 0;
    for (int r = 0; r < 3; ++r) d += u1[r] * u0[r];
    for (int r = 0; r < 3; ++r) {
      u1[r] -= d * u0[r];
      n += u1[r] * u1[r];
    }
    n = sqrt(n);
    for (int r = 0; r < 3; ++r) u1[r] /= n;
  } else {
    const int mi = fabs(u0[0]) <= fabs(u0[1]) ? (fabs(u0[0]) <= fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
    const double e[3] = {mi == 0 ? 1.0 : 0.0, mi == 1 ? 1.0 : 0.0, mi == 2 ? 1.0 : 0.0};
    cf::cross3(u0, e, u1);
    const double n = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    for (int r = 0; r < 3; ++r) u1[r] /= n;
  }
  cf::cross3(u0, u1, u2);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = u0[i] * v0[j] + u1[i] * v1[j] + u2[i] * v2[j];
}

// TransformationEstimationSVD / SampleConsensusModelRegistration::estimateRigidTransformationSVD on ns pairs: the demeaned
// sigma in double, scp_rotation, t = mean(tgt) - R mean(src); rounded once to the float 4x4 T (row-major)
PCLHIP_HD void scp_umeyama(const float (*ps)[3], const float (*pt)[3], int ns, float* T) {
  double sm[3] = {0, 0, 0}, dm[3] = {0, 0, 0}, sigma[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, R[3][3];
  for (int i = 0; i < ns; ++i)
    for (int d = 0; d < 3; ++d) {
      sm[d] += double(ps[i][d]);
      dm[d] += double(pt[i][d]);
    }
  for (int d = 0; d < 3; ++d) {
    sm[d] /= double(ns);
    dm[d] /= double(ns);
  }
  for (int i = 0; i < ns; ++i)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) sigma[r][c] += (double(pt[i][r]) - dm[r]) * (double(ps[i][c]) - sm[c]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sigma[r][c] /= double(ns);
  scp_rotation(sigma, R);
  cf::zero16(T);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = float(R[i][j]);
    T[4 * i + 3] = float(dm[i] - (R[i][0] * sm[0] + R[i][1] * sm[1] + R[i][2] * sm[2]));
  }
  T[15] = 1.0f;
}

}  // namespace pclhip
