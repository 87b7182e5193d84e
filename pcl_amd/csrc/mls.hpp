// mls.hpp -- MovingLeastSquares without upsampling over the index (included by radius.hip).
// Replaces pcl::MovingLeastSquares<PointInT, PointOutT>::process / performProcessing / computeMLSPointNormal and
// pcl::MLSResult::computeMLSSurface / projectQueryPoint (surface/include/pcl/surface/mls.h, impl/mls.hpp) for
// setUpsamplingMethod(NONE), polynomial order 0, 1 or 2 and the projection methods NONE and SIMPLE: the search surface is
// the input, a neighbourhood every indexed point with float d2 < float(r * r), the point itself included (the relation of
// pclhip_radius_search).  Per indexed point q with m neighbours, in ascending original index:
//   1. m < 3: no output record
//   2. plane: centroid c and C = sum (p_j - c)(p_j - c)^T in double; the smallest eigenvalue l0 of C and its unit
//      eigenvector n; mean = q - ((q - c) . n) n; curvature = |l0 / trace(C)| (0 when the trace is 0);
//      v = unitOrthogonal(n) by Eigen's rule, u = n x v
//   3. fit (order 2 and m >= 6 only): d = p_j - mean, w = exp(-d.d / sqr_gauss_param), (u_j, v_j, f_j) = (d.u, d.v, d.n),
//      P_j = (1, v, v^2, u, uv, u^2); (sum w P P^T) coeff = sum w P f by Cholesky in double; a pivot that is not positive
//      or a coeff[0] that is not finite leaves the point with its plane
//   4. projection of the query: with a fit and SIMPLE, point = mean + coeff[0] n and
//      normal = normalize(n - coeff[3] u - coeff[1] v); otherwise point = mean, normal = n
//   5. one record per surviving point: xyz, (normal, curvature), the original index -- floats -- and, when asked for, the
//      unrounded doubles
// Everything between the loads and the emit is RELATIVE TO THE QUERY: e_j = p_j - q (exact in double), the record holds
// o = mean - q = ((sum e / m) . n) n, the fit's d is e_j - o, the fitted record o + coeff[0] n, and q is added once, in
// mls_emit_kernel.  A mean stored at the point's own coordinates would be rounded at |q| (2^-40 at 8192) and hand every
// neighbour of the fit that common error: far from the origin the normal then leaves its bound, which knows nothing of |q|.
// The point itself cannot escape one rounding at |q|: its bound carries the term 2 * 2^-53 * max_i |q_i| (include/pclhip.h).
// A positive radius whose float square is 0 gives every point an empty neighbourhood (fpfh.hpp's rule): no output, no
// walk.
//
// Pipeline (one stream, one read-back: the count):
//   mls_plane_kernel   one lane per indexed point in kd order: m, sum d and the six sums of d d^T over the hits of every
//                      staged leaf (d = p_j - q widened before the subtraction: |d| < r, so the one-pass form
//                      C = sum d d^T - (sum d)(sum d)^T / m loses nothing), then a cyclic Jacobi on named scalars that
//                      carries the rotation.  Writes the plane record (mean - q, n, curvature, m: 8 doubles) by kd position
//                      and the survivor flag by ORIGINAL index.  One writer per slot, no atomics.
//   mls_fit_kernel     the same walk again for the lanes with m >= 6 (a group of 64 without one is skipped): the 15
//                      moments sum w u^a v^b (a + b <= 4) and the 6 moments sum w f u^a v^b (a + b <= 2), from which the
//                      6 x 6 system is assembled (the reference's P diag(w) P^T up to summation order); Cholesky and the
//                      two triangular solves on constant indices.  A fitted lane overwrites its own record with the
//                      projected point (less q) and normal.  Not launched for order < 2 or the method NONE.
//   scan (device_scan.hpp) + mls_emit_kernel   stable compaction in original-index order, no atomic ticket; kd order ->
//                      original order through the index's rank array; point = q + the record's offset
// Both walks are traverse<Policy, true> with a fixed bound inside for_each_query_group: the order of the sums is a function
// of the index alone, two calls give the same bytes.  No wave waits for another; the Jacobi sweeps are capped.
//
// Deviations from the reference:
//   * the sign of n: the reference's eigen33 leaves it to its cross products (its own test compares abs(normal)); here the
//     component of n with the largest magnitude is positive, ties go to the lowest axis.  Points and curvature do not
//     depend on it
//   * the sums run in traversal order, one-pass and shifted by the query (the reference: ascending distance, two-pass); the
//     moments replace the matrix product
//   * the eigenvector comes from the Jacobi iteration below (the reference: the closed-form eigen33)
//   * non-finite records are neither queries nor neighbours and produce no output (the reference's valid = false branch
//     reads a stale num_neighbors)
//   * the index covers the whole unscaled cloud
//   * not built: the ORTHOGONAL projection (its Newton loop, impl/mls.hpp:551-579, ends on an absolute 1e-8 with no
//     iteration cap), order > 2, every upsampling method, setIndices, another search surface, cached MLS results
#pragma once

#include "device_scan.hpp"
#include "iss.hpp"      // iss_rotate
#include "outlier.hpp"  // OR_BLOCK, OR_WAVES, outlier_grid, or_blocks
#include "traverse.hpp"

namespace pclhip {
namespace {

constexpr int MLS_REC = 8;  // doubles per record: point / mean less the query (3), normal (3), curvature, m

// Pass 1: the neighbour count, the sum of d = p_j - q and the six sums of d d^T
struct MlsPlane {
  float t;
  double px, py, pz;
  uint32_t cnt, n;
  double sx, sy, sz;
  double cxx, cxy, cxz, cyy, cyz, czz;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return t; }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id == NO_INDEX) return;
    const float4* s = reinterpret_cast<const float4*>(buf) + slot;  // transposed staging
    uint32_t mask = leaf_hits_lt<16>(s, qx[0], qy[0], qz[0], t);
    const uint32_t base = leaf_id * uint32_t(LEAF);
    if (n - base < uint32_t(LEAF)) mask &= (1u << (n - base)) - 1u;  // the padding of the last leaf is no neighbour
    cnt += uint32_t(__builtin_popcount(mask));
    while (mask != 0) {
      const uint32_t j = uint32_t(__builtin_ctz(mask));
      mask &= mask - 1u;
      const double dx = double(leaf_coord<16>(s, 0, j)) - px;
      const double dy = double(leaf_coord<16>(s, 1, j)) - py;
      const double dz = double(leaf_coord<16>(s, 2, j)) - pz;
      sx += dx;
      sy += dy;
      sz += dz;
      cxx = fma(dx, dx, cxx);
      cxy = fma(dx, dy, cxy);
      cxz = fma(dx, dz, cxz);
      cyy = fma(dy, dy, cyy);
      cyz = fma(dy, dz, cyz);
      czz = fma(dz, dz, czz);
    }
  }
};

// iss_rotate's rotation applied to the columns p and q of the accumulated eigenvector matrix (one row per call)
__device__ __forceinline__ void mls_rotate_row(double c, double sn, double& vp, double& vq) {
  const double a = vp, b = vq;
  vp = c * a - sn * b;
  vq = sn * a + c * b;
}

// one Jacobi rotation in the (p, q) plane (iss_rotate) that also turns the three rows of V
__device__ __forceinline__ void mls_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                           double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
  const double c = 1.0 / sqrt(fma(tt, tt, 1.0)), sn = tt * c;
  app = fma(-tt, apq, app);
  aqq = fma(tt, apq, aqq);
  apq = 0.0;
  mls_rotate_row(c, sn, arp, arq);
  mls_rotate_row(c, sn, v0p, v0q);
  mls_rotate_row(c, sn, v1p, v1q);
  mls_rotate_row(c, sn, v2p, v2q);
}

// the smallest eigenvalue of the symmetric matrix (a00 a01 a02; . a11 a12; . . a22) and its unit eigenvector, the sign by
// the rule of the header.  Cyclic Jacobi as iss_eigenvalues, on named scalars (run-time-indexed 3 x 3 arrays are moved to
// LDS or scratch by the compiler: ndt_cells.hpp); equal eigenvalues give the lowest axis' column.
__device__ __forceinline__ void mls_smallest_eigenpair(double a00, double a01, double a02, double a11, double a12, double a22,
                                                       double& l0, double& nx, double& ny, double& nz) {
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = fabs(a01) + fabs(a02) + fabs(a12);
    const double dia = fabs(a00) + fabs(a11) + fabs(a22);
    if (!(off > 1e-20 * dia)) break;  // (a NaN ends the loop as well)
    mls_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    mls_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    mls_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  l0 = a00; nx = v00; ny = v10; nz = v20;
  if (a11 < l0) { l0 = a11; nx = v01; ny = v11; nz = v21; }
  if (a22 < l0) { l0 = a22; nx = v02; ny = v12; nz = v22; }
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  nx /= len; ny /= len; nz /= len;
  const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
  const double lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
  if (lead < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
}

// Eigen's unitOrthogonal for 3-vectors (Eigen/src/Geometry/OrthoMethods.h; isMuchSmallerThan at 1e-12), then u = n x v
__device__ __forceinline__ void mls_frame(double nx, double ny, double nz, double& ux, double& uy, double& uz, double& vx,
                                          double& vy, double& vz) {
  if (!(fabs(nx) <= fabs(nz) * 1e-12) || !(fabs(ny) <= fabs(nz) * 1e-12)) {
    const double h = sqrt(nx * nx + ny * ny);
    vx = -ny / h; vy = nx / h; vz = 0.0;
  } else {
    const double h = sqrt(ny * ny + nz * nz);
    vx = 0.0; vy = -nz / h; vz = ny / h;
  }
  ux = ny * vz - nz * vy;
  uy = nz * vx - nx * vz;
  uz = nx * vy - ny * vx;
}

// waves per SIMD (kernel-resource-usage, gfx950): see DESIGN.md row f-13
__global__ __launch_bounds__(OR_BLOCK) void mls_plane_kernel(IndexView ix, float t, double* __restrict__ rec,
                                                             uint32_t* __restrict__ flag) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, nullptr, ix.n, [&](uint32_t pos, bool real, float4 p) {
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {real};
    MlsPlane pol;
    pol.t = t;
    pol.n = ix.n;
    pol.px = double(p.x); pol.py = double(p.y); pol.pz = double(p.z);
    pol.cnt = 0;
    pol.sx = pol.sy = pol.sz = 0.0;
    pol.cxx = pol.cxy = pol.cxz = pol.cyy = pol.cyz = pol.czz = 0.0;
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a point
    traverse<MlsPlane, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (!real) return;
    double* r = rec + size_t(pos) * MLS_REC;
    const double m = double(pol.cnt);
    r[7] = m;
    if (pol.cnt < 3u) return;  // no output record: nobody reads the rest
    const double a00 = pol.cxx - pol.sx * pol.sx / m, a01 = pol.cxy - pol.sx * pol.sy / m, a02 = pol.cxz - pol.sx * pol.sz / m;
    const double a11 = pol.cyy - pol.sy * pol.sy / m, a12 = pol.cyz - pol.sy * pol.sz / m, a22 = pol.czz - pol.sz * pol.sz / m;
    const double trace = a00 + a11 + a22;
    double l0, nx, ny, nz;
    mls_smallest_eigenpair(a00, a01, a02, a11, a12, a22, l0, nx, ny, nz);
    // q - c = -(sum d) / m; the record keeps o = mean - q: q, and with it the rounding at |q|, joins in mls_emit_kernel
    const double dist = -(pol.sx / m * nx + pol.sy / m * ny + pol.sz / m * nz);
    r[0] = -dist * nx;
    r[1] = -dist * ny;
    r[2] = -dist * nz;
    r[3] = nx;
    r[4] = ny;
    r[5] = nz;
    r[6] = trace != 0.0 ? fabs(l0 / trace) : 0.0;
    flag[__float_as_uint(p.w)] = 1u;
  });
}

// Pass 2: the weighted moments of the neighbours in the lane's plane frame.  muv: sum w u^a v^b, fuv: sum w f u^a v^b
struct MlsFit {
  float t;
  uint32_t n;
  double mx, my, mz;  // o = mean - q
  double nx, ny, nz, ux, uy, uz, vx, vy, vz;
  double inv_sg;
  double m00, m01, m02, m03, m04, m10, m11, m12, m13, m20, m21, m22, m30, m31, m40;
  double f00, f01, f02, f10, f11, f20;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return t; }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id == NO_INDEX) return;
    const float4* s = reinterpret_cast<const float4*>(buf) + slot;
    uint32_t mask = leaf_hits_lt<16>(s, qx[0], qy[0], qz[0], t);
    const uint32_t base = leaf_id * uint32_t(LEAF);
    if (n - base < uint32_t(LEAF)) mask &= (1u << (n - base)) - 1u;
    while (mask != 0) {
      const uint32_t j = uint32_t(__builtin_ctz(mask));
      mask &= mask - 1u;
      // p_j - q is exact in double (two floats); a mean rounded at |q| never enters: a cloud at 8192 keeps its bound
      const double dx = (double(leaf_coord<16>(s, 0, j)) - double(qx[0])) - mx;
      const double dy = (double(leaf_coord<16>(s, 1, j)) - double(qy[0])) - my;
      const double dz = (double(leaf_coord<16>(s, 2, j)) - double(qz[0])) - mz;
      const double w = exp(-(dx * dx + dy * dy + dz * dz) * inv_sg);
      const double u = dx * ux + dy * uy + dz * uz;
      const double v = dx * vx + dy * vy + dz * vz;
      const double f = dx * nx + dy * ny + dz * nz;
      const double wv = w * v, wu = w * u, wf = w * f;
      const double wvv = wv * v, wuv = wu * v, wuu = wu * u;
      const double wvvv = wvv * v, wuvv = wuv * v, wuuv = wuu * v, wuuu = wuu * u;
      m00 += w;
      m01 += wv;
      m10 += wu;
      m02 += wvv;
      m11 += wuv;
      m20 += wuu;
      m03 += wvvv;
      m12 += wuvv;
      m21 += wuuv;
      m30 += wuuu;
      m04 = fma(wvvv, v, m04);
      m13 = fma(wuvv, v, m13);
      m22 = fma(wuuv, v, m22);
      m31 = fma(wuuu, v, m31);
      m40 = fma(wuuu, u, m40);
      f00 += wf;
      f01 = fma(wf, v, f01);
      f10 = fma(wf, u, f10);
      f02 = fma(wf * v, v, f02);
      f11 = fma(wf * u, v, f11);
      f20 = fma(wf * u, u, f20);
    }
  }
};

// A x = b for the symmetric 6 x 6 matrix whose lower triangle is in a (row-major, full storage), by Cholesky; every index
// is a constant after unrolling, the arrays live in registers.  -> false when a pivot is not positive (NaN included).
__device__ __forceinline__ bool mls_cholesky_solve6(double (&a)[6][6], double (&b)[6]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = a[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= a[j][k] * a[j][k];
    ok = ok && d > 0.0;
    const double l = sqrt(d);
    a[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = a[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= a[i][k] * a[j][k];
      a[i][j] = s / l;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {  // L y = b
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= a[i][k] * b[k];
    b[i] = s / a[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {  // L^T x = y
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= a[k][i] * b[k];
    b[i] = s / a[i][i];
  }
  return ok;
}

// waves per SIMD (kernel-resource-usage, gfx950): see DESIGN.md row f-13
__global__ __launch_bounds__(OR_BLOCK) void mls_fit_kernel(IndexView ix, float t, double sqr_gauss_param,
                                                           double* __restrict__ rec) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, nullptr, ix.n, [&](uint32_t pos, bool real, float4 p) {
    double* r = rec + size_t(pos) * MLS_REC;
    const bool fits = real && r[7] >= 6.0;
    if (__builtin_amdgcn_ballot_w64(fits) == 0) return;  // every record of the group stays the plane's
    MlsFit pol;
    pol.t = t;
    pol.n = ix.n;
    pol.inv_sg = 1.0 / sqr_gauss_param;
    pol.mx = fits ? r[0] : 0.0; pol.my = fits ? r[1] : 0.0; pol.mz = fits ? r[2] : 0.0;
    pol.nx = fits ? r[3] : 0.0; pol.ny = fits ? r[4] : 0.0; pol.nz = fits ? r[5] : 1.0;
    mls_frame(pol.nx, pol.ny, pol.nz, pol.ux, pol.uy, pol.uz, pol.vx, pol.vy, pol.vz);
    pol.m00 = pol.m01 = pol.m02 = pol.m03 = pol.m04 = pol.m10 = pol.m11 = pol.m12 = pol.m13 = 0.0;
    pol.m20 = pol.m21 = pol.m22 = pol.m30 = pol.m31 = pol.m40 = 0.0;
    pol.f00 = pol.f01 = pol.f02 = pol.f10 = pol.f11 = pol.f20 = 0.0;
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {fits};
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a point
    traverse<MlsFit, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (!fits) return;
    // P = (1, v, v^2, u, uv, u^2): entry (k, l) of sum w P P^T is the moment of the summed exponents
    double a[6][6], b[6];
    a[0][0] = pol.m00;
    a[1][0] = pol.m01; a[1][1] = pol.m02;
    a[2][0] = pol.m02; a[2][1] = pol.m03; a[2][2] = pol.m04;
    a[3][0] = pol.m10; a[3][1] = pol.m11; a[3][2] = pol.m12; a[3][3] = pol.m20;
    a[4][0] = pol.m11; a[4][1] = pol.m12; a[4][2] = pol.m13; a[4][3] = pol.m21; a[4][4] = pol.m22;
    a[5][0] = pol.m20; a[5][1] = pol.m21; a[5][2] = pol.m22; a[5][3] = pol.m30; a[5][4] = pol.m31; a[5][5] = pol.m40;
    b[0] = pol.f00; b[1] = pol.f01; b[2] = pol.f02; b[3] = pol.f10; b[4] = pol.f11; b[5] = pol.f20;
    if (!mls_cholesky_solve6(a, b) || !isfinite(b[0])) return;
    double ox = pol.nx - b[3] * pol.ux - b[1] * pol.vx;
    double oy = pol.ny - b[3] * pol.uy - b[1] * pol.vy;
    double oz = pol.nz - b[3] * pol.uz - b[1] * pol.vz;
    const double len = sqrt(ox * ox + oy * oy + oz * oz);
    r[0] = pol.mx + b[0] * pol.nx;
    r[1] = pol.my + b[0] * pol.ny;
    r[2] = pol.mz + b[0] * pol.nz;
    r[3] = ox / len;
    r[4] = oy / len;
    r[5] = oz / len;
  });
}

// the records of the ids i with flag[i] != 0, ascending (excl: exclusive scan of flag), kd order -> original order by rank;
// what does not fit the caller's capacity is dropped.  The record's offset o (or o + coeff[0] n) becomes the point here:
// q + offset, the one operation of the call that rounds at |q|
__global__ __launch_bounds__(OR_BLOCK) void mls_emit_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl,
                                                            const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                            const float4* __restrict__ pts,
                                                            const double* __restrict__ rec, float* __restrict__ out_points,
                                                            float* __restrict__ out_normals, int32_t* __restrict__ out_indices,
                                                            double* __restrict__ out_double, uint64_t capacity) {
  const uint64_t i = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  if (i >= n_orig || flag[i] == 0u) return;
  const uint64_t e = excl[i];
  if (e >= capacity) return;
  const uint32_t pos = rank[i];
  const double* r = rec + size_t(pos) * MLS_REC;
  const float4 q = pts[pos];
  const double point[3] = {double(q.x) + r[0], double(q.y) + r[1], double(q.z) + r[2]};
  if (out_points != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_points[e * 3 + k] = float(point[k]);
  }
  if (out_normals != nullptr) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out_normals[e * 4 + k] = float(r[3 + k]);
  }
  if (out_indices != nullptr) out_indices[e] = int32_t(i);
  if (out_double != nullptr) {
#pragma unroll
    for (int k = 0; k < MLS_REC; ++k) out_double[e * MLS_REC + k] = k < 3 ? point[k] : r[k];
  }
}

}  // namespace

// The host side of pclhip_mls_process (api.hip): t is the float square of the search radius, `fit` whether the polynomial
// pass runs (order 2 with the SIMPLE projection).
pclhip_status mls_process(pclhip_index* ix, float t, double sqr_gauss_param, bool fit, float* out_points, float* out_normals,
                          int32_t* out_indices, uint64_t capacity, uint64_t* n_out, double* out_double) {
  pclhip_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const uint64_t n_orig = ix->n_orig;
  const uint32_t n = ix->n;
  *n_out = 0;
  ix->mls_pass_ms[0] = ix->mls_pass_ms[1] = 0.0;
  if (n_orig == 0 || n == 0 || !(t > 0.0f)) return PCLHIP_OK;  // nothing lies within d2 < 0: m = 0 < 3 everywhere
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  DeviceScope scope(ctx);
  uint32_t *tot = nullptr, *flag = nullptr, *excl = nullptr;
  uint2* part = nullptr;
  double* rec = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&tot, 16));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&flag, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&excl, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((n_orig + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rec, size_t(n) * MLS_REC * 8));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(tot, 0, 16, s));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(flag, 0, size_t(n_orig) * 4, s));
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.event(&e0));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e1));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e2));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e3));
  const IndexView v = ix->view();
  (void)hipEventRecord(e0, s);
  PCLHIP_LAUNCH_FED(ctx, mls_plane_kernel, dim3(outlier_grid(ctx, mls_plane_kernel, n)), dim3(OR_BLOCK), 0, s, v, t, rec, flag);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  (void)hipEventRecord(e1, s);
  if (fit) {
    PCLHIP_LAUNCH_FED(ctx, mls_fit_kernel, dim3(outlier_grid(ctx, mls_fit_kernel, n)), dim3(OR_BLOCK), 0, s, v, t,
                      sqr_gauss_param, rec);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  (void)hipEventRecord(e2, s);
  launch_scan_u32(s, flag, n_orig, part, tot, excl);
  const uint64_t cap = capacity < n_orig ? capacity : n_orig;
  const bool pts_dev = out_points != nullptr && is_device_pointer(out_points);
  const bool nrm_dev = out_normals != nullptr && is_device_pointer(out_normals);
  const bool idx_dev = out_indices != nullptr && is_device_pointer(out_indices);
  const bool dbl_dev = out_double != nullptr && is_device_pointer(out_double);
  float *d_pts = out_points, *d_nrm = out_normals;
  int32_t* d_idx = out_indices;
  double* d_dbl = out_double;
  if (cap > 0) {
    if (out_points != nullptr && !pts_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_pts, size_t(cap) * 12));
    if (out_normals != nullptr && !nrm_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_nrm, size_t(cap) * 16));
    if (out_indices != nullptr && !idx_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_idx, size_t(cap) * 4));
    if (out_double != nullptr && !dbl_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_dbl, size_t(cap) * MLS_REC * 8));
    hipLaunchKernelGGL(mls_emit_kernel, or_blocks(n_orig), dim3(OR_BLOCK), 0, s, flag, excl, ix->rank, n_orig, v.pts, rec, d_pts,
                       d_nrm, d_idx, d_dbl, cap);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  (void)hipEventRecord(e3, s);
  uint32_t h[4] = {0, 0, 0, 0};
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(h, tot, 16, hipMemcpyDeviceToHost, s));  // the count: the call's one read-back
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t count = h[0];
  const uint64_t kept = count < cap ? count : cap;
  if (kept > 0) {
    if (out_points != nullptr && !pts_dev)
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_points, d_pts, size_t(kept) * 12, hipMemcpyDeviceToHost, s));
    if (out_normals != nullptr && !nrm_dev)
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_normals, d_nrm, size_t(kept) * 16, hipMemcpyDeviceToHost, s));
    if (out_indices != nullptr && !idx_dev)
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_indices, d_idx, size_t(kept) * 4, hipMemcpyDeviceToHost, s));
    if (out_double != nullptr && !dbl_dev)
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_double, d_dbl, size_t(kept) * MLS_REC * 8, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  }
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, e0, e3) == hipSuccess) ix->last_kernel_ms = ms;
  if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ix->mls_pass_ms[0] = ms;
  if (hipEventElapsedTime(&ms, e1, e2) == hipSuccess) ix->mls_pass_ms[1] = ms;
  *n_out = count;
  if (count > capacity) {
    set_error(ctx, "mls: more output records than the capacity of the output buffers");
    return PCLHIP_ERR_OVERFLOW;
  }
  return PCLHIP_OK;
}

}  // namespace pclhip
