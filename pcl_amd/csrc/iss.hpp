// iss.hpp -- ISSKeypoint3D without boundary estimation over the index (included by radius.hip).
// Replaces pcl::ISSKeypoint3D<PointInT, PointOutT>::getScatterMatrix and ::detectKeypoints
// (keypoints/include/pcl/keypoints/impl/iss_3d.hpp:164-208, 302-473) for border_radius == 0: the search surface is the
// input, a neighbourhood every indexed point with float d2 < float(r * r), the point itself included (the relation of
// pclhip_radius_search).
//   1. per point i with m >= min_neighbors points within the salient radius: C = sum (p_j - p_i)(p_j - p_i)^T, the
//      coordinates widened to double before the subtraction, six sums in double; eigenvalues e1 >= e2 >= e3 in double;
//      s_i = e3 iff e2 / e1 < gamma_21 && e3 / e2 < gamma_32 (a NaN ratio fails), else 0
//   2. a point with s_i > 0 is a keypoint iff its non-max-radius neighbourhood holds >= min_neighbors points and none of
//      them has s_i < s_j (strict: equal saliencies all win)
//   3. the keypoints' original indices, ascending
// A positive radius whose float square is 0 gives every point an empty neighbourhood (fpfh.hpp's rule): m = 0, no
// keypoints, no walk.
//
// Pipeline (one stream, one read-back: the count):
//   iss_scatter_kernel   one lane per indexed point in kd order: the six sums over the hits of every staged leaf (the lane
//                        walks its own hit mask, as FpfhSpfh::leaf_lane), then a cyclic Jacobi on named scalars; s (and,
//                        when asked for, the three eigenvalues) in kd order.  One writer per slot, no atomics.
//   iss_nms_kernel       one lane per indexed point; a group of 64 with no salient lane is skipped; per hit the neighbour's s
//                        is read by its kd position (a leaf's 16 values: 128 contiguous bytes); a lane that has seen a larger
//                        neighbour reports a negative bound and leaves the walk (RorCount's way: it is no maximum, so its
//                        count no longer matters).  The flag goes to the point's ORIGINAL index.
//   scan (device_scan.hpp) + iss_emit_kernel   stable compaction in original-index order: ascending, no atomic ticket
//   iss_gather_kernel    the optional outputs, kd order -> original order
// Both walks are traverse<Policy, true> with a fixed bound inside for_each_query_group: the order of the sums is a function
// of the index alone, two calls give the same bytes.  No wave waits for another.
//
// Deviations from the reference:
//   * a point with e3 < 0 or a non-finite eigenvalue is not salient (the reference `continue`s past the store of its third
//     eigenvalue and later reads uninitialised memory for it)
//   * boundary estimation (border_radius > 0, normal_radius) is not built
//   * the index covers the whole unscaled cloud; non-finite records are never keypoints and never neighbours
//   * the eigenvalues come from the Jacobi iteration below and the sums run in traversal order (the reference: Eigen's QR
//     iteration, ascending distance)
#pragma once

#include "device_scan.hpp"
#include "outlier.hpp"  // OR_BLOCK, OR_WAVES, outlier_grid, or_blocks
#include "traverse.hpp"

namespace pclhip {
namespace {

// Pass 1: the neighbour count and the six sums of the scatter matrix
struct IssScatter {
  float t;
  double px, py, pz;
  uint32_t cnt, n;
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
      cxx = fma(dx, dx, cxx);
      cxy = fma(dx, dy, cxy);
      cxz = fma(dx, dz, cxz);
      cyy = fma(dy, dy, cyy);
      cyz = fma(dy, dz, cyz);
      czz = fma(dz, dz, czz);
    }
  }
};

// one Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix; r is the third index
__device__ __forceinline__ void iss_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  // (theta * theta may overflow: t = 0 then, apq is below anything the diagonal can feel)
  const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
  const double c = 1.0 / sqrt(fma(tt, tt, 1.0)), sn = tt * c;
  app = fma(-tt, apq, app);
  aqq = fma(tt, apq, aqq);
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - sn * rq;
  arq = sn * rp + c * rq;
}

// eigenvalues of the symmetric matrix (a00 a01 a02; . a11 a12; . . a22), descending.  Cyclic Jacobi, the three rotations
// written out on named scalars (run-time-indexed 3 x 3 arrays are moved to LDS or scratch by the compiler:
// ndt_cells.hpp).  The sweeps end when the off-diagonal part is below 1e-20 of the diagonal's magnitude: what is left
// moves an eigenvalue by less than that (Weyl), far inside one rounding of the sums.
__device__ __forceinline__ void iss_eigenvalues(double a00, double a01, double a02, double a11, double a12, double a22,
                                                double& e1, double& e2, double& e3) {
#pragma unroll 1
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = fabs(a01) + fabs(a02) + fabs(a12);
    const double dia = fabs(a00) + fabs(a11) + fabs(a22);
    if (!(off > 1e-20 * dia)) break;  // (a NaN ends the loop as well)
    iss_rotate(a00, a11, a01, a02, a12);
    iss_rotate(a00, a22, a02, a01, a12);
    iss_rotate(a11, a22, a12, a01, a02);
  }
  double x = a00, y = a11, z = a22, w;
  if (x < y) { w = x; x = y; y = w; }
  if (y < z) { w = y; y = z; z = w; }
  if (x < y) { w = x; x = y; y = w; }
  e1 = x;
  e2 = y;
  e3 = z;
}

// waves per SIMD (kernel-resource-usage, gfx950): see DESIGN.md row f-12
__global__ __launch_bounds__(OR_BLOCK) void iss_scatter_kernel(IndexView ix, float t, uint32_t min_nb, double g21, double g32,
                                                               double* __restrict__ sal, double* __restrict__ eig) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, nullptr, ix.n, [&](uint32_t pos, bool real, float4 p) {
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {real};
    IssScatter pol;
    pol.t = t;
    pol.n = ix.n;
    pol.px = double(p.x); pol.py = double(p.y); pol.pz = double(p.z);
    pol.cnt = 0;
    pol.cxx = pol.cxy = pol.cxz = pol.cyy = pol.cyz = pol.czz = 0.0;
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a point
    traverse<IssScatter, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (!real) return;
    double e1 = 0.0, e2 = 0.0, e3 = 0.0, s = 0.0;
    if (pol.cnt >= min_nb) {
      iss_eigenvalues(pol.cxx, pol.cxy, pol.cxz, pol.cyy, pol.cyz, pol.czz, e1, e2, e3);
      const bool ok = isfinite(e1) && isfinite(e2) && isfinite(e3) && e3 >= 0.0;
      if (ok && e2 / e1 < g21 && e3 / e2 < g32) s = e3;
    }
    sal[pos] = s;
    if (eig != nullptr) {
      eig[size_t(pos) * 3] = e1;
      eig[size_t(pos) * 3 + 1] = e2;
      eig[size_t(pos) * 3 + 2] = e3;
    }
  });
}

// Pass 2: is the lane's saliency the largest of its non-max neighbourhood, and does that hold enough points
struct IssNms {
  float t;
  double si;
  uint32_t cnt, n;
  bool bigger;
  const double* sal;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return bigger ? -1.0f : t; }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id == NO_INDEX || bigger) return;
    const float4* s = reinterpret_cast<const float4*>(buf) + slot;
    uint32_t mask = leaf_hits_lt<16>(s, qx[0], qy[0], qz[0], t);
    const uint32_t base = leaf_id * uint32_t(LEAF);
    if (n - base < uint32_t(LEAF)) mask &= (1u << (n - base)) - 1u;
    cnt += uint32_t(__builtin_popcount(mask));
    while (mask != 0) {
      const uint32_t j = uint32_t(__builtin_ctz(mask));
      mask &= mask - 1u;
      if (si < sal[base + j]) bigger = true;
    }
  }
};

__global__ __launch_bounds__(OR_BLOCK) void iss_nms_kernel(IndexView ix, float t, uint32_t min_nb,
                                                           const double* __restrict__ sal, uint32_t* __restrict__ flag) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, nullptr, ix.n, [&](uint32_t pos, bool real, float4 p) {
    IssNms pol;
    pol.t = t;
    pol.n = ix.n;
    pol.sal = sal;
    pol.si = real ? sal[pos] : 0.0;
    pol.cnt = 0;
    pol.bigger = false;
    const bool salient = real && pol.si > 0.0;
    if (__builtin_amdgcn_ballot_w64(salient) == 0) return;  // the flags were cleared before the launch
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {salient};
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a point
    traverse<IssNms, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (salient && !pol.bigger && pol.cnt >= min_nb) flag[__float_as_uint(p.w)] = 1u;
  });
}

// ids i with flag[i] != 0, ascending (excl: exclusive scan of flag); what does not fit the caller's capacity is dropped
__global__ __launch_bounds__(OR_BLOCK) void iss_emit_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl,
                                                            uint64_t n_orig, int32_t* __restrict__ out, uint64_t capacity) {
  const uint64_t i = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  if (i < n_orig && flag[i] != 0u && uint64_t(excl[i]) < capacity) out[excl[i]] = int32_t(i);
}

// saliency and eigenvalues of record i: 0 / NaN for a record the index dropped
__global__ __launch_bounds__(OR_BLOCK) void iss_gather_kernel(const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                              const double* __restrict__ sal, const double* __restrict__ eig,
                                                              double* __restrict__ out_sal, double* __restrict__ out_eig) {
  const uint64_t i = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  if (i >= n_orig) return;
  const uint32_t pos = rank[i];
  if (out_sal != nullptr) out_sal[i] = pos != NO_INDEX ? sal[pos] : 0.0;
  if (out_eig != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_eig[i * 3 + k] = pos != NO_INDEX ? eig[size_t(pos) * 3 + k] : __builtin_nan("");
  }
}

}  // namespace

// The host side of pclhip_iss_keypoints (api.hip): t_sal and t_nms are the float squares of the two radii.
pclhip_status iss_keypoints(pclhip_index* ix, float t_sal, float t_nms, double g21, double g32, uint32_t min_nb,
                            int32_t* out_indices, uint64_t capacity, uint64_t* n_keypoints, double* out_saliency,
                            double* out_eigenvalues) {
  pclhip_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const uint64_t n_orig = ix->n_orig;
  const uint32_t n = ix->n;
  *n_keypoints = 0;
  if (n_orig == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  DeviceScope scope(ctx);
  uint32_t *tot = nullptr, *flag = nullptr, *excl = nullptr;
  uint2* part = nullptr;
  double *sal = nullptr, *eig = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&tot, 16));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&flag, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&excl, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((n_orig + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&sal, size_t(n > 0 ? n : 1) * 8));
  if (out_eigenvalues != nullptr) PCLHIP_CHECK_HIP(ctx, scope.alloc(&eig, size_t(n > 0 ? n : 1) * 24));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(tot, 0, 16, s));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(flag, 0, size_t(n_orig) * 4, s));
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.event(&e0));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e1));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e2));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e3));
  const IndexView v = ix->view();
  (void)hipEventRecord(e0, s);
  if (n > 0) {
    if (t_sal > 0.0f) {
      PCLHIP_LAUNCH_FED(ctx, iss_scatter_kernel, dim3(outlier_grid(ctx, iss_scatter_kernel, n)), dim3(OR_BLOCK), 0, s, v, t_sal,
                        min_nb, g21, g32, sal, eig);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    } else {  // nothing lies within d2 < 0: m = 0 < min_neighbors everywhere
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(sal, 0, size_t(n) * 8, s));
      if (eig != nullptr) PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(eig, 0, size_t(n) * 24, s));
    }
  }
  (void)hipEventRecord(e1, s);
  if (n > 0 && t_sal > 0.0f && t_nms > 0.0f) {
    PCLHIP_LAUNCH_FED(ctx, iss_nms_kernel, dim3(outlier_grid(ctx, iss_nms_kernel, n)), dim3(OR_BLOCK), 0, s, v, t_nms, min_nb,
                      sal, flag);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  (void)hipEventRecord(e2, s);
  launch_scan_u32(s, flag, n_orig, part, tot, excl);
  const uint64_t cap = capacity < n_orig ? capacity : n_orig;
  const bool out_dev = out_indices != nullptr && is_device_pointer(out_indices);
  int32_t* d_out = out_indices;
  if (cap > 0 && !out_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_out, size_t(cap) * 4));
  if (cap > 0) {
    hipLaunchKernelGGL(iss_emit_kernel, or_blocks(n_orig), dim3(OR_BLOCK), 0, s, flag, excl, n_orig, d_out, cap);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  const bool sal_dev = out_saliency != nullptr && is_device_pointer(out_saliency);
  const bool eig_dev = out_eigenvalues != nullptr && is_device_pointer(out_eigenvalues);
  double *d_sal = out_saliency, *d_eig = out_eigenvalues;
  if (out_saliency != nullptr && !sal_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_sal, size_t(n_orig) * 8));
  if (out_eigenvalues != nullptr && !eig_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_eig, size_t(n_orig) * 24));
  if (out_saliency != nullptr || out_eigenvalues != nullptr) {
    hipLaunchKernelGGL(iss_gather_kernel, or_blocks(n_orig), dim3(OR_BLOCK), 0, s, ix->rank, n_orig, sal, eig, d_sal, d_eig);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  (void)hipEventRecord(e3, s);
  uint32_t h[4] = {0, 0, 0, 0};
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(h, tot, 16, hipMemcpyDeviceToHost, s));  // the count: the call's one read-back
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  const uint64_t count = h[0];
  const uint64_t fit = count < cap ? count : cap;
  if (fit > 0 && !out_dev) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_indices, d_out, size_t(fit) * 4, hipMemcpyDeviceToHost, s));
  if (out_saliency != nullptr && !sal_dev)
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_saliency, d_sal, size_t(n_orig) * 8, hipMemcpyDeviceToHost, s));
  if (out_eigenvalues != nullptr && !eig_dev)
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_eigenvalues, d_eig, size_t(n_orig) * 24, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, e0, e3) == hipSuccess) ix->last_kernel_ms = ms;
  if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ix->iss_pass_ms[0] = ms;
  if (hipEventElapsedTime(&ms, e1, e2) == hipSuccess) ix->iss_pass_ms[1] = ms;
  *n_keypoints = count;
  if (count > capacity) {
    set_error(ctx, "iss: more keypoints than the capacity of out_indices");
    return PCLHIP_ERR_OVERFLOW;
  }
  return PCLHIP_OK;
}

}  // namespace pclhip
