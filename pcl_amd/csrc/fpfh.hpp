// fpfh.hpp -- FPFHEstimation with setRadiusSearch over the index (included by radius.hip).
// Replaces pcl::FPFHEstimation<PointInT, PointNT, PointOutT>::computeFeature (features/include/pcl/features/impl/fpfh.hpp
// :51-303) with pcl::computePairFeatures (features/src/pfh.cpp:45-103): the search surface is the input, the
// neighbourhood every indexed point with float d2 < float(r * r), 11 / 11 / 11 bins.  A positive r whose float square
// is 0 gives every point an EMPTY neighbourhood (d2 < 0 never holds, not even for the point itself): the reference then
// leaves the SPFH row at zero (fpfh.hpp:224-225) and writes a NaN FPFH row (:255-261), and so do the two kernels -- without
// a walk, the bound is the same for every point.
//
// Pipeline (one stream, one read-back at the end):
//   outlier_pos_kernel   (with indices only) entry -> sorted position, marked and compacted so the queries run in kd order
//   fpfh_spfh_kernel     per point: the pair features against every neighbour but itself, binned into three 11-bin
//                        COUNTERS (integers, in LDS: run-time indexed, one column per lane), then every bin = hist_incr
//                        added count times in float, as computePointSPFHSignature adds it: a value that does not depend on
//                        the order of the neighbours.  One 33-float row per point in kd order.
//   fpfh_weight_kernel   per query: sum over the neighbours with d2 != 0 of (1.0f / d2) * their SPFH row.  The products of
//                        two floats are exact in double and are summed in double in traversal order (the reference sums
//                        float products in float in ascending distance: the result sits inside that sum's own rounding),
//                        then every histogram is scaled by 100.0 / its sum in double (fpfh.hpp:161-177).  Rows in kd order.
//   fpfh_emit_kernel     rows -> the caller's records in query order; NaN for records the index dropped
// Both walks are traverse<Policy, true> (lane-sparse) with a fixed bound, the strict hit mask of traverse.hpp's leaf_hits_lt,
// inside traverse.hpp's one-lane-per-point group loop (for_each_query_group).  The lane's own leaf is NOT evaluated ahead of the
// walk as ror_count_kernel does: a fixed radius gains no bound from it, and the pair code would exist twice; the own leaf
// only names the node the walk starts under.
//
// Deviation (the reference casts a NaN feature to int there: undefined): a point whose own normal is not finite gets 33
// NaN in both outputs; a neighbour whose normal is not finite is skipped in both passes but still counts towards
// hist_incr = 100 / (neighbours - 1).
#pragma once

#include "device_scan.hpp"
#include "outlier.hpp"  // OR_BLOCK, OR_WAVES, outlier_grid, or_blocks, outlier_pos_kernel, outlier_compact_kernel
#include "traverse.hpp"

namespace pclhip {
namespace {

constexpr int FPFH_BINS = 11;
constexpr int FPFH_DIM = 3 * FPFH_BINS;
constexpr uint32_t FPFH_MAX_COUNT = 65535u;  // what a bin counter holds

__device__ __forceinline__ float fpfh_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// floor(11 * x) clamped to 0..10 (fpfh.hpp:91-103; a NaN lands in bin 0)
__device__ __forceinline__ int fpfh_bin(double x) {
  const double b = floor(double(FPFH_BINS) * x);
  return int(fmin(fmax(b, 0.0), double(FPFH_BINS - 1)));
}

// pcl::computePairFeatures in float, the operations in the order of tests/fpfh_restatement.py; a degenerate pair
// (distance 0 or d parallel to u) has f1 = f2 = f3 = 0 and is binned all the same (FPFHEstimation::computePairFeatures
// returns true)
__device__ __forceinline__ void fpfh_pair_bins(float px, float py, float pz, float n1x, float n1y, float n1z, float cx,
                                               float cy, float cz, float n2x, float n2y, float n2z, int& b1, int& b2,
                                               int& b3) {
  float dx = __fsub_rn(cx, px), dy = __fsub_rn(cy, py), dz = __fsub_rn(cz, pz);
  const float f4 = __fsqrt_rn(fpfh_dot(dx, dy, dz, dx, dy, dz));
  float f1 = 0.0f, f2 = 0.0f, f3 = 0.0f;
  if (f4 != 0.0f) {
    const float angle1 = __fdiv_rn(fpfh_dot(n1x, n1y, n1z, dx, dy, dz), f4);
    const float angle2 = __fdiv_rn(fpfh_dot(n2x, n2y, n2z, dx, dy, dz), f4);
    float ux = n1x, uy = n1y, uz = n1z, tx = n2x, ty = n2y, tz = n2z;
    if (acosf(fabsf(angle1)) > acosf(fabsf(angle2))) {  // the roles of the two points swap
      ux = n2x; uy = n2y; uz = n2z;
      tx = n1x; ty = n1y; tz = n1z;
      dx = -dx; dy = -dy; dz = -dz;
      f3 = -angle2;
    } else {
      f3 = angle1;
    }
    float vx = __fsub_rn(__fmul_rn(dy, uz), __fmul_rn(dz, uy));
    float vy = __fsub_rn(__fmul_rn(dz, ux), __fmul_rn(dx, uz));
    float vz = __fsub_rn(__fmul_rn(dx, uy), __fmul_rn(dy, ux));
    const float vn = __fsqrt_rn(fpfh_dot(vx, vy, vz, vx, vy, vz));
    if (vn != 0.0f) {
      vx = __fdiv_rn(vx, vn);
      vy = __fdiv_rn(vy, vn);
      vz = __fdiv_rn(vz, vn);
      const float wx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
      const float wy = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
      const float wz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
      f2 = fpfh_dot(vx, vy, vz, tx, ty, tz);
      f1 = atan2f(fpfh_dot(wx, wy, wz, tx, ty, tz), fpfh_dot(ux, uy, uz, tx, ty, tz));
    } else {
      f3 = 0.0f;
    }
  }
  const float d_pi = 1.0f / (2.0f * 3.14159274101257324f);  // fpfh.h:98, a float
  b1 = fpfh_bin((double(f1) + 3.14159265358979323846) * double(d_pi));
  b2 = fpfh_bin((double(f2) + 1.0) * 0.5);
  b3 = fpfh_bin((double(f3) + 1.0) * 0.5);
}

// Pass 1.  A lane walks the candidates of a leaf that passed d2 < t one after the other (its own hit mask: a round costs
// the largest number of hits among the lanes, not 16 pair evaluations).
struct FpfhSpfh {
  float t;
  float px, py, pz, nx, ny, nz;
  uint32_t self;       // the query's own position: the one neighbour that is not binned
  uint32_t cnt;        // neighbours, the point itself included
  uint16_t* col;       // this lane's column of the wave's counters: bin b at col[b * WAVE]
  const float4* nrm;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return t; }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id == NO_INDEX) return;
    const float4* s = reinterpret_cast<const float4*>(buf) + slot;  // transposed staging
    uint32_t mask = leaf_hits_lt<16>(s, qx[0], qy[0], qz[0], t);
    cnt += uint32_t(__builtin_popcount(mask));
    const uint32_t base = leaf_id * uint32_t(LEAF);
    if (base == (self & ~uint32_t(LEAF - 1))) mask &= ~(1u << (self & uint32_t(LEAF - 1)));
    while (mask != 0) {
      const uint32_t j = uint32_t(__builtin_ctz(mask));
      mask &= mask - 1u;
      const float4 n2 = nrm[base + j];
      if (!(isfinite(n2.x) && isfinite(n2.y) && isfinite(n2.z))) continue;
      int b1, b2, b3;
      fpfh_pair_bins(px, py, pz, nx, ny, nz, leaf_coord<16>(s, 0, j), leaf_coord<16>(s, 1, j), leaf_coord<16>(s, 2, j),
                     n2.x, n2.y, n2.z, b1, b2, b3);
      col[b1 * WAVE] += 1;
      col[(FPFH_BINS + b2) * WAVE] += 1;
      col[(2 * FPFH_BINS + b3) * WAVE] += 1;
    }
  }
};

// waves per SIMD (kernel-resource-usage, gfx950): see DESIGN.md row f-8
__global__ __launch_bounds__(OR_BLOCK) void fpfh_spfh_kernel(IndexView ix, float t, float* __restrict__ spfh,
                                                             uint32_t* __restrict__ overflow) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  __shared__ uint16_t hist_s[OR_WAVES][FPFH_DIM][WAVE];
  load_top_cache(ix, topbox_s);
  const int lane = threadIdx.x & (WAVE - 1);
  TraverseStats ts;
  FpfhSpfh pol;
  pol.t = t;
  pol.nrm = ix.nrm;
  pol.col = &hist_s[threadIdx.x / WAVE][0][lane];
  for_each_query_group(ix, nullptr, ix.n, [&](uint32_t pos, bool real, float4 p) {
    float4 nq = make_float4(0, 0, 0, 0);
    if (real) nq = ix.nrm[pos];
    const bool fin = real && isfinite(nq.x) && isfinite(nq.y) && isfinite(nq.z);
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {fin};
    pol.px = p.x; pol.py = p.y; pol.pz = p.z;
    pol.nx = nq.x; pol.ny = nq.y; pol.nz = nq.z;
    pol.self = pos;
    pol.cnt = 0;
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) pol.col[b * WAVE] = 0;
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a point
    if (t > 0.0f)  // (t == 0: nothing lies within d2 < 0, the counters stay at zero)
      traverse<FpfhSpfh, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (!real) return;
    float* row = spfh + size_t(pos) * FPFH_DIM;
    if (!fin) {
      for (int b = 0; b < FPFH_DIM; ++b) row[b] = __builtin_nanf("");
      return;
    }
    const uint32_t others = pol.cnt > 0u ? pol.cnt - 1u : 0u;  // (cnt == 0 only with t == 0: the point misses itself)
    if (others > FPFH_MAX_COUNT) *overflow = 1u;  // a bin may have wrapped: the call fails
    const float incr = __fdiv_rn(100.0f, float(others));  // fpfh.hpp:77 (inf for a lone point: never added)
    for (int b = 0; b < FPFH_DIM; ++b) {
      const uint32_t c = pol.col[b * WAVE];
      float v = 0.0f;
      for (uint32_t k = 0; k < c; ++k) v = __fadd_rn(v, incr);
      row[b] = v;
    }
  });
}

// Pass 2: acc[b] += double(row[b]) * double(1.0f / d2) over the neighbours with d2 != 0 (the point itself and its exact
// duplicates: fpfh.hpp:132) whose row is not NaN
struct FpfhWeight {
  float t;
  double acc[FPFH_DIM];
  const float* spfh;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return t; }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id == NO_INDEX) return;
    const float4* s = reinterpret_cast<const float4*>(buf) + slot;
    uint32_t mask = leaf_hits_lt<16>(s, qx[0], qy[0], qz[0], t);
    while (mask != 0) {
      const uint32_t j = uint32_t(__builtin_ctz(mask));
      mask &= mask - 1u;
      const float d2 = l2_simple(qx[0], qy[0], qz[0], leaf_coord<16>(s, 0, j), leaf_coord<16>(s, 1, j), leaf_coord<16>(s, 2, j));
      const float* row = spfh + (size_t(leaf_id) * LEAF + j) * FPFH_DIM;
      if (d2 == 0.0f || isnan(row[0])) continue;
      const double w = double(__fdiv_rn(1.0f, d2));
#pragma unroll
      for (int b = 0; b < FPFH_DIM; ++b) acc[b] = fma(double(row[b]), w, acc[b]);
    }
  }
};

__global__ __launch_bounds__(OR_BLOCK) void fpfh_weight_kernel(IndexView ix, const uint32_t* __restrict__ qpos, uint32_t nq,
                                                               float t, const float* __restrict__ spfh,
                                                               float* __restrict__ fpfh) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, qpos, nq, [&](uint32_t pos, bool real, float4 p) {
    FpfhWeight pol;
    pol.t = t;
    pol.spfh = spfh;
    const bool fin = real && !isnan(spfh[size_t(pos) * FPFH_DIM]);  // the point's own normal is finite
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {fin};
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) pol.acc[b] = 0.0;
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a query
    if (!(t > 0.0f)) {  // no neighbour, not even the query itself: the reference divides by the sum of no weights
      if (real)
        for (int b = 0; b < FPFH_DIM; ++b) fpfh[size_t(pos) * FPFH_DIM + b] = __builtin_nanf("");
      return;
    }
    traverse<FpfhWeight, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (!real) return;
    float* row = fpfh + size_t(pos) * FPFH_DIM;
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      double sum = 0.0;
#pragma unroll
      for (int b = 0; b < FPFH_BINS; ++b) sum += pol.acc[h * FPFH_BINS + b];
      const double f = sum != 0.0 ? 100.0 / sum : 0.0;  // histogram values sum up to 100
#pragma unroll
      for (int b = 0; b < FPFH_BINS; ++b) row[h * FPFH_BINS + b] = fin ? float(pol.acc[h * FPFH_BINS + b] * f) : __builtin_nanf("");
    }
  });
}

// value b of entry j <- row of record idx[j] (or j); NaN where the index holds no such point.  Rows whose first value is
// NaN are counted.
__global__ __launch_bounds__(OR_BLOCK) void fpfh_emit_kernel(const float* __restrict__ rows, const int32_t* __restrict__ idx,
                                                             uint64_t m, const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                             char* __restrict__ out, uint64_t stride,
                                                             unsigned long long* __restrict__ nan_count) {
  const uint64_t e = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  if (e >= m * FPFH_DIM) return;
  const uint64_t j = e / FPFH_DIM;
  const uint32_t b = uint32_t(e % FPFH_DIM);
  const int64_t id = idx ? int64_t(idx[j]) : int64_t(j);
  uint32_t pos = NO_INDEX;
  if (id >= 0 && uint64_t(id) < n_orig) pos = rank[id];
  const float v = pos != NO_INDEX ? rows[size_t(pos) * FPFH_DIM + b] : __builtin_nanf("");
  reinterpret_cast<float*>(out + j * stride)[b] = v;
  if (b == 0 && nan_count != nullptr && isnan(v)) atomicAdd(nan_count, 1ull);
}

inline dim3 fpfh_emit_blocks(uint64_t m) { return dim3(uint32_t((m * FPFH_DIM + OR_BLOCK - 1) / OR_BLOCK)); }

}  // namespace

// The host side of pclhip_fpfh (api.hip).
pclhip_status fpfh_compute(pclhip_index* ix, const int32_t* indices, uint64_t n_indices, double radius, void* out,
                           size_t out_stride, float* out_spfh, uint64_t* out_nan_count) {
  pclhip_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const uint64_t m64 = indices ? n_indices : ix->n_orig;
  PCLHIP_REQUIRE(ctx, m64 < 0x7FFFFFFFull, "too many queries");
  const uint32_t n = ix->n;
  if (out_nan_count) *out_nan_count = 0;
  if (m64 == 0 && (out_spfh == nullptr || ix->n_orig == 0)) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  DeviceScope scope(ctx);
  const uint32_t m = uint32_t(m64);
  const void* d_idx_v = nullptr;
  if (indices && m > 0) {
    void* owned = nullptr;
    const pclhip_status st = to_device(ctx, indices, size_t(m) * 4, &d_idx_v, &owned);
    if (st != PCLHIP_OK) return st;
    scope.mem.push_back(owned);
  }
  const int32_t* d_idx = static_cast<const int32_t*>(d_idx_v);
  struct ReadBack {
    unsigned long long nans;
    uint32_t tot_q[4];
    uint32_t bad;
    uint32_t overflow;
  };
  ReadBack* rb = nullptr;
  float *spfh = nullptr, *rows = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rb, sizeof(ReadBack)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&spfh, size_t(n) * FPFH_DIM * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rows, size_t(n) * FPFH_DIM * 4));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(rb, 0, sizeof(ReadBack), s));
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.event(&e0));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e1));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e2));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e3));
  (void)hipEventRecord(e0, s);
  uint32_t* qpos = nullptr;
  uint32_t nq = n;
  if (indices && m > 0) {
    // the positions asked for, ascending: the queries of the second pass stay in kd order
    uint32_t *epos = nullptr, *mark = nullptr, *qexcl = nullptr;
    uint2* part = nullptr;
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&epos, size_t(m) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&mark, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&qexcl, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&qpos, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((uint64_t(n) + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
    if (n > 0) PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(mark, 0, size_t(n) * 4, s));
    hipLaunchKernelGGL(outlier_pos_kernel, or_blocks(m), dim3(OR_BLOCK), 0, s, d_idx, m, ix->rank, ix->n_orig, epos,
                       n > 0 ? mark : nullptr, &rb->bad);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    if (n > 0) {
      launch_scan_u32(s, mark, n, part, rb->tot_q, qexcl);
      hipLaunchKernelGGL(outlier_compact_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, mark, qexcl, n, qpos);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    }
    ReadBack h;
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    PCLHIP_REQUIRE(ctx, h.bad == 0, "indices out of range");
    nq = h.tot_q[0];
  }
  const float t = float(radius * radius);  // kdtree_flann.hpp:398
  const IndexView v = ix->view();
  (void)hipEventRecord(e1, s);
  if (n > 0) {
    PCLHIP_LAUNCH_FED(ctx, fpfh_spfh_kernel, dim3(outlier_grid(ctx, fpfh_spfh_kernel, n)), dim3(OR_BLOCK), 0, s, v, t, spfh,
                      &rb->overflow);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  (void)hipEventRecord(e2, s);
  if (nq > 0 && m > 0) {
    PCLHIP_LAUNCH_FED(ctx, fpfh_weight_kernel, dim3(outlier_grid(ctx, fpfh_weight_kernel, nq)), dim3(OR_BLOCK), 0, s, v, qpos,
                      nq, t, spfh, rows);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  (void)hipEventRecord(e3, s);
  // rows -> the caller's records: straight into device memory, through a dense copy into host memory
  float *d_out = nullptr, *d_spfh = nullptr;
  const bool out_dev = out != nullptr && is_device_pointer(out);
  const bool spfh_dev = out_spfh != nullptr && is_device_pointer(out_spfh);
  if (m > 0) {
    char* dst = static_cast<char*>(out);
    uint64_t stride = out_stride;
    if (!out_dev) {
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_out, size_t(m) * FPFH_DIM * 4));
      dst = reinterpret_cast<char*>(d_out);
      stride = FPFH_DIM * 4;
    }
    hipLaunchKernelGGL(fpfh_emit_kernel, fpfh_emit_blocks(m), dim3(OR_BLOCK), 0, s, rows, d_idx, uint64_t(m), ix->rank,
                       ix->n_orig, dst, stride, &rb->nans);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  if (out_spfh != nullptr && ix->n_orig > 0) {
    char* dst = reinterpret_cast<char*>(out_spfh);
    if (!spfh_dev) {
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_spfh, size_t(ix->n_orig) * FPFH_DIM * 4));
      dst = reinterpret_cast<char*>(d_spfh);
    }
    hipLaunchKernelGGL(fpfh_emit_kernel, fpfh_emit_blocks(ix->n_orig), dim3(OR_BLOCK), 0, s, spfh, (const int32_t*)nullptr,
                       ix->n_orig, ix->rank, ix->n_orig, dst, uint64_t(FPFH_DIM * 4), (unsigned long long*)nullptr);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  hipEvent_t e4 = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.event(&e4));
  (void)hipEventRecord(e4, s);
  ReadBack h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  if (h.overflow != 0) {
    set_error(ctx, "fpfh: a neighbourhood holds more than 65536 points (a bin counter cannot hold it)");
    return PCLHIP_ERR_OVERFLOW;
  }
  if (m > 0 && !out_dev)
    PCLHIP_CHECK_HIP(ctx, hipMemcpy2DAsync(out, out_stride, d_out, FPFH_DIM * 4, FPFH_DIM * 4, m, hipMemcpyDeviceToHost, s));
  if (out_spfh != nullptr && ix->n_orig > 0 && !spfh_dev)
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_spfh, d_spfh, size_t(ix->n_orig) * FPFH_DIM * 4, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, e0, e4) == hipSuccess) ix->last_kernel_ms = ms;
  if (hipEventElapsedTime(&ms, e1, e2) == hipSuccess) ix->fpfh_pass_ms[0] = ms;
  if (hipEventElapsedTime(&ms, e2, e3) == hipSuccess) ix->fpfh_pass_ms[1] = ms;
  if (out_nan_count) *out_nan_count = h.nans;
  return PCLHIP_OK;
}

}  // namespace pclhip
