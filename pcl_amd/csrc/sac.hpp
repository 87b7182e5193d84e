// sac.hpp -- SACSegmentation for SACMODEL_PLANE under SAC_RANSAC (segmentation/include/pcl/segmentation/impl/
// sac_segmentation.hpp:79-133, sample_consensus/.../impl/ransac.hpp:56-217, impl/sac_model_plane.hpp:80-118,153-230,311-360;
// the semantics are stated in include/pclhip.h).  Included by radius.hip.
//
// Per call, stream-ordered:
//   sac_gather_kernel       the point set once, as contiguous float4 records (x, y, z, position bits)
// then batches of B trials; per batch:
//   sac_hypothesis_kernel   one thread per trial: the draws (scp_draw.hpp), the plane of the three samples in the reference's
//                           float order, the skip flag; trace record, coefficients (d = NaN for a skipped trial)
//   sac_count_kernel        the hot path: points x hypotheses.  A lane keeps SAC_P points in registers (packed pairs), the
//                           wave walks the batch's hypotheses -- their coefficients are wave-uniform reads of a const array
//                           (scalar loads) -- and per (hypothesis, point slot) one compare gives a ballot whose popcount goes
//                           to a wave-uniform counter.  Lane h % 64 keeps the wave's count of hypothesis h; every 64
//                           hypotheses the lanes add theirs to the block's LDS counters, and the block adds those to count[h]
//                           once, after its last tile.  Integer adds: the order never shows.  A skipped trial is not scored.
//                           Every point is read once per batch.
//   one read-back           the batch's trace records and counts; sac::Replay (sac_replay.hpp) consumes them in trial order
// After the replay: sac_flag_kernel with the winner's coefficients (from device memory), scan + stable compaction
// (device_scan.hpp) -> the inlier list; with optimize_coefficients sac_moments_kernel (the nine double sums over the inlier
// list in block_sums.hpp's fixed order), block_sums_finalize_kernel, sac_refit_kernel (one thread: covariance in double
// rounded once to float, normals_math.hpp's eigen33 path), then flags, scan and compaction again; the complement list from
// the same flags.  ONE more read-back: the coefficients and the list lengths.
// The host side of the call is sac_segment_run in sac_models.hpp, shared with the constrained and the normal plane models.
#pragma once

#include <cfloat>
#include <cmath>
#include <vector>

#include "block_sums.hpp"
#include "device_scan.hpp"
#include "normals_math.hpp"
#include "sac_replay.hpp"
#include "scp_draw.hpp"
#include "traverse.hpp"

namespace pclhip {
namespace {

constexpr int SAC_BLOCK = 256;
constexpr int SAC_WAVES = SAC_BLOCK / WAVE;
constexpr int SAC_P = 12;                         // points a lane keeps in registers (measured: 8 -> 1.71 ms, 12 -> 1.52, 16 -> 1.53)
constexpr int SAC_TILE = SAC_BLOCK * SAC_P;       // points a block scores per step
constexpr int SAC_MAX_BATCH = 1024;               // hypotheses of a pass (the block's LDS counters)
constexpr int SAC_AUTO_BATCH = 64;                // first batch of a call that names none; doubles up to SAC_MAX_BATCH
constexpr int SAC_MOMENT_BLOCKS = 1024;           // rows of the refit's sums at most (a function of the list length only)
constexpr uint64_t SAC_TRACE_MAX = 65536;

struct SacDev {         // device-resident results of a call
  float coef[4];        // the winner's coefficients, then the refined ones
  uint32_t tot[4];      // scan totals of the flags: tot[0] = inliers
  uint32_t bad_index;   // an entry of `indices` outside the cloud
  uint32_t refined;
  uint32_t invalid;     // the coefficients fail their model's gate (sac_models.hpp): the selection is empty
  uint32_t pad;
};

inline dim3 sac_blocks_of(uint64_t n) { return dim3(uint32_t((n + SAC_BLOCK - 1) / SAC_BLOCK)); }

__global__ __launch_bounds__(SAC_BLOCK) void sac_gather_kernel(const char* __restrict__ rec, size_t stride, uint64_t n_rec,
                                                               const int32_t* __restrict__ idx, uint32_t n,
                                                               float4* __restrict__ out, SacDev* __restrict__ st) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t r = idx ? int64_t(idx[i]) : int64_t(i);
  float4 v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __uint_as_float(i));
  if (r >= 0 && uint64_t(r) < n_rec) {
    const float* p = reinterpret_cast<const float*>(rec + size_t(r) * stride);
    v.x = p[0]; v.y = p[1]; v.z = p[2];
  } else {
    st->bad_index = 1u;  // (every writer stores the same value)
  }
  out[i] = v;
}

// computeModelCoefficients (impl/sac_model_plane.hpp:93-113) for trial it0 + t
__global__ __launch_bounds__(SAC_BLOCK) void sac_hypothesis_kernel(uint64_t seed, uint32_t it0, uint32_t nit, uint32_t n,
                                                                   const float4* __restrict__ pts,
                                                                   pclhip_sac_plane_trace* __restrict__ rec,
                                                                   float4* __restrict__ models) {
  const uint32_t t = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (t >= nit) return;
  int s[scp::MAX_SAMPLES];
  scp::select_samples(seed, it0 + t, 3, int(n), s);
  const float4 p0 = pts[s[0]], p1 = pts[s[1]], p2 = pts[s[2]];
  const float ux = __fsub_rn(p1.x, p0.x), uy = __fsub_rn(p1.y, p0.y), uz = __fsub_rn(p1.z, p0.z);
  const float vx = __fsub_rn(p2.x, p0.x), vy = __fsub_rn(p2.y, p0.y), vz = __fsub_rn(p2.z, p0.z);
  const float cx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
  const float cy = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
  const float cz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
  const float norm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz)));
  const bool skip = norm < 1e-5f;  // Eigen's dummy_precision<float>; false for a NaN
  const float a = __fdiv_rn(cx, norm), b = __fdiv_rn(cy, norm), c = __fdiv_rn(cz, norm);
  const float d = -__fadd_rn(__fadd_rn(__fmul_rn(a, p0.x), __fmul_rn(b, p0.y)), __fmul_rn(c, p0.z));
  models[t] = make_float4(a, b, c, skip ? __builtin_nanf("") : d);  // (sac_count_kernel passes over a d that is not finite)
  pclhip_sac_plane_trace& r = rec[t];
  r.samples[0] = s[0]; r.samples[1] = s[1]; r.samples[2] = s[2];
  r.skipped = skip ? 1 : 0;
  r.coefficients[0] = a; r.coefficients[1] = b; r.coefficients[2] = c; r.coefficients[3] = d;
  r.count = 0u;
}

// countWithinDistance of H models at once.  counts[] is zero before the launch.
__global__ __launch_bounds__(SAC_BLOCK) void sac_count_kernel(const float4* __restrict__ pts, uint32_t n,
                                                              const float4* __restrict__ models, uint32_t H, float thr,
                                                              uint32_t* __restrict__ counts) {
  __shared__ uint32_t cnt_s[SAC_MAX_BATCH];
  for (uint32_t h = threadIdx.x; h < H; h += SAC_BLOCK) cnt_s[h] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint32_t tiles = (n + SAC_TILE - 1) / SAC_TILE;
  const float nan = __builtin_nanf("");
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // the wave's SAC_P * 64 points: slot k of lane l is point base + k * 64 + l (coalesced); past the end: NaN, never inside
    const uint32_t base = tile * uint32_t(SAC_TILE) + wave * uint32_t(SAC_P * WAVE) + lane;
    v2f px[SAC_P / 2], py[SAC_P / 2], pz[SAC_P / 2];
#pragma unroll
    for (int k = 0; k < SAC_P / 2; ++k) {
      const uint32_t i0 = base + uint32_t(2 * k) * WAVE, i1 = i0 + WAVE;
      float4 q0 = make_float4(nan, nan, nan, 0.0f), q1 = q0;
      if (i0 < n) q0 = pts[i0];
      if (i1 < n) q1 = pts[i1];
      px[k] = v2f{q0.x, q1.x};
      py[k] = v2f{q0.y, q1.y};
      pz[k] = v2f{q0.z, q1.z};
    }
    for (uint32_t h0 = 0; h0 < H; h0 += WAVE) {
      const uint32_t hn = H - h0 < uint32_t(WAVE) ? H - h0 : uint32_t(WAVE);
      uint32_t mine = 0u;  // lane j: the wave's count of hypothesis h0 + j
      float4 next = models[h0];  // (h is the same for the wave: scalar loads, one hypothesis ahead)
      for (uint32_t j = 0; j < hn; ++j) {
        const float4 m = next;
        next = models[h0 + (j + 1 < hn ? j + 1 : j)];
        // a skipped trial carries d = NaN and is not scored; any d that is not finite counts 0 whatever the points are
        if (!(__builtin_fabsf(m.w) <= FLT_MAX)) continue;
        const v2f a = {m.x, m.x}, b = {m.y, m.y}, c = {m.z, m.z}, d = {m.w, m.w};
        uint32_t cw = 0u;
#pragma unroll
        for (int k = 0; k < SAC_P / 2; ++k) {
          const v2f e = (a * px[k] + b * py[k]) + (c * pz[k] + d);  // (-ffp-contract=off: no fused multiply-add)
          cw += uint32_t(__popcll(__builtin_amdgcn_ballot_w64(__builtin_fabsf(e.x) < thr)));
          cw += uint32_t(__popcll(__builtin_amdgcn_ballot_w64(__builtin_fabsf(e.y) < thr)));
        }
        mine += lane == j ? cw : 0u;
      }
      if (mine != 0u) atomicAdd(&cnt_s[h0 + lane], mine);
    }
  }
  __syncthreads();
  for (uint32_t h = threadIdx.x; h < H; h += SAC_BLOCK) {
    const uint32_t v = cnt_s[h];
    if (v != 0u) atomicAdd(&counts[h], v);
  }
}

// selectWithinDistance as flags by position, with the coefficients the device holds
__global__ __launch_bounds__(SAC_BLOCK) void sac_flag_kernel(const float4* __restrict__ pts, uint32_t n,
                                                             const SacDev* __restrict__ st, float thr,
                                                             uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float a = st->coef[0], b = st->coef[1], c = st->coef[2], d = st->coef[3];
  const float4 p = pts[i];
  const float e = __fadd_rn(__fadd_rn(__fmul_rn(a, p.x), __fmul_rn(b, p.y)), __fadd_rn(__fmul_rn(c, p.z), d));
  flag[i] = st->invalid == 0u && __builtin_fabsf(e) < thr ? 1u : 0u;
}

// the two lists from one set of flags, in the order of the point set: cloud indices of the inliers and of the rest
__global__ __launch_bounds__(SAC_BLOCK) void sac_lists_kernel(const uint32_t* __restrict__ flag,
                                                              const uint32_t* __restrict__ excl, uint32_t n,
                                                              const int32_t* __restrict__ idx, int32_t* __restrict__ inl,
                                                              int32_t* __restrict__ outl) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t id = idx ? idx[i] : int32_t(i);
  const uint32_t before = excl[i];
  if (flag[i] != 0u) {
    inl[before] = id;
  } else if (outl != nullptr) {
    outl[i - before] = id;
  }
}

// computeMeanAndCovarianceMatrix (common/include/pcl/common/impl/centroid.hpp:581-650) over the inlier list, shifted by
// its first point: xx xy xz yy yz zz x y z, in double.  Thread g of the grid adds entries g, g + threads, ... in order.
__global__ __launch_bounds__(SAC_BLOCK) void sac_moments_kernel(const float4* __restrict__ pts,
                                                                const uint32_t* __restrict__ pos_list, uint32_t m,
                                                                double* __restrict__ partials) {
  double acc[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] = 0.0;
  const float4 k4 = pts[pos_list[0]];
  const double kx = double(k4.x), ky = double(k4.y), kz = double(k4.z);
  const uint32_t threads = gridDim.x * SAC_BLOCK;
  for (uint32_t e = blockIdx.x * SAC_BLOCK + threadIdx.x; e < m; e += threads) {
    const float4 p = pts[pos_list[e]];
    const double x = double(p.x) - kx, y = double(p.y) - ky, z = double(p.z) - kz;
    acc[0] += x * x; acc[1] += x * y; acc[2] += x * z;
    acc[3] += y * y; acc[4] += y * z; acc[5] += z * z;
    acc[6] += x; acc[7] += y; acc[8] += z;
  }
  block_rows<9, SAC_WAVES, 9>(acc, partials);
}

// positions of the inliers, in order (the refit walks them)
__global__ __launch_bounds__(SAC_BLOCK) void sac_positions_kernel(const uint32_t* __restrict__ flag,
                                                                  const uint32_t* __restrict__ excl, uint32_t n,
                                                                  uint32_t* __restrict__ pos_list, uint32_t m) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i < n && flag[i] != 0u && excl[i] < m) pos_list[excl[i]] = i;
}

// optimizeModelCoefficients (impl/sac_model_plane.hpp:331-359) from the nine sums: one thread
__global__ void sac_refit_kernel(const double* __restrict__ sums, const float4* __restrict__ pts,
                                 const uint32_t* __restrict__ pos_list, uint32_t m, SacDev* __restrict__ st) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const float4 k4 = pts[pos_list[0]];
  double a[9];
  for (int i = 0; i < 9; ++i) a[i] = sums[i] / double(m);
  const double cd[6] = {a[0] - a[6] * a[6], a[1] - a[6] * a[7], a[2] - a[6] * a[8],
                        a[3] - a[7] * a[7], a[4] - a[7] * a[8], a[5] - a[8] * a[8]};
  float cov[9];
  cov[0] = float(cd[0]); cov[1] = float(cd[1]); cov[2] = float(cd[2]);
  cov[4] = float(cd[3]); cov[5] = float(cd[4]); cov[8] = float(cd[5]);
  cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
  const float cx = float(a[6] + double(k4.x)), cy = float(a[7] + double(k4.y)), cz = float(a[8] + double(k4.z));
  float nx, ny, nz, curv;
  solve_plane(cov, nx, ny, nz, curv);
  const float d = -__fadd_rn(__fadd_rn(__fmul_rn(nx, cx), __fmul_rn(ny, cy)), __fmul_rn(nz, cz));
  if (isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(d)) {
    st->coef[0] = nx; st->coef[1] = ny; st->coef[2] = nz; st->coef[3] = d;
    st->refined = 1u;
  }
}

// the point set of a call on the device
struct SacCloud {
  float4* pts = nullptr;
  const int32_t* idx = nullptr;  // device copy of `indices` (null: every record)
  uint32_t n = 0;
};

pclhip_status sac_stage(pclhip_ctx* ctx, DeviceScope& scope, const void* cloud, uint64_t n_rec, size_t stride,
                        const int32_t* indices, uint64_t n_indices, SacDev* st, SacCloud* out) {
  hipStream_t s = ctx->stream;
  const uint64_t n = indices ? n_indices : n_rec;
  out->n = uint32_t(n);
  if (n == 0) return PCLHIP_OK;
  const void* dcloud = nullptr;
  void* owned = nullptr;
  pclhip_status rc = to_device(ctx, cloud, size_t(n_rec) * stride, &dcloud, &owned);
  if (rc != PCLHIP_OK) return rc;
  if (owned) scope.mem.push_back(owned);
  if (indices) {
    const void* didx = nullptr;
    rc = to_device(ctx, indices, size_t(n_indices) * sizeof(int32_t), &didx, &owned);
    if (rc != PCLHIP_OK) return rc;
    if (owned) scope.mem.push_back(owned);
    out->idx = static_cast<const int32_t*>(didx);
  }
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&out->pts, size_t(n) * sizeof(float4)));
  hipLaunchKernelGGL(sac_gather_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, static_cast<const char*>(dcloud), stride, n_rec,
                     out->idx, uint32_t(n), out->pts, st);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  return PCLHIP_OK;
}

// grid of the scoring pass: by occupancy, no more blocks than tiles
uint32_t sac_count_grid(const pclhip_ctx* ctx, uint32_t n) {
  static int per_cu = 0;
  if (per_cu == 0) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, sac_count_kernel, SAC_BLOCK, 0) != hipSuccess || v < 1) {
      (void)hipGetLastError();
      v = 4;
    }
    per_cu = v;
  }
  const uint64_t tiles = (uint64_t(n) + SAC_TILE - 1) / SAC_TILE;
  const uint64_t most = uint64_t(per_cu) * uint64_t(ctx->num_cus > 0 ? ctx->num_cus : 1);
  return uint32_t(tiles < most ? (tiles > 0 ? tiles : 1) : most);
}

pclhip_status sac_checked_params(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const int32_t* indices,
                                 uint64_t n_indices) {
  PCLHIP_REQUIRE(ctx, stride >= 12 && stride % 4 == 0, "stride must be a multiple of 4 and >= 12 bytes");
  PCLHIP_REQUIRE(ctx, n_rec < 0x7FFFFFFFull && n_indices < 0x7FFFFFFFull, "cloud too large for int32 indices");
  PCLHIP_REQUIRE(ctx, cloud != nullptr || n_rec == 0, "null cloud");
  PCLHIP_REQUIRE(ctx, indices == nullptr || n_rec > 0 || n_indices == 0, "indices into an empty cloud");
  return PCLHIP_OK;
}

// n entries of a device list to a host or device buffer
pclhip_status sac_copy_out(pclhip_ctx* ctx, int32_t* out, const int32_t* dev, uint64_t n) {
  if (out == nullptr || n == 0 || out == dev) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out, dev, size_t(n) * 4, hipMemcpyDefault, ctx->stream));
  return PCLHIP_OK;
}

// the call, for the plane and for the models of sac_models.hpp (defined there: radius.hip includes it after this file)
pclhip_status sac_segment_run(pclhip_ctx* ctx, const char* fn, const void* cloud, uint64_t n_rec, size_t stride,
                              const void* normals, size_t nstride, const int32_t* indices, uint64_t n_indices,
                              const pclhip_sac_plane_params* P, const pclhip_sac_model_params* MP, float out_coeff[4],
                              int32_t* out_inliers, uint64_t inliers_capacity, uint64_t* out_n_inliers, int32_t* out_outliers,
                              uint64_t outliers_capacity, uint64_t* out_n_outliers, pclhip_sac_plane_stats* out_stats);

}  // namespace
}  // namespace pclhip

extern "C" {

void pclhip_sac_plane_params_default(pclhip_sac_plane_params* p) {
  if (!p) return;
  // sac_segmentation.h:83-98
  p->distance_threshold = 0.0;
  p->max_iterations = 50;
  p->probability = 0.99;
  p->optimize_coefficients = 1;
  p->seed = 0;
  p->batch_size = 0;
}

pclhip_status pclhip_sac_plane_evaluate(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride,
                                        const int32_t* indices, uint64_t n_indices, double threshold, const float* coeffs,
                                        int n_models, uint32_t* out_counts) {
  using namespace pclhip;
  if (!ctx || n_models < 0 || (n_models > 0 && (!coeffs || !out_counts))) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  pclhip_status rc = sac_checked_params(ctx, cloud, n_rec, stride, indices, n_indices);
  if (rc != PCLHIP_OK) return rc;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DeviceScope scope(ctx);
  SacDev* st = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&st, sizeof(SacDev)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(st, 0, sizeof(SacDev), s));
  SacCloud pc;
  if ((rc = sac_stage(ctx, scope, cloud, n_rec, stride, indices, n_indices, st, &pc)) != PCLHIP_OK) return rc;
  for (int m = 0; m < n_models; ++m) out_counts[m] = 0u;
  if (pc.n == 0 || n_models == 0) return PCLHIP_OK;
  SacDev h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  PCLHIP_REQUIRE(ctx, h.bad_index == 0u, "an entry of indices lies outside the cloud");
  float4* models = nullptr;
  uint32_t* counts = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&models, size_t(SAC_MAX_BATCH) * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&counts, size_t(SAC_MAX_BATCH) * 4));
  const float thr = float(threshold);
  const uint32_t grid = sac_count_grid(ctx, pc.n);
  for (int m0 = 0; m0 < n_models; m0 += SAC_MAX_BATCH) {
    const uint32_t H = uint32_t(n_models - m0 < SAC_MAX_BATCH ? n_models - m0 : SAC_MAX_BATCH);
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(models, coeffs + size_t(m0) * 4, size_t(H) * sizeof(float4), hipMemcpyHostToDevice, s));
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, size_t(H) * 4, s));
    hipLaunchKernelGGL(sac_count_kernel, dim3(grid), dim3(SAC_BLOCK), 0, s, pc.pts, pc.n, models, H, thr, counts);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_counts + m0, counts, size_t(H) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  }
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_segment_plane(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride,
                                       const int32_t* indices, uint64_t n_indices, const pclhip_sac_plane_params* P,
                                       float out_coeff[4], int32_t* out_inliers, uint64_t inliers_capacity,
                                       uint64_t* out_n_inliers, int32_t* out_outliers, uint64_t outliers_capacity,
                                       uint64_t* out_n_outliers, pclhip_sac_plane_stats* out_stats) {
  return pclhip::sac_segment_run(ctx, "pclhip_sac_segment_plane", cloud, n_rec, stride, nullptr, 0, indices, n_indices, P, nullptr,
                                 out_coeff, out_inliers, inliers_capacity, out_n_inliers, out_outliers, outliers_capacity,
                                 out_n_outliers, out_stats);
}

pclhip_status pclhip_sac_last_trace(pclhip_ctx* ctx, pclhip_sac_plane_trace* buf, uint64_t capacity, uint64_t* count) {
  if (!ctx || !count || (capacity > 0 && !buf)) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *count = ctx->sac_trace.size();
  const uint64_t m = capacity < *count ? capacity : *count;
  if (m > 0) std::memcpy(buf, ctx->sac_trace.data(), size_t(m) * sizeof(pclhip_sac_plane_trace));
  return PCLHIP_OK;
}

}  // extern "C"
