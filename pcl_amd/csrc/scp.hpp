// scp.hpp -- SampleConsensusPrerejective (registration/include/pcl/registration/sample_consensus_prerejective.h,
// impl/sample_consensus_prerejective.hpp:78-348, correspondence_rejection_poly.h:208-338).  Included by radius.hip: the
// scoring pass is a bounded 1-NN traversal of the target index.
//
// Ahead of the iterations, stream-ordered, nothing read back:
//   scp_mark_kernel          one thread per iteration of the WHOLE alignment (a draw is a function of the iteration, so
//                            the samples are known before the first batch): marks the source rows whose feature neighbours
//                            are not cached yet; scan + compaction (device_scan.hpp) -> their list
//   feature_knn_kernel<D,K>  exact brute-force k-NN over D-float rows for the listed rows, one launch: one query per lane,
//                            its row in registers, the target rows staged through a 64-row LDS tile that every lane reads
//                            by broadcast, a sorted top-k of (d2 bits, index) keys per lane.  FLANN's L2_Simple<float> in
//                            its order: the distance depends on the two rows only, never on the tiling.  A wave walks
//                            its target rows serially, so few queries would leave the device idle: the grid splits the
//                            target rows into up to 16 shares and feature_knn_merge_kernel merges the shares' sorted lists
//                            (the keys are totally ordered: the same result, bit for bit).
// Then the iterations in batches of B; per batch:
//   scp_hypothesis_kernel    one thread per iteration: draws, the pick among the k neighbours, the polygon test in the
//                            reference's float order, umeyama in double (scp_rotation); trace record,
//                            transform, survivor flag; scan + compaction -> the H surviving transforms in iteration order
//   scp_fitness_kernel       the hot path.  Work item = (hypothesis, 64 source points in the source's kd order): x' = T x
//                            fused (Transformer::se3 order), traverse<ScpNearest> with the bound float(corr_dist^2)
//                            (strict).  A group whose moved box is further than the bound from the top boxes ends at the
//                            root.  FIXED schedule: wave w of the grid takes items w, w + waves, ...; H is read from
//                            device memory.  Per item the inlier count (a ballot) and the wave tree of the double d2
//                            values go to ONE row, part[h * groups + g]: no atomics, one writer.
//   scp_finalize_kernel      one wave per hypothesis adds its rows in the order of block_sums_finalize_kernel (lane l rows
//                            l, l + 64, ..., then the butterfly): the sums depend on (source, target, T) only -- a batch
//                            gives the bits of H single calls.  error = float(sum / count).
//   scp_select_kernel        one wave: the first minimum of the batch under the acceptance rule against the state the
//                            earlier batches left (lowest error, transform, count); counts the rejected iterations.
// After the last batch scp_fitness_kernel<true> scores the winner alone and flags its inliers by original index; scan +
// compaction give the ascending list.  ONE read-back per align (state + list length); with a trace one per batch.
#pragma once

#include <cfloat>
#include <chrono>
#include <cmath>

#include "block_sums.hpp"
#include "device_scan.hpp"
#include "icp_xform.hpp"
#include "scp_draw.hpp"
#include "scp_umeyama.hpp"
#include "traverse.hpp"

namespace pclhip {
struct ScpState {  // device-resident across the batches of an alignment; read back once
  float lowest_error;
  int converged;
  int best_iteration;
  uint32_t best_count;
  uint32_t rejected;
  uint32_t knn_rows;
  uint32_t pad[2];
  float T[16];
  uint32_t tot_inl[4];  // scan totals of the winner's inlier flags
};
}  // namespace pclhip

struct pclhip_scp {
  pclhip_ctx* ctx = nullptr;
  pclhip_index* target = nullptr;
  // source: a device copy of the records, the points by original index and in kd order (w = original index)
  void* src = nullptr;
  size_t src_stride = 0;
  uint64_t src_n = 0;
  float4* src_orig = nullptr;
  float4* src_sorted = nullptr;
  uint32_t ngroups = 0;
  // features: dense device copies
  float* src_feat = nullptr;
  uint64_t src_feat_n = 0;
  int src_D = 0;
  float* tgt_feat = nullptr;
  uint64_t tgt_feat_n = 0;
  int tgt_D = 0;
  uint32_t* tgt_ok = nullptr;  // 1: the row is finite
  uint32_t tgt_finite = 0;
  // the feature-neighbour cache: per source row k_cached target indices
  int k_cached = 0;
  int32_t* nn_idx = nullptr;
  uint32_t* nn_cnt = nullptr;
  uint32_t* have = nullptr;  // [src_n] the row's neighbours are cached
  uint32_t* need = nullptr;  // [src_n] marked by the running batch
  uint32_t* row_excl = nullptr;
  uint32_t* row_list = nullptr;
  uint32_t* tot_rows = nullptr;  // [4]
  uint2* scan_part = nullptr;
  // batch state (sized by ensure_batch)
  int batch_cap = 0;
  pclhip_scp_trace* rec = nullptr;
  float* T_all = nullptr;       // [B][12]
  uint32_t* survive = nullptr;  // [B]
  uint32_t* surv_excl = nullptr;
  uint32_t* surv_it = nullptr;  // [B] batch slot of survivor h
  float* Ts = nullptr;          // [B][12] the survivors' transforms
  uint32_t* tot_surv = nullptr; // [4]
  uint2* surv_part = nullptr;   // scan scratch of a batch
  double2* part = nullptr;      // [B * ngroups] (sum of d2, inliers)
  uint32_t* h_cnt = nullptr;    // [B]
  float* h_err = nullptr;       // [B]
  uint32_t* inl_flag = nullptr; // [src_n]
  uint32_t* inl_excl = nullptr;
  int32_t* inl_list = nullptr;
  uint64_t inl_count = 0;
  pclhip::ScpState* state = nullptr;
  pclhip::ScpState* state_host = nullptr;  // pinned
  int fit_blocks = 0;
  std::vector<hipEvent_t> events;  // pairs, in launch order: the k-NN, then (hypotheses, fitness) per batch
  double last_ms[3] = {0, 0, 0};
  pclhip_scp_trace* trace = nullptr;
  int trace_capacity = 0;
  float final_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  pclhip_icp* icp = nullptr;  // getFitnessScore, made on first use
  bool icp_source_set = false;
};

namespace pclhip {
namespace {

constexpr int SCP_BLOCK = 256;
constexpr int SCP_WAVES = SCP_BLOCK / WAVE;
constexpr int FK_TILE = 64;  // target rows per LDS tile
constexpr int FK_DMAX = 64;
constexpr int FK_KMAX = 32;
constexpr uint64_t SCP_MAX_ITEMS = uint64_t(1) << 22;  // rows of a batch (hypotheses x groups): 64 MB
inline dim3 scp_blocks_of(uint64_t n) { return dim3(uint32_t((n + SCP_BLOCK - 1) / SCP_BLOCK)); }

// ---- feature k-NN ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCP_BLOCK) void feature_finite_kernel(const float* __restrict__ rows, uint32_t stride_f, uint32_t n,
                                                                   int D, uint32_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (i >= n) return;
  bool f = true;
  for (int d = 0; d < D; ++d) f = f && isfinite(rows[size_t(i) * stride_f + d]);
  ok[i] = f ? 1u : 0u;
}

// One query row per lane (query = list[t] or t; results at slot `query`), one wave per block.  DT: the row's register
// size (33: FPFHSignature33; 64: any D <= 64), KT: the top-k's.
template <int DT, int KT>
__global__ __launch_bounds__(WAVE) void feature_knn_kernel(const float* __restrict__ tgt, uint32_t tgt_stride_f, uint32_t nt,
                                                           const uint32_t* __restrict__ tgt_ok, const float* __restrict__ qry,
                                                           uint32_t qry_stride_f, const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ nlist_dev, uint32_t nq_host, int D, int k,
                                                           uint32_t kk, int32_t* __restrict__ out_idx, float* __restrict__ out_d2,
                                                           uint32_t* __restrict__ out_cnt, uint32_t* __restrict__ have,
                                                           uint32_t* __restrict__ need, uint32_t chunk,
                                                           unsigned long long* __restrict__ partial, uint32_t slots,
                                                           uint32_t S) {
  __shared__ float tile_s[FK_TILE * DT];
  __shared__ uint32_t ok_s[FK_TILE];
  const uint32_t nq = nlist_dev ? *nlist_dev : nq_host;
  const uint32_t qblock = blockIdx.x / S, share = blockIdx.x - qblock * S;  // (a 1-D grid: query block major)
  if (qblock * uint32_t(WAVE) >= nq) return;  // the whole wave
  const uint32_t t = qblock * uint32_t(WAVE) + threadIdx.x;
  const bool real = t < nq;
  const uint32_t q = real ? (list ? list[t] : t) : 0u;
  float qv[DT];
  bool qfinite = real;
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    qv[d] = (real && d < D) ? qry[size_t(q) * qry_stride_f + d] : 0.0f;
    qfinite = qfinite && isfinite(qv[d]);
  }
  uint64_t top[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) top[j] = KEY_NONE;
  // this block's share of the target rows (a multiple of the tile)
  const uint32_t t_lo = uint64_t(share) * chunk < nt ? share * chunk : nt, t_hi = nt - t_lo < chunk ? nt : t_lo + chunk;
  for (uint32_t t0 = t_lo; t0 < t_hi; t0 += FK_TILE) {
    const uint32_t rows = t_hi - t0 < uint32_t(FK_TILE) ? t_hi - t0 : uint32_t(FK_TILE);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < rows * uint32_t(D); e += WAVE) {
      const uint32_t r = e / uint32_t(D), d = e - r * uint32_t(D);
      tile_s[r * DT + d] = tgt[size_t(t0 + r) * tgt_stride_f + d];
    }
    if (threadIdx.x < rows) ok_s[threadIdx.x] = tgt_ok[t0 + threadIdx.x];
    __syncthreads();
    for (uint32_t r = 0; r < rows; ++r) {
      if (ok_s[r] == 0u) continue;  // (the same for every lane)
      const float* row = tile_s + r * DT;
      float acc = 0.0f;
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        if (DT == 33 || d < D) {
          const float diff = __fsub_rn(qv[d], row[d]);
          acc = __fadd_rn(acc, __fmul_rn(diff, diff));
        }
      }
      uint64_t c = make_key(acc, t0 + r);
      if (c < top[KT - 1]) {
#pragma unroll
        for (int j = 0; j < KT; ++j) {  // sorted insert on constant indices
          const uint64_t lo = c < top[j] ? c : top[j], hi = c < top[j] ? top[j] : c;
          top[j] = lo;
          c = hi;
        }
      }
    }
  }
  if (!real) return;
  if (partial != nullptr) {  // the shares' lists are merged by feature_knn_merge_kernel
    if (!qfinite) top[0] = KEY_NONE - 1ull;  // (marks the query; no candidate has index 0xFFFFFFFE at distance +inf)
#pragma unroll
    for (int j = 0; j < KT; ++j) partial[(size_t(share) * slots + t) * KT + j] = top[j];
    return;
  }
  const uint32_t cnt = qfinite ? kk : 0u;
#pragma unroll
  for (int j = 0; j < KT; ++j) {
    if (j < k) {
      const bool on = uint32_t(j) < cnt;
      out_idx[size_t(q) * k + j] = on ? int32_t(key_index(top[j])) : -1;
      if (out_d2) out_d2[size_t(q) * k + j] = on ? key_dist(top[j]) : __builtin_inff();
    }
  }
  out_cnt[q] = cnt;
  if (have) have[q] = 1u;
  if (need) need[q] = 0u;
}

// the sorted lists of the S shares of a query -> its k nearest (the keys are totally ordered: the result is the one-share one)
template <int KT>
__global__ __launch_bounds__(SCP_BLOCK) void feature_knn_merge_kernel(const unsigned long long* __restrict__ partial, uint32_t slots,
                                                                      uint32_t S, const uint32_t* __restrict__ list,
                                                                      const uint32_t* __restrict__ nlist_dev, uint32_t nq_host, int k,
                                                                      uint32_t kk, int32_t* __restrict__ out_idx,
                                                                      float* __restrict__ out_d2, uint32_t* __restrict__ out_cnt,
                                                                      uint32_t* __restrict__ have, uint32_t* __restrict__ need) {
  const uint32_t nq = nlist_dev ? *nlist_dev : nq_host;
  const uint32_t t = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (t >= nq) return;
  const uint32_t q = list ? list[t] : t;
  uint64_t top[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) top[j] = KEY_NONE;
  bool qfinite = true;
  for (uint32_t s = 0; s < S; ++s) {
    const unsigned long long* row = partial + (size_t(s) * slots + t) * KT;
    for (int i = 0; i < KT; ++i) {
      uint64_t c = row[i];
      if (i == 0 && c == KEY_NONE - 1ull) qfinite = false;
      if (!(c < top[KT - 1])) break;  // the share's list is sorted: nothing further fits
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        const uint64_t lo = c < top[j] ? c : top[j], hi = c < top[j] ? top[j] : c;
        top[j] = lo;
        c = hi;
      }
    }
  }
  const uint32_t cnt = qfinite ? kk : 0u;
#pragma unroll
  for (int j = 0; j < KT; ++j) {
    if (j < k) {
      const bool on = uint32_t(j) < cnt;
      out_idx[size_t(q) * k + j] = on ? int32_t(key_index(top[j])) : -1;
      if (out_d2) out_d2[size_t(q) * k + j] = on ? key_dist(top[j]) : __builtin_inff();
    }
  }
  out_cnt[q] = cnt;
  if (have) have[q] = 1u;
  if (need) need[q] = 0u;
}

struct FeatureKnnArgs {
  const float* tgt;
  uint32_t tgt_stride_f, nt;
  const uint32_t* tgt_ok;
  const float* qry;
  uint32_t qry_stride_f;
  const uint32_t* list;
  const uint32_t* nlist_dev;
  uint32_t nq_max;  // the grid covers this many queries (= the count when nlist_dev is null)
  int D, k;
  uint32_t kk;
  int32_t* out_idx;
  float* out_d2;
  uint32_t* out_cnt;
  uint32_t *have, *need;
  uint32_t splits;               // shares of the target rows (1: no merge pass)
  unsigned long long* partial;   // [splits][nq_max][KT] keys when splits > 1
};

constexpr uint32_t FK_MIN_CHUNK = 4 * FK_TILE;  // target rows a share is worth
constexpr uint32_t FK_MAX_SPLITS = 16;
inline int feature_knn_kt(int k) { return k <= 1 ? 1 : k <= 8 ? 8 : 32; }
// shares of the target rows for nq queries: enough blocks for four waves per SIMD, no share below FK_MIN_CHUNK rows, the
// shares' lists within 256 MB
inline uint32_t feature_knn_splits(const pclhip_ctx* ctx, uint32_t nq, uint32_t nt, int k) {
  const uint64_t qwaves = (uint64_t(nq) + WAVE - 1) / WAVE;
  const uint64_t want = uint64_t(ctx->num_cus > 0 ? ctx->num_cus : 1) * 16;
  uint64_t S = qwaves > 0 ? (want + qwaves - 1) / qwaves : 1;
  if (S > nt / FK_MIN_CHUNK) S = nt / FK_MIN_CHUNK;
  const uint64_t per = uint64_t(nq > 0 ? nq : 1) * feature_knn_kt(k) * 8;
  if (S > (uint64_t(256) << 20) / per) S = (uint64_t(256) << 20) / per;
  if (S > FK_MAX_SPLITS) S = FK_MAX_SPLITS;
  return uint32_t(S < 1 ? 1 : S);
}

template <int DT>
void launch_feature_knn_d(hipStream_t s, const FeatureKnnArgs& a) {
  const uint32_t S = a.splits > 1 && a.partial != nullptr ? a.splits : 1u;
  const uint32_t chunk = ((a.nt + S - 1) / S + FK_TILE - 1) / FK_TILE * FK_TILE;
  const dim3 grid(((a.nq_max + WAVE - 1) / WAVE) * S), block(WAVE);
  unsigned long long* partial = S > 1 ? a.partial : nullptr;
#define PCLHIP_FK_LAUNCH(KT)                                                                                                 \
  do {                                                                                                                       \
    hipLaunchKernelGGL((feature_knn_kernel<DT, KT>), grid, block, 0, s, a.tgt, a.tgt_stride_f, a.nt, a.tgt_ok, a.qry,         \
                       a.qry_stride_f, a.list, a.nlist_dev, a.nq_max, a.D, a.k, a.kk, a.out_idx, a.out_d2, a.out_cnt, a.have, \
                       a.need, chunk, partial, a.nq_max, S);                                                                  \
    if (S > 1)                                                                                                               \
      hipLaunchKernelGGL((feature_knn_merge_kernel<KT>), scp_blocks_of(a.nq_max), dim3(SCP_BLOCK), 0, s, partial, a.nq_max, S,  \
                         a.list, a.nlist_dev, a.nq_max, a.k, a.kk, a.out_idx, a.out_d2, a.out_cnt, a.have, a.need);           \
  } while (0)
  if (a.k <= 1)
    PCLHIP_FK_LAUNCH(1);
  else if (a.k <= 8)
    PCLHIP_FK_LAUNCH(8);
  else
    PCLHIP_FK_LAUNCH(32);
#undef PCLHIP_FK_LAUNCH
}

void launch_feature_knn(hipStream_t s, const FeatureKnnArgs& a) {
  if (a.nq_max == 0) return;
  if (a.D == 33)
    launch_feature_knn_d<33>(s, a);
  else
    launch_feature_knn_d<FK_DMAX>(s, a);
}

// the finite rows of a feature set: flags and their number (one read-back)
pclhip_status feature_finite(pclhip_ctx* ctx, const float* rows, uint32_t stride_f, uint32_t n, int D, uint32_t* ok,
                             uint32_t* n_finite) {
  *n_finite = 0;
  if (n == 0) return PCLHIP_OK;
  hipStream_t s = ctx->stream;
  DeviceScope scope(ctx);
  uint2* part = nullptr;
  uint32_t* tot = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((uint64_t(n) + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&tot, 4 * sizeof(uint32_t)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(tot, 0, 4 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(feature_finite_kernel, dim3((n + SCP_BLOCK - 1) / SCP_BLOCK), dim3(SCP_BLOCK), 0, s, rows, stride_f, n, D, ok);
  launch_scan_u32(s, ok, n, part, tot, nullptr);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  uint32_t h[4] = {0, 0, 0, 0};
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(h, tot, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  *n_finite = h[0];
  return PCLHIP_OK;
}

// ---- hypotheses --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCP_BLOCK) void scp_gather_kernel(const char* __restrict__ rec, size_t stride, uint32_t n,
                                                               float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float* p = reinterpret_cast<const float*>(rec + size_t(i) * stride);
  out[i] = make_float4(p[0], p[1], p[2], 0.0f);
}

__global__ __launch_bounds__(SCP_BLOCK) void scp_mark_kernel(uint64_t seed, uint32_t it0, uint32_t nit, int ns, uint32_t n_src,
                                                             const uint32_t* __restrict__ have, uint32_t* __restrict__ need) {
  const uint32_t t = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (t >= nit) return;
  int s[scp::MAX_SAMPLES];
  scp::select_samples(seed, it0 + t, ns, int(n_src), s);
  for (int i = 0; i < ns; ++i)
    if (uint32_t(s[i]) < n_src && have[s[i]] == 0u) need[s[i]] = 1u;  // (every writer stores the same value)
}

// list[excl[i]] = i for the marked i
__global__ __launch_bounds__(SCP_BLOCK) void scp_compact_kernel(const uint32_t* __restrict__ mark, const uint32_t* __restrict__ excl,
                                                                uint32_t n, uint32_t* __restrict__ list) {
  const uint32_t i = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (i < n && mark[i] != 0u) list[excl[i]] = i;
}

struct ScpHypArgs {
  uint64_t seed;
  uint32_t it0, nit;
  int ns, k;
  uint32_t n_src, n_tgt_orig;
  float simsq;
  const float4* src_orig;
  const float4* tgt_pts;     // kd order
  const uint32_t* tgt_rank;  // original index -> position (NO_INDEX: dropped)
  const int32_t* nn_idx;
  const uint32_t* nn_cnt;
  pclhip_scp_trace* rec;
  float* T_all;
  uint32_t* survive;
};

__global__ __launch_bounds__(SCP_BLOCK) void scp_hypothesis_kernel(ScpHypArgs a) {
  const uint32_t t = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (t >= a.nit) return;
  const uint32_t it = a.it0 + t;
  int s[scp::MAX_SAMPLES], m[scp::MAX_SAMPLES];
  float ps[scp::MAX_SAMPLES][3], pt[scp::MAX_SAMPLES][3];
  scp::select_samples(a.seed, it, a.ns, int(a.n_src), s);
  int rejected = 0;
  for (int i = 0; i < a.ns; ++i) {
    m[i] = -1;
    const uint32_t row = uint32_t(s[i]);
    const float4 p = a.src_orig[row];
    ps[i][0] = p.x; ps[i][1] = p.y; ps[i][2] = p.z;
    pt[i][0] = pt[i][1] = pt[i][2] = 0.0f;
    const uint32_t cnt = a.nn_cnt[row];
    if (cnt == 0u) {
      rejected = 2;
      continue;
    }
    // findSimilarFeatures (:146-151): the nearest when k == 1, else one of the k at random
    const int pick = a.k == 1 ? 0 : scp::draw_index(a.seed, it, uint32_t(a.ns + i), int(cnt));
    m[i] = a.nn_idx[size_t(row) * a.k + pick];
    const uint32_t pos = (m[i] >= 0 && uint32_t(m[i]) < a.n_tgt_orig) ? a.tgt_rank[m[i]] : NO_INDEX;
    if (pos == NO_INDEX) {
      rejected = 2;
      continue;
    }
    const float4 q = a.tgt_pts[pos];
    pt[i][0] = q.x; pt[i][1] = q.y; pt[i][2] = q.z;
  }
  if (rejected == 0) {  // thresholdPolygon (correspondence_rejection_poly.h:208-230): one edge when cardinality is 2
    const int edges = a.ns == 2 ? 1 : a.ns;
    for (int i = 0; i < edges && rejected == 0; ++i) {
      const int j = (i + 1) % a.ns;
      if (!scp::edge_similar(scp::edge_sq(ps[i], ps[j]), scp::edge_sq(pt[i], pt[j]), a.simsq)) rejected = 1;
    }
  }
  float T[16];
  cf::zero16(T);
  if (rejected == 0) scp_umeyama(ps, pt, a.ns, T);  // TransformationEstimationSVD (scp_umeyama.hpp)
  a.survive[t] = rejected == 0 ? 1u : 0u;
  for (int e = 0; e < 12; ++e) a.T_all[size_t(t) * 12 + e] = T[e];
  pclhip_scp_trace& r = a.rec[t];
  r.iteration = int(it);
  r.rejected = rejected;
  for (int i = 0; i < scp::MAX_SAMPLES; ++i) {
    r.samples[i] = i < a.ns ? s[i] : -1;
    r.matches[i] = i < a.ns ? m[i] : -1;
  }
  for (int e = 0; e < 16; ++e) r.transformation[e] = T[e];
  r.inliers = 0;
  r.error = FLT_MAX;
}

__global__ __launch_bounds__(SCP_BLOCK) void scp_survivors_kernel(const uint32_t* __restrict__ survive,
                                                                  const uint32_t* __restrict__ excl, uint32_t nit,
                                                                  const float* __restrict__ T_all, float* __restrict__ Ts,
                                                                  uint32_t* __restrict__ surv_it) {
  const uint32_t t = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (t >= nit || survive[t] == 0u) return;
  const uint32_t h = excl[t];
  surv_it[h] = t;
  for (int e = 0; e < 12; ++e) Ts[size_t(h) * 12 + e] = T_all[size_t(t) * 12 + e];
}

// ---- scoring -----------------------------------------------------------------------------------------------------------
// 1-NN distance below a strict bound: the minimum alone (no index is asked for)
struct ScpNearest {
  static constexpr int QPL = 1;
  float best;
  __device__ __forceinline__ float worst(int) const { return best; }
  __device__ __forceinline__ void leaf(const float* l, uint32_t, const float* qx, const float* qy, const float* qz) {
    const v2f qx2 = {qx[0], qx[0]}, qy2 = {qy[0], qy[0]}, qz2 = {qz[0], qz[0]};
    float m = best;
#pragma unroll
    for (int j = 0; j < LEAF / 2; ++j) {
      const v2f r = pair_dist(l, j, qx2, qy2, qz2);
      m = __builtin_fminf(m, __builtin_fminf(r.x, r.y));
    }
    best = m;
  }
};

template <bool EMIT>
__global__ __launch_bounds__(SCP_BLOCK) void scp_fitness_kernel(IndexView ix, const float4* __restrict__ src, uint32_t n,
                                                                const float* __restrict__ Ts, uint32_t t_stride,
                                                                const uint32_t* __restrict__ h_dev, uint32_t h_host, float bound,
                                                                double2* __restrict__ part, uint32_t* __restrict__ flags) {
  __shared__ WaveLdsBoxT<LEAF_BATCH * LEAF_FLOATS * 4> wl_s[SCP_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint32_t H = h_dev ? *h_dev : h_host;
  const uint32_t ngroups = (n + WAVE - 1) / WAVE;
  const uint64_t items = uint64_t(H) * ngroups;
  const uint64_t waves = uint64_t(gridDim.x) * SCP_WAVES;
  TraverseStats ts;
  for (uint64_t item = uint64_t(blockIdx.x) * SCP_WAVES + wave; item < items; item += waves) {
    const uint32_t h = uint32_t(item / ngroups), g = uint32_t(item - uint64_t(h) * ngroups);
    const float* M = Ts + size_t(h) * t_stride;  // (the same for the wave)
    const uint32_t i = g * WAVE + lane;
    float4 p = make_float4(0, 0, 0, 0);
    const bool real = i < n;
    if (real) p = src[i];
    const float tx = xform_row(M[0], M[1], M[2], M[3], p.x, p.y, p.z, 1);
    const float ty = xform_row(M[4], M[5], M[6], M[7], p.x, p.y, p.z, 1);
    const float tz = xform_row(M[8], M[9], M[10], M[11], p.x, p.y, p.z, 1);
    const bool vv[1] = {real && isfinite(tx) && isfinite(ty) && isfinite(tz)};
    const float qx[1] = {tx}, qy[1] = {ty}, qz[1] = {tz};
    ScpNearest pol;
    pol.best = bound;
    traverse(ix, qx, qy, qz, vv, pol, wl_s[wave], topbox_s, ts);
    const bool inl = vv[0] && pol.best < bound;
    const uint64_t mask = __builtin_amdgcn_ballot_w64(inl);
    const double sum = wave_sum_d(inl ? double(pol.best) : 0.0);
    if (lane == 0) part[item] = make_double2(sum, double(__popcll(mask)));
    if (EMIT && real) {
      const uint32_t id = __float_as_uint(p.w);
      if (id < n) flags[id] = inl ? 1u : 0u;
    }
  }
}

// one wave per hypothesis: its rows in a fixed order; error = float(sum / count), FLT_MAX without an inlier
__global__ __launch_bounds__(WAVE) void scp_finalize_kernel(const double2* __restrict__ part, uint32_t ngroups,
                                                            const uint32_t* __restrict__ h_dev, uint32_t h_host,
                                                            uint32_t* __restrict__ h_cnt, float* __restrict__ h_err,
                                                            const uint32_t* __restrict__ surv_it, pclhip_scp_trace* __restrict__ rec) {
  const uint32_t H = h_dev ? *h_dev : h_host;
  const uint32_t h = blockIdx.x;
  if (h >= H) return;
  const int lane = threadIdx.x;
  double a = 0.0, c = 0.0;
  for (uint32_t g = lane; g < ngroups; g += WAVE) {
    const double2 v = part[size_t(h) * ngroups + g];
    a += v.x;
    c += v.y;
  }
  a = wave_sum_d(a);
  c = wave_sum_d(c);
  if (lane == 0) {
    const uint32_t cnt = uint32_t(c);
    const float err = cnt > 0u ? float(a / c) : FLT_MAX;
    h_cnt[h] = cnt;
    h_err[h] = err;
    if (rec != nullptr && surv_it != nullptr) {
      rec[surv_it[h]].inliers = cnt;
      rec[surv_it[h]].error = err;
    }
  }
}

// the acceptance rule (:284-293) over the batch's survivors in iteration order, against the state so far
__global__ __launch_bounds__(WAVE) void scp_select_kernel(const uint32_t* __restrict__ h_dev, uint32_t h_host, uint32_t nit,
                                                          uint32_t it0, int is_guess, uint32_t n_src, float inlier_fraction,
                                                          const uint32_t* __restrict__ h_cnt, const float* __restrict__ h_err,
                                                          const uint32_t* __restrict__ surv_it, const float* __restrict__ Ts,
                                                          const uint32_t* __restrict__ rows_dev, ScpState* __restrict__ st) {
  const uint32_t H = h_dev ? *h_dev : h_host;
  const int lane = threadIdx.x;
  unsigned long long best = ~0ull;
  for (uint32_t h = lane; h < H; h += WAVE) {
    const float frac = float(h_cnt[h]) / float(n_src);
    if (frac >= inlier_fraction) {
      const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(h_err[h])) << 32) | h;  // errors are >= 0
      best = key < best ? key : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = __shfl_xor(best, o);
    best = v < best ? v : best;
  }
  if (lane == 0) {
    if (best != ~0ull) {
      const uint32_t h = uint32_t(best);
      const float err = h_err[h];
      if (err < st->lowest_error) {
        st->lowest_error = err;
        st->converged = 1;
        st->best_iteration = is_guess ? -1 : int(it0 + surv_it[h]);
        st->best_count = h_cnt[h];
        for (int e = 0; e < 12; ++e) st->T[e] = Ts[size_t(h) * 12 + e];
        st->T[12] = st->T[13] = st->T[14] = 0.0f;
        st->T[15] = 1.0f;
      }
    }
    if (!is_guess) st->rejected += nit - H;
    if (rows_dev) st->knn_rows += *rows_dev;
  }
}

__global__ __launch_bounds__(SCP_BLOCK) void scp_inlier_list_kernel(const uint32_t* __restrict__ mark, const uint32_t* __restrict__ excl,
                                                                    uint32_t n, int32_t* __restrict__ list) {
  const uint32_t i = blockIdx.x * SCP_BLOCK + threadIdx.x;
  if (i < n && mark[i] != 0u) list[excl[i]] = int32_t(i);
}

inline dim3 scp_blocks(uint64_t n) { return scp_blocks_of(n); }

// ---- host side -----------------------------------------------------------------------------------------------------------
template <class T>
void scp_free(pclhip_ctx* ctx, T*& p) {
  dev_free_if(ctx, p);
  p = nullptr;
}

void scp_drop_cache(pclhip_scp* S) {
  pclhip_ctx* ctx = S->ctx;
  scp_free(ctx, S->nn_idx);
  S->k_cached = 0;
  if (S->have && S->src_n) (void)hipMemsetAsync(S->have, 0, size_t(S->src_n) * 4, ctx->stream);
}

void scp_drop_batch(pclhip_scp* S) {
  pclhip_ctx* ctx = S->ctx;
  scp_free(ctx, S->rec);
  scp_free(ctx, S->T_all);
  scp_free(ctx, S->survive);
  scp_free(ctx, S->surv_excl);
  scp_free(ctx, S->surv_it);
  scp_free(ctx, S->Ts);
  scp_free(ctx, S->part);
  scp_free(ctx, S->h_cnt);
  scp_free(ctx, S->h_err);
  scp_free(ctx, S->surv_part);
  S->batch_cap = 0;
}

void scp_drop_source(pclhip_scp* S) {
  pclhip_ctx* ctx = S->ctx;
  if (S->icp) {
    pclhip_icp_destroy(S->icp);
    S->icp = nullptr;
    S->icp_source_set = false;
  }
  scp_free(ctx, S->src);
  scp_free(ctx, S->src_orig);
  scp_free(ctx, S->src_sorted);
  scp_free(ctx, S->nn_idx);
  scp_free(ctx, S->nn_cnt);
  scp_free(ctx, S->have);
  scp_free(ctx, S->need);
  scp_free(ctx, S->row_excl);
  scp_free(ctx, S->row_list);
  scp_free(ctx, S->scan_part);
  scp_free(ctx, S->inl_flag);
  scp_free(ctx, S->inl_excl);
  scp_free(ctx, S->inl_list);
  scp_drop_batch(S);
  S->k_cached = 0;
  S->src_n = 0;
  S->ngroups = 0;
  S->inl_count = 0;
}

// the batch a call works with: what the caller asked for, bounded by the rows it needs
int scp_batch_of(const pclhip_scp* S, int asked) {
  uint64_t b = asked > 0 ? uint64_t(asked) : 2048u;
  const uint64_t cap = SCP_MAX_ITEMS / (S->ngroups > 0 ? S->ngroups : 1u);
  if (b > cap) b = cap;
  return int(b > 0 ? b : 1);
}

pclhip_status scp_ensure_batch(pclhip_scp* S, int B) {
  pclhip_ctx* ctx = S->ctx;
  if (B <= S->batch_cap) return PCLHIP_OK;
  scp_drop_batch(S);
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->rec, size_t(B) * sizeof(pclhip_scp_trace)));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->T_all, size_t(B) * 12 * 4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->survive, size_t(B) * 4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->surv_excl, size_t(B) * 4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->surv_it, size_t(B) * 4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->Ts, size_t(B) * 12 * 4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->part, size_t(B) * S->ngroups * sizeof(double2)));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->h_cnt, size_t(B) * 4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->h_err, size_t(B) * 4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->surv_part, size_t((uint64_t(B) + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
  S->batch_cap = B;
  return PCLHIP_OK;
}

// event pair `pair` of the running call (made on first use, kept with the object)
pclhip_status scp_event(pclhip_scp* S, size_t pair, int which, hipEvent_t* ev) {
  while (S->events.size() < 2 * (pair + 1)) {
    hipEvent_t e = nullptr;
    PCLHIP_CHECK_HIP(S->ctx, hipEventCreate(&e));
    S->events.push_back(e);
  }
  *ev = S->events[2 * pair + which];
  return PCLHIP_OK;
}

// H transforms (device, 12 floats each; H on the device or on the host) -> h_cnt / h_err
void scp_launch_score(pclhip_scp* S, const float* Ts, const uint32_t* h_dev, uint32_t h_host, uint32_t h_max, float bound,
                      const uint32_t* surv_it, pclhip_scp_trace* rec) {
  hipStream_t s = S->ctx->stream;
  const IndexView v = S->target->view();
  const uint32_t n = uint32_t(S->src_n);
  const uint64_t want = (uint64_t(h_max) * S->ngroups + SCP_WAVES - 1) / SCP_WAVES;
  const uint32_t grid = uint32_t(want < uint64_t(S->fit_blocks) ? (want > 0 ? want : 1) : uint64_t(S->fit_blocks));
  hipLaunchKernelGGL(scp_fitness_kernel<false>, dim3(grid), dim3(SCP_BLOCK), 0, s, v, S->src_sorted, n, Ts, 12u, h_dev, h_host,
                     bound, S->part, static_cast<uint32_t*>(nullptr));
  hipLaunchKernelGGL(scp_finalize_kernel, dim3(h_max), dim3(WAVE), 0, s, S->part, S->ngroups, h_dev, h_host, S->h_cnt, S->h_err,
                     surv_it, rec);
}

float scp_bound(const pclhip_scp_params* P) {
  return float(P->max_correspondence_distance * P->max_correspondence_distance);  // :319 (corr_dist_threshold_ is a double)
}

pclhip_status scp_copy_dense(pclhip_ctx* ctx, const void* rows, size_t stride, uint64_t n, int D, float** dst) {
  dev_free_if(ctx, *dst);
  *dst = nullptr;
  if (n == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, dst, size_t(n) * D * 4));
  PCLHIP_CHECK_HIP(ctx, hipMemcpy2DAsync(*dst, size_t(D) * 4, rows, stride, size_t(D) * 4, size_t(n), hipMemcpyDefault, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PCLHIP_OK;
}

}  // namespace
}  // namespace pclhip

extern "C" {

pclhip_status pclhip_feature_knn(pclhip_ctx* ctx, const void* target_rows, size_t target_stride, uint64_t n_target,
                                 const void* query_rows, size_t query_stride, uint64_t n_query, int D, int k, int32_t* out_idx,
                                 float* out_d2, uint32_t* out_cnt) {
  using namespace pclhip;
  if (!ctx) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  PCLHIP_REQUIRE(ctx, D >= 1 && D <= FK_DMAX, "D must be in 1 .. 64");
  PCLHIP_REQUIRE(ctx, k >= 1 && k <= FK_KMAX, "k must be in 1 .. 32");
  PCLHIP_REQUIRE(ctx, target_stride >= size_t(D) * 4 && target_stride % 4 == 0 && query_stride >= size_t(D) * 4 && query_stride % 4 == 0,
                 "strides must be multiples of 4 and hold D floats");
  PCLHIP_REQUIRE(ctx, n_target < 0x7FFFFFFFull && n_query < 0x7FFFFFFFull, "too many rows for int32 indices");
  PCLHIP_REQUIRE(ctx, (target_rows || !n_target) && (query_rows || !n_query) && ((out_idx && out_cnt) || !n_query), "null buffer");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DeviceScope scope(ctx);
  float *tgt = nullptr, *qry = nullptr;
  pclhip_status st = scp_copy_dense(ctx, target_rows, target_stride, n_target, D, &tgt);
  scope.mem.push_back(tgt);
  if (st != PCLHIP_OK) return st;
  st = scp_copy_dense(ctx, query_rows, query_stride, n_query, D, &qry);
  scope.mem.push_back(qry);
  if (st != PCLHIP_OK) return st;
  uint32_t* ok = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&ok, size_t(n_target) * 4));
  uint32_t n_finite = 0;
  st = feature_finite(ctx, tgt, uint32_t(D), uint32_t(n_target), D, ok, &n_finite);
  if (st != PCLHIP_OK) return st;
  if (n_finite == 0) {
    set_error(ctx, "pclhip_feature_knn: no finite target row");
    return PCLHIP_ERR_STATE;
  }
  if (n_query == 0) return PCLHIP_OK;
  const size_t nq = size_t(n_query);
  int32_t* d_idx = nullptr;
  float* d_d2 = nullptr;
  uint32_t* d_cnt = nullptr;
  const bool idx_dev = is_device_pointer(out_idx), d2_dev = out_d2 && is_device_pointer(out_d2), cnt_dev = is_device_pointer(out_cnt);
  if (idx_dev) d_idx = out_idx; else PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_idx, nq * k * 4));
  if (d2_dev) d_d2 = out_d2; else if (out_d2) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_d2, nq * k * 4));
  if (cnt_dev) d_cnt = out_cnt; else PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_cnt, nq * 4));
  FeatureKnnArgs a;
  a.tgt = tgt; a.tgt_stride_f = uint32_t(D); a.nt = uint32_t(n_target); a.tgt_ok = ok;
  a.qry = qry; a.qry_stride_f = uint32_t(D); a.list = nullptr; a.nlist_dev = nullptr; a.nq_max = uint32_t(n_query);
  a.D = D; a.k = k; a.kk = n_finite < uint32_t(k) ? n_finite : uint32_t(k);
  a.out_idx = d_idx; a.out_d2 = d_d2; a.out_cnt = d_cnt; a.have = nullptr; a.need = nullptr;
  a.splits = feature_knn_splits(ctx, a.nq_max, a.nt, k);
  a.partial = nullptr;
  if (a.splits > 1) PCLHIP_CHECK_HIP(ctx, scope.alloc(&a.partial, size_t(a.splits) * a.nq_max * feature_knn_kt(k) * 8));
  launch_feature_knn(s, a);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  if (!idx_dev) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_idx, d_idx, nq * k * 4, hipMemcpyDeviceToHost, s));
  if (out_d2 && !d2_dev) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_d2, d_d2, nq * k * 4, hipMemcpyDeviceToHost, s));
  if (!cnt_dev) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_cnt, d_cnt, nq * 4, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  return PCLHIP_OK;
}

void pclhip_scp_params_default(pclhip_scp_params* p) {
  if (!p) return;
  // sample_consensus_prerejective.h:121-131 and its member initialisers; registration.h (corr_dist_threshold_)
  p->max_iterations = 5000;
  p->nr_samples = 3;
  p->k_correspondences = 2;
  p->similarity_threshold = 0.6f;
  p->inlier_fraction = 0.0f;
  p->max_correspondence_distance = std::sqrt(DBL_MAX);
  p->seed = 0;
  p->batch_size = 2048;
}

pclhip_status pclhip_scp_create(pclhip_index* target, pclhip_scp** out) {
  using namespace pclhip;
  if (!target || !out) return PCLHIP_ERR_INVALID;
  *out = nullptr;
  pclhip_ctx* ctx = target->ctx;
  PCLHIP_REQUIRE(ctx, !target->scaled, "SampleConsensusPrerejective needs an index built in the cloud's own coordinates");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  pclhip_scp* S = new pclhip_scp();
  S->ctx = ctx;
  S->target = target;
  if (dev_malloc(ctx, &S->state, sizeof(ScpState)) != hipSuccess || dev_malloc(ctx, &S->tot_rows, 16) != hipSuccess ||
      dev_malloc(ctx, &S->tot_surv, 16) != hipSuccess || pinned_malloc(ctx, &S->state_host, sizeof(ScpState)) != hipSuccess) {
    set_error(ctx, "allocation failed in pclhip_scp_create");
    pclhip_scp_destroy(S);
    return PCLHIP_ERR_HIP;
  }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, scp_fitness_kernel<false>, SCP_BLOCK, 0) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    per_cu = 2;
  }
  S->fit_blocks = per_cu * (ctx->num_cus > 0 ? ctx->num_cus : 1);
  *out = S;
  return PCLHIP_OK;
}

void pclhip_scp_destroy(pclhip_scp* S) {
  using namespace pclhip;
  if (!S) return;
  pclhip_ctx* ctx = S->ctx;
  (void)hipStreamSynchronize(ctx->stream);
  scp_drop_source(S);
  scp_free(ctx, S->src_feat);
  scp_free(ctx, S->tgt_feat);
  scp_free(ctx, S->tgt_ok);
  scp_free(ctx, S->state);
  scp_free(ctx, S->tot_rows);
  scp_free(ctx, S->tot_surv);
  if (S->state_host) pinned_free(ctx, S->state_host, sizeof(ScpState));
  for (hipEvent_t e : S->events) (void)hipEventDestroy(e);
  delete S;
}

pclhip_status pclhip_scp_set_source(pclhip_scp* S, const void* points, size_t stride, uint64_t n) {
  using namespace pclhip;
  if (!S || (!points && n)) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = S->ctx;
  PCLHIP_REQUIRE(ctx, stride >= 12 && stride % 4 == 0, "stride must be a multiple of 4 and >= 12 bytes");
  PCLHIP_REQUIRE(ctx, n < 0x7FFFFFFFull, "cloud too large for int32 indices");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  (void)hipStreamSynchronize(s);
  scp_drop_source(S);
  if (n == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->src, size_t(n) * stride));
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(S->src, points, size_t(n) * stride, hipMemcpyDefault, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  S->src_stride = stride;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->src_orig, size_t(n) * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->src_sorted, size_t(n) * sizeof(float4)));
  hipLaunchKernelGGL(scp_gather_kernel, scp_blocks(n), dim3(SCP_BLOCK), 0, s, static_cast<const char*>(S->src), stride, uint32_t(n),
                     S->src_orig);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  uint32_t n_finite = 0;
  float lo[3], hi[3];
  pclhip_status st = spatial_order(ctx, S->src, stride, n, nullptr, 0, S->src_sorted, uint32_t(n), &n_finite, lo, hi, true, nullptr);
  if (st != PCLHIP_OK) return st;
  const size_t n4 = size_t(n) * 4;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->nn_cnt, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->have, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->need, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->row_excl, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->row_list, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->inl_flag, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->inl_excl, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->inl_list, n4));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->scan_part, size_t((n + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(S->have, 0, n4, s));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(S->need, 0, n4, s));
  S->src_n = n;
  S->ngroups = uint32_t((n + WAVE - 1) / WAVE);
  return PCLHIP_OK;
}

static pclhip_status scp_set_features(pclhip_scp* S, const void* rows, size_t stride, uint64_t n, int D, bool target) {
  using namespace pclhip;
  if (!S || (!rows && n)) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = S->ctx;
  PCLHIP_REQUIRE(ctx, D >= 1 && D <= FK_DMAX, "D must be in 1 .. 64");
  PCLHIP_REQUIRE(ctx, stride >= size_t(D) * 4 && stride % 4 == 0, "stride must be a multiple of 4 and hold D floats");
  PCLHIP_REQUIRE(ctx, n < 0x7FFFFFFFull, "too many rows for int32 indices");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  (void)hipStreamSynchronize(ctx->stream);
  scp_drop_cache(S);
  float** dst = target ? &S->tgt_feat : &S->src_feat;
  const pclhip_status st = scp_copy_dense(ctx, rows, stride, n, D, dst);
  if (st != PCLHIP_OK) return st;
  if (!target) {
    S->src_feat_n = n;
    S->src_D = D;
    return PCLHIP_OK;
  }
  S->tgt_feat_n = n;
  S->tgt_D = D;
  scp_free(ctx, S->tgt_ok);
  S->tgt_finite = 0;
  if (n == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->tgt_ok, size_t(n) * 4));
  return feature_finite(ctx, S->tgt_feat, uint32_t(D), uint32_t(n), D, S->tgt_ok, &S->tgt_finite);
}

pclhip_status pclhip_scp_set_source_features(pclhip_scp* S, const void* rows, size_t stride, uint64_t n, int D) {
  return scp_set_features(S, rows, stride, n, D, false);
}

pclhip_status pclhip_scp_set_target_features(pclhip_scp* S, const void* rows, size_t stride, uint64_t n, int D) {
  return scp_set_features(S, rows, stride, n, D, true);
}

pclhip_status pclhip_scp_set_trace(pclhip_scp* S, pclhip_scp_trace* buf, int capacity) {
  if (!S || capacity < 0 || (capacity > 0 && !buf)) return PCLHIP_ERR_INVALID;
  S->trace = buf;
  S->trace_capacity = capacity;
  return PCLHIP_OK;
}

pclhip_status pclhip_scp_evaluate(pclhip_scp* S, const pclhip_scp_params* P, const float* transforms, int n_transforms,
                                  uint32_t* counts, float* errors) {
  using namespace pclhip;
  if (!S || !P || n_transforms < 0 || (n_transforms > 0 && (!transforms || !counts || !errors))) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = S->ctx;
  PCLHIP_REQUIRE(ctx, S->src_n > 0, "no input source dataset was given");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int B = scp_batch_of(S, P->batch_size);
  pclhip_status st = scp_ensure_batch(S, B);
  if (st != PCLHIP_OK) return st;
  const float bound = scp_bound(P);
  std::vector<float> t12(size_t(B) * 12);
  for (int h0 = 0; h0 < n_transforms; h0 += B) {
    const int H = n_transforms - h0 < B ? n_transforms - h0 : B;
    for (int h = 0; h < H; ++h)
      for (int e = 0; e < 12; ++e) t12[size_t(h) * 12 + e] = transforms[size_t(h0 + h) * 16 + e];
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(S->Ts, t12.data(), size_t(H) * 12 * 4, hipMemcpyHostToDevice, s));
    scp_launch_score(S, S->Ts, nullptr, uint32_t(H), uint32_t(H), bound, nullptr, nullptr);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(counts + h0, S->h_cnt, size_t(H) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(errors + h0, S->h_err, size_t(H) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  }
  return PCLHIP_OK;
}

pclhip_status pclhip_scp_align(pclhip_scp* S, const pclhip_scp_params* P, const float guess_in[16], pclhip_scp_result* res) {
  using namespace pclhip;
  if (!S || !P || !res) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = S->ctx;
  std::memset(res, 0, sizeof *res);
  PCLHIP_REQUIRE(ctx, S->src_n > 0, "no input source dataset was given");
  // the checks of :161-212 and :83-90
  if (!S->src_feat || !S->tgt_feat || S->src_feat_n != S->src_n || S->tgt_feat_n != S->target->n_orig || S->src_D != S->tgt_D) {
    set_error(ctx, !S->src_feat ? "No source features were given! Call setSourceFeatures before aligning."
                   : !S->tgt_feat ? "No target features were given! Call setTargetFeatures before aligning."
                                  : "The points and the feature points need to be in a one-to-one relationship (and of one dimension)");
    return PCLHIP_ERR_STATE;
  }
  PCLHIP_REQUIRE(ctx, P->inlier_fraction >= 0.0f && P->inlier_fraction <= 1.0f, "Illegal inlier fraction, must be in [0,1]");
  PCLHIP_REQUIRE(ctx, P->similarity_threshold >= 0.0f && P->similarity_threshold < 1.0f,
                 "Illegal prerejection similarity threshold, must be in [0,1[");
  PCLHIP_REQUIRE(ctx, P->k_correspondences > 0, "Illegal correspondence randomness, must be > 0");
  PCLHIP_REQUIRE(ctx, P->k_correspondences <= FK_KMAX, "correspondence randomness above 32 is not built");
  PCLHIP_REQUIRE(ctx, P->nr_samples >= 1 && P->nr_samples <= scp::MAX_SAMPLES, "the number of samples must be in 1 .. 8");
  PCLHIP_REQUIRE(ctx, uint64_t(P->nr_samples) <= S->src_n, "The number of samples must not be greater than the number of points");
  PCLHIP_REQUIRE(ctx, P->max_iterations >= 0, "max_iterations must be >= 0");
  if (S->tgt_finite == 0) {
    set_error(ctx, "SampleConsensusPrerejective: no finite target feature row");
    return PCLHIP_ERR_STATE;
  }
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t n = uint32_t(S->src_n);
  const int k = P->k_correspondences, ns = P->nr_samples;
  if (S->k_cached != k) {  // the cache holds the k nearest of a row: another k searches again
    scp_drop_cache(S);
    PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &S->nn_idx, size_t(n) * k * 4));
    S->k_cached = k;
  }
  const int B = scp_batch_of(S, P->batch_size);
  pclhip_status st = scp_ensure_batch(S, B);
  if (st != PCLHIP_OK) return st;
  const float bound = scp_bound(P);
  const float simsq = P->similarity_threshold * P->similarity_threshold;  // correspondence_rejection_poly.h:171
  const float* guess = guess_in ? guess_in : kIdentity16;
  ScpState& h0 = *S->state_host;
  std::memset(&h0, 0, sizeof h0);
  h0.lowest_error = FLT_MAX;
  h0.best_iteration = -2;
  std::memcpy(h0.T, guess, sizeof h0.T);
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(S->state, &h0, sizeof h0, hipMemcpyHostToDevice, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));  // (the pinned block is reused for the read-back)
  size_t pairs = 0;
  hipEvent_t ea = nullptr, eb = nullptr;
  // a guess that is not isApprox(Identity, 0.01f) is scored first (:233-243): |G - I|^2 <= 1e-4 * min(|G|^2, |I|^2)
  double dif = 0.0, gn = 0.0;
  for (int e = 0; e < 16; ++e) {
    dif += double(guess[e] - kIdentity16[e]) * double(guess[e] - kIdentity16[e]);
    gn += double(guess[e]) * double(guess[e]);
  }
  const bool score_guess = !(dif <= 1e-4 * (gn < 4.0 ? gn : 4.0));
  if (score_guess) {
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(S->Ts, guess, 12 * 4, hipMemcpyHostToDevice, s));
    scp_launch_score(S, S->Ts, nullptr, 1u, 1u, bound, nullptr, nullptr);
    hipLaunchKernelGGL(scp_select_kernel, dim3(1), dim3(WAVE), 0, s, static_cast<const uint32_t*>(nullptr), 1u, 1u, 0u, 1, n,
                       P->inlier_fraction, S->h_cnt, S->h_err, static_cast<const uint32_t*>(nullptr), S->Ts, static_cast<const uint32_t*>(nullptr), S->state);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  int ntrace = 0;
  // the feature neighbours of every sample of the alignment that are not cached yet: the draws are a function of the
  // iteration, so the rows are known before the first batch -- one launch over all of them fills the device
  DeviceScope scope(ctx);
  if (P->max_iterations > 0) {
    if ((st = scp_event(S, pairs, 0, &ea)) != PCLHIP_OK || (st = scp_event(S, pairs, 1, &eb)) != PCLHIP_OK) return st;
    ++pairs;
    (void)hipEventRecord(ea, s);
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(S->tot_rows, 0, 16, s));
    const uint32_t nall = uint32_t(P->max_iterations);
    hipLaunchKernelGGL(scp_mark_kernel, scp_blocks(nall), dim3(SCP_BLOCK), 0, s, P->seed, 0u, nall, ns, n, S->have, S->need);
    launch_scan_u32(s, S->need, n, S->scan_part, S->tot_rows, S->row_excl);
    hipLaunchKernelGGL(scp_compact_kernel, scp_blocks(n), dim3(SCP_BLOCK), 0, s, S->need, S->row_excl, n, S->row_list);
    const uint64_t most = uint64_t(nall) * ns;
    FeatureKnnArgs a;
    a.tgt = S->tgt_feat; a.tgt_stride_f = uint32_t(S->tgt_D); a.nt = uint32_t(S->tgt_feat_n); a.tgt_ok = S->tgt_ok;
    a.qry = S->src_feat; a.qry_stride_f = uint32_t(S->src_D); a.list = S->row_list; a.nlist_dev = S->tot_rows;
    a.nq_max = uint32_t(most < n ? most : n);
    a.D = S->src_D; a.k = k; a.kk = S->tgt_finite < uint32_t(k) ? S->tgt_finite : uint32_t(k);
    a.out_idx = S->nn_idx; a.out_d2 = nullptr; a.out_cnt = S->nn_cnt; a.have = S->have; a.need = S->need;
    a.splits = feature_knn_splits(ctx, a.nq_max, a.nt, k);
    a.partial = nullptr;
    if (a.splits > 1) PCLHIP_CHECK_HIP(ctx, scope.alloc(&a.partial, size_t(a.splits) * a.nq_max * feature_knn_kt(k) * 8));
    launch_feature_knn(s, a);
    (void)hipEventRecord(eb, s);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  for (int it0 = 0; it0 < P->max_iterations; it0 += B) {
    const uint32_t nit = uint32_t(P->max_iterations - it0 < B ? P->max_iterations - it0 : B);
    // the hypotheses and the survivors' transforms
    if ((st = scp_event(S, pairs, 0, &ea)) != PCLHIP_OK || (st = scp_event(S, pairs, 1, &eb)) != PCLHIP_OK) return st;
    ++pairs;
    (void)hipEventRecord(ea, s);
    ScpHypArgs ha;
    ha.seed = P->seed; ha.it0 = uint32_t(it0); ha.nit = nit; ha.ns = ns; ha.k = k; ha.n_src = n;
    ha.n_tgt_orig = uint32_t(S->target->n_orig); ha.simsq = simsq; ha.src_orig = S->src_orig; ha.tgt_pts = S->target->pts;
    ha.tgt_rank = S->target->rank; ha.nn_idx = S->nn_idx; ha.nn_cnt = S->nn_cnt; ha.rec = S->rec; ha.T_all = S->T_all;
    ha.survive = S->survive;
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(S->tot_surv, 0, 16, s));
    hipLaunchKernelGGL(scp_hypothesis_kernel, scp_blocks(nit), dim3(SCP_BLOCK), 0, s, ha);
    launch_scan_u32(s, S->survive, nit, S->surv_part, S->tot_surv, S->surv_excl);
    hipLaunchKernelGGL(scp_survivors_kernel, scp_blocks(nit), dim3(SCP_BLOCK), 0, s, S->survive, S->surv_excl, nit, S->T_all, S->Ts,
                       S->surv_it);
    (void)hipEventRecord(eb, s);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    // scoring and the batch's winner
    if ((st = scp_event(S, pairs, 0, &ea)) != PCLHIP_OK || (st = scp_event(S, pairs, 1, &eb)) != PCLHIP_OK) return st;
    ++pairs;
    (void)hipEventRecord(ea, s);
    scp_launch_score(S, S->Ts, S->tot_surv, 0u, nit, bound, S->surv_it, S->rec);
    hipLaunchKernelGGL(scp_select_kernel, dim3(1), dim3(WAVE), 0, s, S->tot_surv, 0u, nit, uint32_t(it0), 0, n, P->inlier_fraction,
                       S->h_cnt, S->h_err, S->surv_it, S->Ts, it0 == 0 ? S->tot_rows : nullptr, S->state);
    (void)hipEventRecord(eb, s);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    if (ntrace < S->trace_capacity) {  // the trace asks for the batch's records
      const int m = S->trace_capacity - ntrace < int(nit) ? S->trace_capacity - ntrace : int(nit);
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(S->trace + ntrace, S->rec, size_t(m) * sizeof(pclhip_scp_trace), hipMemcpyDeviceToHost, s));
      PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
      ntrace += m;
    }
  }
  // the winner alone: its inliers by original index, ascending
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(S->inl_flag, 0, size_t(n) * 4, s));
  {
    const IndexView v = S->target->view();
    const uint64_t want = (uint64_t(S->ngroups) + SCP_WAVES - 1) / SCP_WAVES;
    const uint32_t grid = uint32_t(want < uint64_t(S->fit_blocks) ? want : uint64_t(S->fit_blocks));
    hipLaunchKernelGGL(scp_fitness_kernel<true>, dim3(grid), dim3(SCP_BLOCK), 0, s, v, S->src_sorted, n, S->state->T, 16u,
                       static_cast<const uint32_t*>(nullptr), 1u, bound, S->part, S->inl_flag);
    launch_scan_u32(s, S->inl_flag, n, S->scan_part, S->state->tot_inl, S->inl_excl);
    hipLaunchKernelGGL(scp_inlier_list_kernel, scp_blocks(n), dim3(SCP_BLOCK), 0, s, S->inl_flag, S->inl_excl, n, S->inl_list);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(S->state_host, S->state, sizeof(ScpState), hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));  // the one read-back
  const ScpState& h = *S->state_host;
  S->last_ms[0] = S->last_ms[1] = S->last_ms[2] = 0.0;
  for (size_t p = 0; p < pairs; ++p) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, S->events[2 * p], S->events[2 * p + 1]) == hipSuccess) S->last_ms[p == 0 ? 0 : 1 + (p - 1) % 2] += ms;
  }
  std::memcpy(res->final_transformation, h.T, sizeof h.T);
  std::memcpy(S->final_T, h.T, sizeof h.T);
  S->inl_count = h.converged ? h.tot_inl[0] : 0;
  res->converged = h.converged;
  res->iterations = P->max_iterations;
  res->rejected = int(h.rejected);
  res->best_iteration = h.best_iteration;
  res->best_error = h.lowest_error;
  res->best_count = h.best_count;
  res->trace_count = ntrace;
  res->knn_rows = h.knn_rows;
  res->knn_ms = S->last_ms[0];
  res->hypothesis_ms = S->last_ms[1];
  res->fitness_ms = S->last_ms[2];
  res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PCLHIP_OK;
}

pclhip_status pclhip_scp_inliers(pclhip_scp* S, int32_t* out, uint64_t capacity, uint64_t* count) {
  using namespace pclhip;
  if (!S || !count) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = S->ctx;
  *count = S->inl_count;
  if (S->inl_count == 0 || !out) return PCLHIP_OK;
  if (capacity < S->inl_count) {
    set_error(ctx, "pclhip_scp_inliers: capacity too small (count holds the required size)");
    return PCLHIP_ERR_OVERFLOW;
  }
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out, S->inl_list, size_t(S->inl_count) * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PCLHIP_OK;
}

pclhip_status pclhip_scp_fitness_score(pclhip_scp* S, const float T[16], double max_range, double* score, uint64_t* nr) {
  if (!S || !score) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = S->ctx;
  PCLHIP_REQUIRE(ctx, S->src_n > 0, "the fitness score needs a source");
  pclhip_status st = PCLHIP_OK;
  if (!S->icp) {
    st = pclhip_icp_create(S->target, &S->icp);
    if (st != PCLHIP_OK) return st;
  }
  if (!S->icp_source_set) {
    st = pclhip_icp_set_source(S->icp, S->src, S->src_stride, S->src_n);
    if (st != PCLHIP_OK) return st;
    S->icp_source_set = true;
  }
  return pclhip_icp_fitness_score(S->icp, T ? T : S->final_T, max_range, score, nr);
}

void pclhip_scp_last_ms(const pclhip_scp* S, double* knn_ms, double* hypothesis_ms, double* fitness_ms) {
  if (knn_ms) *knn_ms = S ? S->last_ms[0] : 0.0;
  if (hypothesis_ms) *hypothesis_ms = S ? S->last_ms[1] : 0.0;
  if (fitness_ms) *fitness_ms = S ? S->last_ms[2] : 0.0;
}

}  // extern "C"
