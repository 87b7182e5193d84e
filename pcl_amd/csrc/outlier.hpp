// outlier.hpp -- StatisticalOutlierRemoval and RadiusOutlierRemoval over the index (included by radius.hip).
// Replaces the serial k-NN loops of pcl::StatisticalOutlierRemoval<PointT>::applyFilterIndices
// (filters/include/pcl/filters/impl/statistical_outlier_removal.hpp:47-132) and
// pcl::RadiusOutlierRemoval<PointT>::applyFilterIndices (.../radius_outlier_removal.hpp:48-172).
//
// Pipeline (one stream, one read-back at the end):
//   outlier_pos_kernel     entry j (the cloud's records, or indices[j]) -> sorted position (rank), NO_INDEX for a non-finite
//                          record; with indices, the positions asked for are marked and compacted (device_scan.hpp) so the
//                          queries still run in kd order
//   sor_dist_kernel<K>     the K smallest d2 VALUES of each query (TopKDist: no indices, no positions; K = 16 / 32 / 64 in
//                          registers), then sqrt in double of every float d2, summed in ascending order, / (K - 1), rounded
//                          to float: one float per query
//   sor_dist_heap_kernel   the same for K > 64 with a per-thread max-heap of floats in global memory (grid-sized, not
//                          query-sized)
//   ror_count_kernel       capped count of the points with d2 <= t: a lane stops wanting leaves once it has min_pts + 1
//   sor_partial_kernel     per-entry distances in query order + per-block (sum, sq_sum, valid) in double
//   sor_finalize_kernel    the block sums -> mean, stddev, threshold on the device (both: the fixed order of block_sums.hpp)
//   outlier_keep_kernel    classification; the keep flags are scanned (device_scan.hpp) and
//   outlier_emit_kernel    writes the kept and removed ids, stable, in query order.
// The three search kernels give every lane one query inside traverse.hpp's for_each_query_group; FPFH's and the clusters'
// kernels (fpfh.hpp, cluster.hpp) run in the same loop and borrow this file's launch geometry.
#pragma once

#include <algorithm>
#include <limits>

#include "block_sums.hpp"
#include "device_scan.hpp"
#include "traverse.hpp"

namespace pclhip {
namespace {

constexpr int OR_BLOCK = 256;
constexpr int OR_WAVES = OR_BLOCK / WAVE;
constexpr int OR_PER = 16;                       // entries per thread of the fixed-order partial sums
constexpr int OR_CHUNK = OR_BLOCK * OR_PER;      // entries per block

// entry j -> sorted position of its record; records out of range count into *bad; mark[pos] = 1 for the compaction
__global__ __launch_bounds__(OR_BLOCK) void outlier_pos_kernel(const int32_t* __restrict__ idx, uint32_t m,
                                                             const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                             uint32_t* __restrict__ epos, uint32_t* __restrict__ mark,
                                                             uint32_t* __restrict__ bad) {
  const uint32_t j = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (j >= m) return;
  const int64_t id = idx ? int64_t(idx[j]) : int64_t(j);
  uint32_t pos = NO_INDEX;
  if (id >= 0 && uint64_t(id) < n_orig) pos = rank[id];
  else atomicAdd(bad, 1u);
  epos[j] = pos;
  if (mark != nullptr && pos != NO_INDEX) mark[pos] = 1u;
}

// positions p with mark[p] != 0, ascending (excl: exclusive scan of mark)
__global__ __launch_bounds__(OR_BLOCK) void outlier_compact_kernel(const uint32_t* __restrict__ mark,
                                                                 const uint32_t* __restrict__ excl, uint32_t n,
                                                                 uint32_t* __restrict__ qpos) {
  const uint32_t p = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (p < n && mark[p] != 0u) qpos[excl[p]] = p;
}

// sum_{c=1..kk-1} sqrt(double(d2[c])) in ascending order, / (kk - 1), to float (statistical_outlier_removal.hpp:96-99).
// The square root is taken in double of the float d2 (the reference's sqrt(float) may resolve either way; on its own test
// cloud both give the same filter).  kk == 1 divides 0 by 0, as the reference does.
// (A rolled loop that shifts the run down by one per term: unrolled, the 63 double square roots of K = 64 were scheduled
// side by side and took the kernel to 256 VGPRs + 27 AGPRs.)
template <int K>
__device__ __forceinline__ float sor_mean_of(float* d, int kk) {
  double s = 0.0;
#pragma unroll 1
  for (int c = 1; c < kk; ++c) {
#pragma unroll
    for (int j = 0; j < K - 1; ++j) d[j] = d[j + 1];  // d[0] = the c-th smallest
    s += sqrt(double(d[0]));
  }
  return float(s / double(kk - 1));
}

// One lane per query; the queries are the index's own points (qpos == nullptr: position i) or the ascending positions
// qpos[0..nq), so a wave's queries are spatially compact either way.  kk = min(mean_k + 1, finite points) <= K.
// waves per SIMD (kernel-resource-usage, gfx950): K = 16: 98 VGPRs -> 4; K = 32: 128 -> 4; K = 64: 213 VGPRs -> 2, no
// scratch (bounded to 3 waves it spills 180 bytes per lane)
#define SOR_MINW(K) ((K) <= 32 ? 4 : 1)
template <int K>
__global__ __launch_bounds__(OR_BLOCK, SOR_MINW(K)) void sor_dist_kernel(IndexView ix, const uint32_t* __restrict__ qpos, uint32_t nq,
                                                            int kk, float* __restrict__ dpos) {
  // TopKDist stages no original indices: 3 KB of staging per wave
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, qpos, nq, [&](uint32_t pos, bool valid, float4 p) {
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {valid};
    TopKDist<K> dist;
    dist.init(nullptr);
    // the own leaf first (it holds the query itself): the walk starts with a k-th distance of a few point spacings
    if (valid) dist.seed_own_leaf(ix.soa, pos / LEAF, qx, qy, qz);
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a query
    traverse<TopKDist<K>, true>(ix, qx, qy, qz, vv, dist, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (valid) dpos[pos] = sor_mean_of<K>(dist.d, kk);
  });
}

// K > 64: the kk smallest d2 in a per-thread binary max-heap of floats, heap[slot * nthreads + thread] (coalesced), then
// sorted ascending in place and summed like sor_mean_of.  Wave-uniform leaf evaluation (TopKHeap's scheme).
struct TopKDistHeap {
  float* heap;
  size_t stride;
  int k;
  float root;
  static constexpr int QPL = 1;
  __device__ __forceinline__ float worst(int) const { return root; }
  __device__ __forceinline__ float at(int i) const { return heap[size_t(i) * stride]; }
  __device__ __forceinline__ void put(int i, float v) { heap[size_t(i) * stride] = v; }
  __device__ void init() {
    for (int i = 0; i < k; ++i) put(i, __builtin_inff());
    root = __builtin_inff();
  }
  __device__ void sift_down(float v, int end) {  // v replaces the root of heap[0..end)
    int i = 0;
    for (;;) {
      const int l = 2 * i + 1, r = l + 1;
      int big = i;
      float bv = v;
      if (l < end) {
        const float lv = at(l);
        if (lv > bv) {
          bv = lv;
          big = l;
        }
      }
      if (r < end) {
        const float rv = at(r);
        if (rv > bv) {
          bv = rv;
          big = r;
        }
      }
      if (big == i) break;
      put(i, bv);
      i = big;
    }
    put(i, v);
  }
  __device__ __forceinline__ void leaf(const float* l, uint32_t, const float* qx, const float* qy, const float* qz) {
    for (int c = 0; c < LEAF; ++c) {
      const float d = l2_simple(qx[0], qy[0], qz[0], l[c], l[LEAF + c], l[2 * LEAF + c]);
      if (d < root) {
        sift_down(d, k);
        root = at(0);
      }
    }
  }
  __device__ void sort_ascending() {
    for (int end = k - 1; end > 0; --end) {
      const float top = at(0), last = at(end);
      put(end, top);
      sift_down(last, end);
    }
  }
};

__global__ __launch_bounds__(OR_BLOCK) void sor_dist_heap_kernel(IndexView ix, const uint32_t* __restrict__ qpos, uint32_t nq,
                                                                 int kk, float* __restrict__ heap, float* __restrict__ dpos) {
  __shared__ WaveLdsBoxT<LEAF_BATCH * LEAF_FLOATS * 4> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  TopKDistHeap pol;
  pol.stride = size_t(gridDim.x) * OR_BLOCK;
  pol.heap = heap + size_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  pol.k = kk;
  for_each_query_group(ix, qpos, nq, [&](uint32_t pos, bool valid, float4 p) {
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {valid};
    pol.init();
    traverse<TopKDistHeap>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts);
    if (valid) {
      pol.sort_ascending();
      double s = 0.0;
      for (int c = 1; c < kk; ++c) s += sqrt(double(pol.at(c)));
      dpos[pos] = float(s / double(kk - 1));
    }
  });
}

// RadiusOutlierRemoval: how many points of the index lie within d2 <= t, counted up to `need` = min_pts + 1 (the query
// itself included).  A lane that has them reports a negative bound: the traversal neither stages nor hands it another
// leaf, and a wave whose lanes are all done stops.  Lane-sparse evaluation, the own leaf first.  (Inclusive, where
// traverse.hpp's leaf_hits_lt is strict: see there.)
struct RorCount {
  float t;
  uint32_t need, cnt;
  uint32_t exclude = NO_INDEX;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return cnt >= need ? -1.0f : t; }
  template <int STRIDE>
  __device__ __forceinline__ void block(const float4* s, const float* qx, const float* qy, const float* qz) {
    const v2f qx2 = {qx[0], qx[0]}, qy2 = {qy[0], qy[0]}, qz2 = {qz[0], qz[0]};
    uint32_t c = 0;
#pragma unroll
    for (int c4 = 0; c4 < LEAF / 4; ++c4) {
      v2f r0, r1;
      quad_dist<STRIDE>(s, c4, qx2, qy2, qz2, r0, r1);
      c += (r0.x <= t ? 1u : 0u) + (r0.y <= t ? 1u : 0u) + (r1.x <= t ? 1u : 0u) + (r1.y <= t ? 1u : 0u);
    }
    cnt += c;
  }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id != NO_INDEX && cnt < need) block<16>(reinterpret_cast<const float4*>(buf) + slot, qx, qy, qz);
  }
  __device__ __forceinline__ void seed_own_leaf(const float* soa, uint32_t leaf_id, const float* qx, const float* qy,
                                                const float* qz) {
    block<1>(reinterpret_cast<const float4*>(soa + size_t(leaf_id) * LEAF_FLOATS), qx, qy, qz);
    exclude = leaf_id;
  }
};

__global__ __launch_bounds__(OR_BLOCK) void ror_count_kernel(IndexView ix, const uint32_t* __restrict__ qpos, uint32_t nq,
                                                             float t, uint32_t need, uint8_t* __restrict__ enough) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, qpos, nq, [&](uint32_t pos, bool valid, float4 p) {
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    RorCount pol;
    pol.t = t;
    pol.need = need;
    pol.cnt = 0;
    if (valid) pol.seed_own_leaf(ix.soa, pos / LEAF, qx, qy, qz);
    const bool vv[1] = {valid && pol.cnt < need};  // lanes done with their own leaf take no part in the walk
    const uint32_t start = uniform_u32(pos / LEAF);
    traverse<RorCount, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (valid) enough[pos] = pol.cnt >= need ? 1u : 0u;
  });
}

// per entry: the distance in query order (0 for a non-finite record) and per block (sum d, sum fl(d*d), valid) in double.
// Thread t of block b sums entries b * OR_CHUNK + t * OR_PER + [0, OR_PER) in order, then block_rows: the order depends
// on the input alone, not on the device's grid.
__global__ __launch_bounds__(OR_BLOCK) void sor_partial_kernel(const uint32_t* __restrict__ epos, uint32_t m,
                                                             const float* __restrict__ dpos, float* __restrict__ dist,
                                                             double* __restrict__ partial) {
  const uint64_t base = uint64_t(blockIdx.x) * OR_CHUNK + uint64_t(threadIdx.x) * OR_PER;
  double acc[3] = {0.0, 0.0, 0.0};  // sum, sq_sum, valid
  for (int e = 0; e < OR_PER; ++e) {
    const uint64_t j = base + e;
    if (j < m) {
      const uint32_t pos = epos[j];
      const float d = pos != NO_INDEX ? dpos[pos] : 0.0f;
      dist[j] = d;
      acc[0] += double(d);
      acc[1] += double(__fmul_rn(d, d));
      acc[2] += pos != NO_INDEX ? 1.0 : 0.0;
    }
  }
  block_rows<3, OR_WAVES, 3>(acc, partial);
}

// one block: thread t adds the rows t, t + OR_BLOCK, ..., then the wave and block steps -> stats[0..5] = mean, stddev,
// threshold, sum, sq_sum, valid
// (statistical_outlier_removal.hpp:104-117: mean = sum / valid, variance = (sq_sum - sum^2 / valid) / (valid - 1))
__global__ __launch_bounds__(OR_BLOCK) void sor_finalize_kernel(const double* __restrict__ partial, uint32_t nb,
                                                              double std_mul, double* __restrict__ stats) {
  double acc[3] = {0.0, 0.0, 0.0};
  for (uint32_t b = threadIdx.x; b < nb; b += OR_BLOCK) {
    acc[0] += partial[3 * b];
    acc[1] += partial[3 * b + 1];
    acc[2] += partial[3 * b + 2];
  }
  __shared__ double ws[OR_WAVES][3];
  wave_rows(acc, ws);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double a = block_column<OR_WAVES>(ws, 0), b = block_column<OR_WAVES>(ws, 1), c = block_column<OR_WAVES>(ws, 2);
    const double mean = a / c;
    const double var = (b - a * a / c) / (c - 1.0);
    const double sd = sqrt(var);
    stats[0] = mean;
    stats[1] = sd;
    stats[2] = mean + std_mul * sd;
    stats[3] = a;
    stats[4] = b;
    stats[5] = c;
  }
}

// keep[j]: SOR removes d > thr (negative: d <= thr) -- a NaN distance or threshold removes nothing; ROR: enough XOR
// negative, where a non-finite record has no neighbours and (not dense) is removed either way
__global__ __launch_bounds__(OR_BLOCK) void outlier_keep_kernel(const uint32_t* __restrict__ epos, uint32_t m,
                                                              const float* __restrict__ dist, const double* __restrict__ stats,
                                                              const uint8_t* __restrict__ enough, int negative, int dense,
                                                              uint32_t* __restrict__ keep) {
  const uint32_t j = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (j >= m) return;
  bool k;
  if (dist != nullptr) {
    const double d = double(dist[j]), thr = stats[2];
    k = !(negative ? (d <= thr) : (d > thr));
  } else {
    const uint32_t pos = epos[j];
    const bool fin = pos != NO_INDEX;
    const bool en = fin && enough[pos] != 0;
    k = (en != (negative != 0)) && (dense || fin);
  }
  keep[j] = k ? 1u : 0u;
}

// stable split of the entries' ids by keep (excl: exclusive scan of keep)
__global__ __launch_bounds__(OR_BLOCK) void outlier_emit_kernel(const int32_t* __restrict__ idx, uint32_t m,
                                                              const uint32_t* __restrict__ keep,
                                                              const uint32_t* __restrict__ excl, int32_t* __restrict__ kept,
                                                              int32_t* __restrict__ removed) {
  const uint32_t j = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (j >= m) return;
  const int32_t id = idx ? idx[j] : int32_t(j);
  const uint32_t e = excl[j];
  if (keep[j] != 0u) {
    if (kept) kept[e] = id;
  } else if (removed) {
    removed[j - e] = id;
  }
}

template <class Kern>
int outlier_grid(pclhip_ctx* ctx, Kern kernel, uint32_t nq) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, OR_BLOCK, 0) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    per_cu = 2;
  }
  const uint32_t ngroups = (nq + WAVE - 1) / WAVE;
  const uint64_t want = (uint64_t(ngroups) + OR_WAVES - 1) / OR_WAVES;
  const uint64_t cap = uint64_t(per_cu) * uint64_t(ctx->num_cus > 0 ? ctx->num_cus : 1);
  return int(want < cap ? (want > 0 ? want : 1) : cap);
}

inline dim3 or_blocks(uint64_t m) { return dim3(uint32_t((m + OR_BLOCK - 1) / OR_BLOCK)); }

}  // namespace

// The host side of both filters (pclhip_statistical_outlier_removal / pclhip_radius_outlier_removal, api.hip).
pclhip_status outlier_filter(pclhip_index* ix, const int32_t* indices, uint64_t n_indices, const OutlierParams& prm,
                             int32_t* kept, uint64_t* n_kept, int32_t* removed, uint64_t* n_removed, float* mean_dist,
                             double* stats6) {
  pclhip_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const bool sor = prm.kind == OutlierParams::SOR;
  const uint64_t m64 = indices ? n_indices : ix->n_orig;
  PCLHIP_REQUIRE(ctx, m64 < 0x7FFFFFFFull, "too many queries");
  const uint32_t m = uint32_t(m64), n = ix->n;
  *n_kept = 0;
  *n_removed = 0;
  if (stats6) {
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    stats6[0] = stats6[1] = stats6[2] = qnan;  // 0 / 0, as the reference divides
    stats6[3] = stats6[4] = stats6[5] = 0.0;
  }
  if (m == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  DeviceScope scope(ctx);
  const void* d_idx_v = nullptr;
  void* owned = nullptr;
  if (indices) {
    const pclhip_status st = to_device(ctx, indices, size_t(m) * 4, &d_idx_v, &owned);
    if (st != PCLHIP_OK) return st;
    scope.mem.push_back(owned);
  }
  const int32_t* d_idx = static_cast<const int32_t*>(d_idx_v);
  // read-back block: stats[6] (double), then the scans' totals and the bad-index counter
  struct ReadBack {
    double stats[6];
    uint32_t tot_keep[4];
    uint32_t tot_q[4];
    uint32_t bad;
    uint32_t pad[3];
  };
  ReadBack* rb = nullptr;
  uint32_t *epos = nullptr, *keep = nullptr, *kexcl = nullptr, *mark = nullptr, *qexcl = nullptr, *qpos = nullptr;
  uint2* part = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rb, sizeof(ReadBack)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&epos, size_t(m) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&keep, size_t(m) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&kexcl, size_t(m) * 4));
  const uint64_t scan_blocks = (uint64_t(m > n ? m : n) + SC_BLOCK - 1) / SC_BLOCK;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t(scan_blocks + 1) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(rb, 0, sizeof(ReadBack), s));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.event(&e0));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e1));
  (void)hipEventRecord(e0, s);
  if (indices && n > 0) {
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&mark, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(mark, 0, size_t(n) * 4, s));
  }
  hipLaunchKernelGGL(outlier_pos_kernel, or_blocks(m), dim3(OR_BLOCK), 0, s, d_idx, m, ix->rank, ix->n_orig, epos, mark,
                     &rb->bad);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  uint32_t nq = n;
  if (indices) {
    // the positions asked for, ascending: queries stay in kd order
    uint32_t hb[4] = {0, 0, 0, 0};
    if (n > 0) {
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&qexcl, size_t(n) * 4));
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&qpos, size_t(n) * 4));
      launch_scan_u32(s, mark, n, part, rb->tot_q, qexcl);
      hipLaunchKernelGGL(outlier_compact_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, mark, qexcl, n, qpos);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    }
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hb, rb->tot_q, 16, hipMemcpyDeviceToHost, s));
    uint32_t bad = 0;
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&bad, &rb->bad, 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    PCLHIP_REQUIRE(ctx, bad == 0, "indices out of range");
    nq = hb[0];
  }
  const IndexView v = ix->view();
  float* dpos = nullptr;
  uint8_t* enough = nullptr;
  if (sor) {
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&dpos, size_t(n > 0 ? n : 1) * 4));
    const int64_t kk64 = std::min<int64_t>(int64_t(prm.mean_k) + 1, int64_t(n));
    const int kk = int(kk64);
    if (nq > 0) {
      if (kk <= 16) {
        PCLHIP_LAUNCH_FED(ctx, sor_dist_kernel<16>, dim3(outlier_grid(ctx, sor_dist_kernel<16>, nq)), dim3(OR_BLOCK), 0, s, v,
                          qpos, nq, kk, dpos);
      } else if (kk <= 32) {
        PCLHIP_LAUNCH_FED(ctx, sor_dist_kernel<32>, dim3(outlier_grid(ctx, sor_dist_kernel<32>, nq)), dim3(OR_BLOCK), 0, s, v,
                          qpos, nq, kk, dpos);
      } else if (kk <= 64) {
        PCLHIP_LAUNCH_FED(ctx, sor_dist_kernel<64>, dim3(outlier_grid(ctx, sor_dist_kernel<64>, nq)), dim3(OR_BLOCK), 0, s, v,
                          qpos, nq, kk, dpos);
      } else {
        const int grid = outlier_grid(ctx, sor_dist_heap_kernel, nq);
        float* heap = nullptr;
        PCLHIP_CHECK_HIP(ctx, scope.alloc(&heap, size_t(grid) * OR_BLOCK * size_t(kk) * 4));
        PCLHIP_LAUNCH_FED(ctx, sor_dist_heap_kernel, dim3(grid), dim3(OR_BLOCK), 0, s, v, qpos, nq, kk, heap, dpos);
      }
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    }
    float* dist = nullptr;
    const bool dist_dev = mean_dist != nullptr && is_device_pointer(mean_dist);
    if (dist_dev) dist = mean_dist;
    else PCLHIP_CHECK_HIP(ctx, scope.alloc(&dist, size_t(m) * 4));
    const uint32_t nb = uint32_t((uint64_t(m) + OR_CHUNK - 1) / OR_CHUNK);
    double* partial = nullptr;
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&partial, size_t(nb) * 3 * sizeof(double)));
    hipLaunchKernelGGL(sor_partial_kernel, dim3(nb), dim3(OR_BLOCK), 0, s, epos, m, dpos, dist, partial);
    hipLaunchKernelGGL(sor_finalize_kernel, dim3(1), dim3(OR_BLOCK), 0, s, partial, nb, prm.std_mul, rb->stats);
    hipLaunchKernelGGL(outlier_keep_kernel, or_blocks(m), dim3(OR_BLOCK), 0, s, epos, m, dist, rb->stats,
                       (const uint8_t*)nullptr, prm.negative, 1, keep);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    if (mean_dist != nullptr && !dist_dev)
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(mean_dist, dist, size_t(m) * 4, hipMemcpyDeviceToHost, s));
  } else {
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&enough, size_t(n > 0 ? n : 1)));
    if (nq > 0) {
      PCLHIP_LAUNCH_FED(ctx, ror_count_kernel, dim3(outlier_grid(ctx, ror_count_kernel, nq)), dim3(OR_BLOCK), 0, s, v, qpos,
                        nq, prm.t, prm.need, enough);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(outlier_keep_kernel, or_blocks(m), dim3(OR_BLOCK), 0, s, epos, m, (const float*)nullptr,
                       (const double*)nullptr, enough, prm.negative, prm.dense, keep);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  launch_scan_u32(s, keep, m, part, rb->tot_keep, kexcl);
  int32_t *d_kept = kept, *d_removed = removed;
  const bool kept_dev = kept != nullptr && is_device_pointer(kept);
  const bool removed_dev = removed != nullptr && is_device_pointer(removed);
  if (kept != nullptr && !kept_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_kept, size_t(m) * 4));
  if (removed != nullptr && !removed_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_removed, size_t(m) * 4));
  hipLaunchKernelGGL(outlier_emit_kernel, or_blocks(m), dim3(OR_BLOCK), 0, s, d_idx, m, keep, kexcl, d_kept, d_removed);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  (void)hipEventRecord(e1, s);
  ReadBack h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));  // counts and statistics: one copy
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t nk = h.tot_keep[0];
  if (kept != nullptr && !kept_dev && nk > 0)
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(kept, d_kept, size_t(nk) * 4, hipMemcpyDeviceToHost, s));
  if (removed != nullptr && !removed_dev && m - nk > 0)
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(removed, d_removed, size_t(m - nk) * 4, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ix->last_kernel_ms = ms;
  *n_kept = nk;
  *n_removed = m - nk;
  if (sor && stats6)
    for (int i = 0; i < 6; ++i) stats6[i] = h.stats[i];
  return PCLHIP_OK;
}

}  // namespace pclhip
