// cluster.hpp -- EuclideanClusterExtraction over the index (included by radius.hip).
// Replaces the breadth-first flood of pcl::extractEuclideanClusters (segmentation/include/pcl/segmentation/impl/
// extract_clusters.hpp:124-217) and the ordering of EuclideanClusterExtraction<PointT>::extract (:223-253).  The clusters are
// the connected components of the graph with an edge wherever float d2 < float(r * r), r = double(float(tolerance)) -- the
// relation of pclhip_radius_search, symmetric because the squares do not see the sign of the differences.  No neighbour
// is ever stored: every hit of the radius walk becomes one union of a concurrent union-find over kd positions.
//
// Pipeline (one stream, one read-back: the two counts):
//   cluster_init_kernel     parent[pos] = pos
//   cluster_hook_kernel     traverse<ClusterHook, true> with the fixed bound t (strict: traverse.hpp's leaf_hits_lt), one lane
//                           per indexed point (for_each_query_group); a hit at position j < own position i unites i and j: both roots by path halving, the larger root hooked under the smaller by compare-and-swap
//   cluster_flatten_kernel  (a launch of its own: the kernel boundary is what makes the hooks visible) parent[pos] = root(pos)
//                           = the smallest kd position of the component, whatever the interleaving of the hook launch was
//   cluster_count_kernel    per root: size (atomicAdd) and smallest original index (atomicMin): integers, order-free
//   cluster_mark_kernel     a[pos] = size of a root inside [min, max], else 0; one scan (device_scan.hpp) gives the number
//                           of clusters, the number of clustered points and a dense id per kept root
//   cluster_keys_kernel     dense id -> (smallest original index, n - size); two stable radix sorts (voxelgrid.hip's passes
//                           through radix_sort_pairs) order the clusters by size descending, ties by smallest original index
//   cluster_rank_kernel     dense id -> rank in that order, the sizes in that order; their scan = the CSR offsets
//   cluster_label_kernel    a label per original record (-1: in no returned cluster) and its sort key
//   one more stable radix sort of (label, original index) in original-index order: every cluster's indices come out
//   ascending, side by side in rank order.  No output position is an atomic ticket.
#pragma once

#include "device_scan.hpp"
#include "outlier.hpp"  // OR_BLOCK, OR_WAVES, outlier_grid, or_blocks
#include "traverse.hpp"

namespace pclhip {
namespace {

// Every access to parent[] inside the hook launch (and the flatten launch, whose threads read slots other threads write)
// is a relaxed agent-scope atomic: the per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's
// stores, so a plain load could keep following a line that went stale many hooks ago.  No fence and no ordering is needed:
// parent[x] <= x always, with equality exactly at a root, and a slot only ever changes to a smaller position of the same
// tree -- so a stale or halved pointer still names an ancestor in the same tree, every find walks strictly downwards and
// ends at a position that was a root when it was read, no payload is handed over between waves, and the only access that
// decides anything is the compare-and-swap on a root's own slot, which fails when the slot is no longer what the find saw.
__device__ __forceinline__ uint32_t cl_load(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cl_store(uint32_t* parent, uint32_t x, uint32_t v) {
  __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving (x -> its grandparent at every step).  Ends: positions decrease strictly.
__device__ __forceinline__ uint32_t cl_find(uint32_t* parent, uint32_t x) {
  uint32_t p = cl_load(parent, x);
  while (p != x) {
    const uint32_t g = cl_load(parent, p);
    if (g == p) return p;
    cl_store(parent, x, g);  // x was not a root when read and never becomes one again: this store races with no hook
    x = g;
    p = cl_load(parent, x);
  }
  return x;
}

// root of x without writes (the flatten launch)
__device__ __forceinline__ uint32_t cl_root(const uint32_t* parent, uint32_t x) {
  uint32_t p = cl_load(parent, x);
  while (p != x) {
    x = p;
    p = cl_load(parent, x);
  }
  return x;
}

// unite the trees of the roots-to-be a and b; returns the root of the united tree as this lane last saw it.  Lock-free: a
// compare-and-swap is lost only to another lane's successful hook of the same root, and is retried from the new roots.
__device__ __forceinline__ uint32_t cl_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cl_find(parent, a);
    b = cl_find(parent, b);
    if (a == b) return a;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    uint32_t expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return lo;
  }
}

// Each edge is seen from both ends; the end with the larger position does the work.  A leaf that starts above the lane's
// own position holds no lower neighbour and is not even tested; padding slots lie above every real position.
struct ClusterHook {
  float t;
  uint32_t self;    // the lane's own position
  uint32_t root;    // its root as last seen: a neighbour found under the same root needs no union
  uint32_t unions;  // unions attempted
  uint32_t* parent;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return t; }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id == NO_INDEX) return;
    const uint32_t base = leaf_id * uint32_t(LEAF);
    if (base >= self) return;
    const float4* s = reinterpret_cast<const float4*>(buf) + slot;  // transposed staging
    uint32_t mask = leaf_hits_lt<16>(s, qx[0], qy[0], qz[0], t);
    if (self - base < uint32_t(LEAF)) mask &= (1u << (self - base)) - 1u;  // the own leaf: the slots below the lane's
    while (mask != 0) {
      const uint32_t j = base + uint32_t(__builtin_ctz(mask));
      mask &= mask - 1u;
      const uint32_t rj = cl_find(parent, j);
      if (rj == root) continue;
      ++unions;
      root = cl_unite(parent, root, rj);
    }
  }
};

__global__ __launch_bounds__(OR_BLOCK) void cluster_init_kernel(uint32_t* __restrict__ parent, uint32_t n) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i < n) parent[i] = i;
}

// One lane per indexed point (for_each_query_group).  The own leaf is not evaluated ahead of the walk as
// ror_count_kernel does: the bound is fixed, so nothing is gained for the walk and the union code would exist twice -- the
// own leaf only names the node the walk starts under, as in fpfh_spfh_kernel.
// No wave waits for another: every loop is a find (ends at a root), a retry of a lost compare-and-swap, or the walk.
// waves per SIMD (kernel-resource-usage, gfx950): see DESIGN.md row f-10
__global__ __launch_bounds__(OR_BLOCK) void cluster_hook_kernel(IndexView ix, float t, uint32_t* parent,
                                                                unsigned long long* __restrict__ unions) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  const int lane = threadIdx.x & (WAVE - 1);
  TraverseStats ts;
  ClusterHook pol;
  pol.t = t;
  pol.parent = parent;
  pol.unions = 0;
  for_each_query_group(ix, nullptr, ix.n, [&](uint32_t pos, bool real, float4 p) {
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {real};
    pol.self = pos;  // (0 for a lane without a point: position 0 has no lower neighbour, such a lane tests nothing)
    pol.root = pol.self;
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a point
    traverse<ClusterHook, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
  });
  uint32_t u = pol.unions;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o);
  if (lane == 0 && u != 0u) atomicAdd(unions, (unsigned long long)u);
}

__global__ __launch_bounds__(OR_BLOCK) void cluster_flatten_kernel(uint32_t* parent, uint32_t n) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i < n) cl_store(parent, i, cl_root(parent, i));
}

// size[root] and minid[root] (the smallest original index) of every component.  Neighbours in kd order mostly share a
// root, and one atomic per point on the root of a 10M-point component took 6.2 ms (the measurement in DESIGN.md row f-10):
// a thread folds CL_PER consecutive positions into runs of equal roots and sends a run when the root changes; its last
// run is merged with the equal roots of its wave (four rounds: a leader's root, the peers' count and minimum by a
// butterfly, one pair of atomics from the leader); what is left after that sends its own.  Integer sums and minima: the
// result does not depend on any of this.
constexpr int CL_PER = 16;
__global__ __launch_bounds__(OR_BLOCK) void cluster_count_kernel(const uint32_t* __restrict__ parent,
                                                                 const float4* __restrict__ pts, uint32_t n,
                                                                 uint32_t* size, uint32_t* minid) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint64_t base = (uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x) * CL_PER;
  uint32_t r = NO_INDEX, cnt = 0, mn = 0xFFFFFFFFu;  // (no root is NO_INDEX: the first position opens a run)
  for (int e = 0; e < CL_PER; ++e) {
    const uint64_t i = base + e;
    if (i >= n) break;
    const uint32_t ri = parent[i], id = __float_as_uint(pts[i].w);
    if (ri != r) {
      if (cnt != 0u) {
        atomicAdd(size + r, cnt);
        atomicMin(minid + r, mn);
      }
      r = ri;
      cnt = 0u;
      mn = 0xFFFFFFFFu;
    }
    ++cnt;
    mn = id < mn ? id : mn;
  }
  bool todo = cnt != 0u;
  for (int round = 0; round < 4; ++round) {
    const unsigned long long open = __builtin_amdgcn_ballot_w64(todo);
    if (open == 0ull) break;
    const int leader = __builtin_ctzll(open);
    const uint32_t lr = __shfl(r, leader);
    const bool mine = todo && r == lr;
    uint32_t c = mine ? cnt : 0u, m = mine ? mn : 0xFFFFFFFFu;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      c += __shfl_xor(c, o);
      const uint32_t x = __shfl_xor(m, o);
      m = x < m ? x : m;
    }
    if (lane == leader) {
      atomicAdd(size + lr, c);
      atomicMin(minid + lr, m);
    }
    if (mine) todo = false;
  }
  if (todo) {
    atomicAdd(size + r, cnt);
    atomicMin(minid + r, mn);
  }
}

__global__ __launch_bounds__(OR_BLOCK) void cluster_mark_kernel(const uint32_t* __restrict__ parent,
                                                                const uint32_t* __restrict__ size, uint32_t n,
                                                                uint32_t min_size, uint32_t max_size,
                                                                uint32_t* __restrict__ a) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t sz = size[i];
  a[i] = (parent[i] == i && sz >= min_size && sz <= max_size) ? sz : 0u;
}

// kept root -> its dense id c (the exclusive count of kept roots below it): kmin[c] = smallest original index, kinv[c] = n - size
__global__ __launch_bounds__(OR_BLOCK) void cluster_keys_kernel(const uint32_t* __restrict__ a,
                                                                const uint32_t* __restrict__ cid,
                                                                const uint32_t* __restrict__ minid, uint32_t n,
                                                                uint32_t* __restrict__ kmin, uint32_t* __restrict__ kinv) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i >= n || a[i] == 0u) return;
  const uint32_t c = cid[i];
  kmin[c] = minid[i];
  kinv[c] = n - a[i];
}

// keys of the second sort, in the order the first one left: key[i] = kinv[val[i]]
__global__ __launch_bounds__(OR_BLOCK) void cluster_gather_kernel(const uint32_t* __restrict__ val,
                                                                  const uint32_t* __restrict__ kinv, uint32_t k,
                                                                  uint32_t* __restrict__ key) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i < k) key[i] = kinv[val[i]];
}

// order[r] = dense id of the cluster of rank r (keys[r] = n - its size) -> crank[dense id] = r, rsize[r]
__global__ __launch_bounds__(OR_BLOCK) void cluster_rank_kernel(const uint32_t* __restrict__ order,
                                                                const uint32_t* __restrict__ keys, uint32_t k, uint32_t n,
                                                                uint32_t* __restrict__ crank, uint32_t* __restrict__ rsize) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (r >= k) return;
  crank[order[r]] = r;
  rsize[r] = n - keys[r];
}

// label of every original record and the key of the last sort (k for a record in no cluster: behind every cluster)
__global__ __launch_bounds__(OR_BLOCK) void cluster_label_kernel(const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                                 const uint32_t* __restrict__ parent,
                                                                 const uint32_t* __restrict__ a,
                                                                 const uint32_t* __restrict__ cid,
                                                                 const uint32_t* __restrict__ crank, uint32_t k,
                                                                 int32_t* __restrict__ labels, uint32_t* __restrict__ key) {
  const uint64_t id = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  if (id >= n_orig) return;
  const uint32_t pos = rank[id];
  int32_t lab = -1;
  if (pos != NO_INDEX) {
    const uint32_t root = parent[pos];
    if (a[root] != 0u) lab = int32_t(crank[cid[root]]);
  }
  if (labels) labels[id] = lab;
  if (key) key[id] = lab < 0 ? k : uint32_t(lab);
}

inline int cluster_bits(uint64_t values) {  // bits that tell `values` keys 0 .. values - 1 apart (at least 1)
  int b = 1;
  while (b < 32 && (uint64_t(1) << b) < values) ++b;
  return b;
}

}  // namespace

// The host side of pclhip_euclidean_clusters (api.hip).  t = float(r * r), validated there.
pclhip_status euclidean_clusters(pclhip_index* ix, float t, uint32_t min_size, uint32_t max_size, int32_t* out_labels,
                                 uint64_t* out_offsets, uint64_t offsets_capacity, int32_t* out_indices,
                                 uint64_t indices_capacity, uint64_t* n_clusters, uint64_t* n_clustered) {
  pclhip_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = ix->n;
  const uint64_t n_orig = ix->n_orig;
  *n_clusters = 0;
  *n_clustered = 0;
  ix->cluster_ms[0] = ix->cluster_ms[1] = 0.0;
  ix->cluster_unions = 0;
  PCLHIP_REQUIRE(ctx, n_orig < 0x7FFFFFFFull, "too many records");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const bool labels_dev = out_labels != nullptr && is_device_pointer(out_labels);
  if (n == 0) {  // nothing is indexed: every record is in no cluster
    if (out_labels != nullptr && n_orig > 0) {
      if (labels_dev) {
        PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(out_labels, 0xFF, size_t(n_orig) * 4, s));
        PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
      } else {
        std::fill(out_labels, out_labels + n_orig, int32_t(-1));
      }
    }
    ix->last_kernel_ms = 0.0;
    if (out_offsets != nullptr) {
      if (offsets_capacity < 1) {
        set_error(ctx, "euclidean clusters: out_offsets holds fewer than n_clusters + 1 entries");
        return PCLHIP_ERR_OVERFLOW;
      }
      out_offsets[0] = 0;
    }
    return PCLHIP_OK;
  }
  DeviceScope scope(ctx);
  struct ReadBack {
    unsigned long long unions;
    uint32_t tot[4];   // clustered points, clusters, largest kept size
    uint32_t tot2[4];  // (the scan of the sizes in rank order)
  };
  ReadBack* rb = nullptr;
  uint32_t *parent = nullptr, *size = nullptr, *minid = nullptr, *a = nullptr, *cid = nullptr;
  uint2* part = nullptr;
  const uint64_t big = n_orig > n ? n_orig : uint64_t(n);
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rb, sizeof(ReadBack)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&parent, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&size, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&minid, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&a, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&cid, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((big + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(rb, 0, sizeof(ReadBack), s));
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr, e4 = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.event(&e0));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e1));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e2));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e3));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e4));
  (void)hipEventRecord(e0, s);
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(size, 0, size_t(n) * 4, s));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(minid, 0xFF, size_t(n) * 4, s));
  hipLaunchKernelGGL(cluster_init_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, parent, n);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  const IndexView v = ix->view();
  (void)hipEventRecord(e1, s);
  if (t > 0.0f) {  // (t == 0: nothing lies within d2 < 0, every point stays its own root -- extract_clusters.hpp:177-181)
    PCLHIP_LAUNCH_FED(ctx, cluster_hook_kernel, dim3(outlier_grid(ctx, cluster_hook_kernel, n)), dim3(OR_BLOCK), 0, s, v, t,
                      parent, &rb->unions);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  (void)hipEventRecord(e2, s);
  hipLaunchKernelGGL(cluster_flatten_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, parent, n);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  (void)hipEventRecord(e3, s);
  hipLaunchKernelGGL(cluster_count_kernel, or_blocks((uint64_t(n) + CL_PER - 1) / CL_PER), dim3(OR_BLOCK), 0, s, parent, ix->pts,
                     n, size, minid);
  hipLaunchKernelGGL(cluster_mark_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, parent, size, n, min_size, max_size, a);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  launch_scan_u32(s, a, n, part, rb->tot, nullptr, cid);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  ReadBack h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));  // the call's one read-back
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t nc = h.tot[0], k = h.tot[1];
  *n_clusters = k;
  *n_clustered = nc;
  ix->cluster_unions = h.unions;

  // the clusters in output order
  uint32_t *crank = nullptr, *rsize = nullptr, *roff = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&crank, size_t(k) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rsize, size_t(k) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&roff, size_t(k) * 4));
  if (k > 0) {
    uint32_t *kmin = nullptr, *kinv = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr, *k2 = nullptr;
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&kmin, size_t(k) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&kinv, size_t(k) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&k1, size_t(k) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&k2, size_t(k) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&v0, size_t(k) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&v1, size_t(k) * 4));
    hipLaunchKernelGGL(cluster_keys_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, a, cid, minid, n, kmin, kinv);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    // ties first: by smallest original index (values = the dense ids); then, stable, by n - size
    uint32_t *ks = nullptr, *vs = nullptr;
    pclhip_status st = radix_sort_pairs(ctx, kmin, v0, k1, v1, k, cluster_bits(n_orig), true, &ks, &vs);
    if (st != PCLHIP_OK) return st;
    uint32_t* vother = vs == v0 ? v1 : v0;
    hipLaunchKernelGGL(cluster_gather_kernel, or_blocks(k), dim3(OR_BLOCK), 0, s, vs, kinv, k, k2);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    uint32_t *ks2 = nullptr, *vs2 = nullptr;
    st = radix_sort_pairs(ctx, k2, vs, k1, vother, k, cluster_bits(n), false, &ks2, &vs2);
    if (st != PCLHIP_OK) return st;
    hipLaunchKernelGGL(cluster_rank_kernel, or_blocks(k), dim3(OR_BLOCK), 0, s, vs2, ks2, k, n, crank, rsize);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    launch_scan_u32(s, rsize, k, part, rb->tot2, roff);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  // labels, and the records sorted by label
  int32_t* d_labels = out_labels;
  if (out_labels != nullptr && !labels_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_labels, size_t(n_orig) * 4));
  const bool want_indices = out_indices != nullptr && k > 0;
  uint32_t *lk0 = nullptr, *lk1 = nullptr, *lv0 = nullptr, *lv1 = nullptr, *sorted_ids = nullptr;
  if (want_indices) {
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&lk0, size_t(n_orig) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&lk1, size_t(n_orig) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&lv0, size_t(n_orig) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&lv1, size_t(n_orig) * 4));
  }
  if (d_labels != nullptr || want_indices) {
    hipLaunchKernelGGL(cluster_label_kernel, or_blocks(n_orig), dim3(OR_BLOCK), 0, s, ix->rank, n_orig, parent, a, cid, crank,
                       k, d_labels, lk0);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  if (want_indices) {
    uint32_t* ks = nullptr;
    const pclhip_status st =
        radix_sort_pairs(ctx, lk0, lv0, lk1, lv1, uint32_t(n_orig), cluster_bits(uint64_t(k) + 1), true, &ks, &sorted_ids);
    if (st != PCLHIP_OK) return st;
  }
  (void)hipEventRecord(e4, s);
  if (out_labels != nullptr && !labels_dev)
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_labels, d_labels, size_t(n_orig) * 4, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, e0, e4) == hipSuccess) ix->last_kernel_ms = ms;
  if (hipEventElapsedTime(&ms, e1, e2) == hipSuccess) ix->cluster_ms[0] = ms;
  if (hipEventElapsedTime(&ms, e2, e3) == hipSuccess) ix->cluster_ms[1] = ms;
  // the counts and the labels are written: what does not fit is an error from here on
  if (out_offsets != nullptr && offsets_capacity < uint64_t(k) + 1) {
    set_error(ctx, "euclidean clusters: out_offsets holds fewer than n_clusters + 1 entries");
    return PCLHIP_ERR_OVERFLOW;
  }
  if (out_indices != nullptr && indices_capacity < nc) {
    set_error(ctx, "euclidean clusters: out_indices holds fewer than n_clustered entries");
    return PCLHIP_ERR_OVERFLOW;
  }
  if (out_offsets != nullptr) {
    std::vector<uint32_t> off(k);
    if (k > 0) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(off.data(), roff, size_t(k) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    for (uint32_t r = 0; r < k; ++r) out_offsets[r] = off[r];
    out_offsets[k] = nc;
  }
  if (want_indices && nc > 0) {
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_indices, sorted_ids, size_t(nc) * 4,
                                         is_device_pointer(out_indices) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  }
  return PCLHIP_OK;
}

}  // namespace pclhip
