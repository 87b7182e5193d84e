// region_growing.hpp -- RegionGrowing over the index (included by radius.hip after cluster.hpp).
// Replaces pcl::RegionGrowing<PointT, NormalT>::extract (segmentation/include/pcl/segmentation/impl/region_growing.hpp
// :231-548) in smooth mode without the residual test.  The reference floods breadth-first from seeds taken in curvature
// order; here the same labels come out of an order-free restatement.  Everything below works on RANKS: the position of a
// point in the order (curvature, original index) ascending.
//   expander   a point with !(curvature > threshold) (every point when the curvature test is off): only expanders and
//              initial seeds hand their label on.  The order is by curvature: every expander precedes every non-expander
//   edge u->v  v is in u's k-NN list, v != u and !(|n_u . n_v| < c), c = cosf(theta) from the host; the dot is the float
//              sum (x x' + y y') + z z'.  The predicate is symmetric, the k-NN relation is not: the graph is directed
//   phase 1    g(v) = the lowest rank of an expander that reaches v along edges through expanders (v itself counts when it
//              is one) = the unique fixed point of g(v) = min(own rank if expander, min over edges u->v, u expander, of
//              g(u)).  v belongs to the segment seeded by the point of rank g(v)
//   phase 2    what is left (g = infinity: non-expanders) in rank order: t is CHOSEN (a seed that claims its unlabelled
//              out-neighbours and expands no further) iff no chosen t' of lower rank has an edge t'->t; otherwise t takes
//              the lowest such t'
//   numbering  segments in the rank order of their seeds, then the size filter, which keeps the order
//
// Pipeline (one stream; the read-backs: the NaN flag, one counter per round, the counts):
//   pclhip_knn               the exact lists of the indexed points (k-NN ties to the lower index)
//   rg_key_kernel            order-preserving curvature bits per original record (-0 as +0), a NaN curvature flagged; one
//                            stable radix sort of (key, original index): ties by the lower original index
//   rg_rank_kernel           rank <-> kd position, the (normal, curvature) record and the expander flag by rank
//   rg_edges_kernel          the neighbours' ranks slot-major (k x n) and a 64-bit mask of the slots that are edges; the
//                            neighbours' normals are gathered here and never again
//   rg_collapse_kernel       two expanders with edges both ways reach the same set: cl_unite (cluster.hpp) on ranks, the root
//                            is the component's lowest rank; a flatten launch; rg_trim_kernel clears the edges that stay
//                            inside a component.  An accelerator only: correctness rests on the fixed point
//   rg_propagate_kernel      rounds of atomicMin along the remaining edges out of expanders and to and from the
//                            component's root, with the shortcut lab = min(lab, lab[point ranked lab], lab[its root]) --
//                            whoever reaches a seed reaches all that seed reaches.  A round counts its changes, the host
//                            stops at zero; every label is at all times the rank of an expander that reaches the point, so
//                            a quiet round is the fixed point
//   rg_block / rg_decide     phase 2 over the compacted leftover list: an undecided point stamps its undecided out-neighbours
//                            of higher rank; an unstamped point is decided (claimed by claim[t], else chosen: it pushes its
//                            rank into claim[] of its out-neighbours).  A round decides at least the lowest undecided rank
//   rg_size / rg_mark        sizes per seed, the size filter, one scan: output numbers and CSR offsets
//   rg_label_kernel          label per original record; one stable radix sort of (label, original index) as cluster.hpp
// Both round loops are capped at n + 1 rounds (PCLHIP_ERR_STATE beyond); no loop on the device waits for another wave.
// lab[], claim[] and parent[] are read and written with relaxed agent-scope atomics inside the launches that change them
// (cluster.hpp: the L2s of the XCDs are not coherent for plain loads); values only decrease, a stale one only costs a round.
//
// Deviations from the reference: curvature ties are broken by the lower original index (its std::sort leaves them open);
// a non-finite point is in no segment (label -1; the reference makes it a segment of one); a NaN normal passes the
// smoothness test as there (NaN < c is false); a NaN curvature of an indexed point is refused.
#pragma once

#include "cluster.hpp"

namespace pclhip {
namespace {

constexpr uint32_t RG_INF = 0xFFFFFFFFu;

struct RgReadBack {
  unsigned long long unions;
  uint32_t tot[4];    // clustered points, segments kept
  uint32_t totl[4];   // leftover points
  uint32_t nan;       // an indexed point has a NaN curvature
  uint32_t indexed;   // records the index holds
  uint32_t counter;   // changes (phase 1) or decisions (phase 2) of the round under way
};

__device__ __forceinline__ uint32_t rg_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// wave sum of c into *dst (every lane of the block calls this)
__device__ __forceinline__ void rg_count(uint32_t c, uint32_t* dst) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & (WAVE - 1)) == 0 && c != 0u) atomicAdd(dst, c);
}

__global__ __launch_bounds__(OR_BLOCK) void rg_key_kernel(const char* __restrict__ normals, size_t stride,
                                                          const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                          uint32_t* __restrict__ key, uint32_t* __restrict__ nan_flag,
                                                          uint32_t* __restrict__ indexed) {
  const uint64_t id = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  uint32_t held = 0;
  if (id < n_orig) {
    uint32_t kv = RG_INF;  // a record the index does not hold: behind every indexed one
    if (rank[id] != NO_INDEX) {
      held = 1;
      float c = *reinterpret_cast<const float*>(normals + id * stride + 12);
      if (c != c) atomicOr(nan_flag, 1u);
      if (c == 0.0f) c = 0.0f;  // -0 ties with +0
      const uint32_t b = __float_as_uint(c);
      kv = (b & 0x80000000u) != 0u ? ~b : (b | 0x80000000u);
    }
    key[id] = kv;
  }
  rg_count(held, indexed);  // the records the index holds: the first that many of the sorted ids
}

__global__ __launch_bounds__(OR_BLOCK) void rg_rank_kernel(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ rank,
                                                           const char* __restrict__ normals, size_t stride, uint32_t n,
                                                           float thr, int curvature_test, uint32_t* __restrict__ rk_of_pos,
                                                           uint32_t* __restrict__ pos_of_rk, float4* __restrict__ nrm,
                                                           uint8_t* __restrict__ expander) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (r >= n) return;
  const uint32_t id = ids[r], pos = rank[id];
  rk_of_pos[pos] = r;
  pos_of_rk[r] = pos;
  const float* rec = reinterpret_cast<const float*>(normals + size_t(id) * stride);
  const float4 v = make_float4(rec[0], rec[1], rec[2], rec[3]);
  nrm[r] = v;
  expander[r] = (curvature_test == 0 || !(v.w > thr)) ? 1 : 0;
}

// lists: row `pos` = the k neighbours of the point at kd position pos as original ids (< 0: no such neighbour)
__global__ __launch_bounds__(OR_BLOCK) void rg_edges_kernel(const int32_t* __restrict__ lists, int k,
                                                            const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                            const uint32_t* __restrict__ rk_of_pos,
                                                            const uint32_t* __restrict__ pos_of_rk,
                                                            const float4* __restrict__ nrm, uint32_t n, float c,
                                                            uint32_t* __restrict__ nbr, uint64_t* __restrict__ mask) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (r >= n) return;
  const float4 nu = nrm[r];
  const int32_t* list = lists + size_t(pos_of_rk[r]) * size_t(k);
  uint64_t m = 0;
  for (int j = 0; j < k; ++j) {
    const int32_t id = list[j];
    uint32_t v = RG_INF;
    if (id >= 0 && uint64_t(id) < n_orig) {
      const uint32_t pp = rank[id];
      if (pp != NO_INDEX) v = rk_of_pos[pp];
    }
    if (v == r) v = RG_INF;
    if (v != RG_INF) {
      const float4 nv = nrm[v];
      const float d = __fadd_rn(__fadd_rn(__fmul_rn(nv.x, nu.x), __fmul_rn(nv.y, nu.y)), __fmul_rn(nv.z, nu.z));
      if (!(fabsf(d) < c)) m |= 1ull << j;
    }
    nbr[size_t(j) * n + r] = v;
  }
  mask[r] = m;
}

#ifndef PCLHIP_RG_NO_COLLAPSE  // (scripts/region_growing_timing.py builds the comparison without the pass)
// Each mutual pair of expanders is seen from both ends; the end with the higher rank does the work.
__global__ __launch_bounds__(OR_BLOCK) void rg_collapse_kernel(const uint32_t* __restrict__ nbr,
                                                               const uint64_t* __restrict__ mask,
                                                               const uint8_t* __restrict__ expander, uint32_t n,
                                                               uint32_t* parent, unsigned long long* __restrict__ unions) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  uint32_t u = 0;
  if (r < n && expander[r] != 0) {
    uint32_t root = r;
    for (uint64_t m = mask[r]; m != 0; m &= m - 1ull) {
      const uint32_t v = nbr[size_t(__builtin_ctzll(m)) * n + r];
      if (v >= r || expander[v] == 0) continue;
      bool back = false;
      for (uint64_t mv = mask[v]; mv != 0 && !back; mv &= mv - 1ull) back = nbr[size_t(__builtin_ctzll(mv)) * n + v] == r;
      if (!back) continue;
      if (cl_find(parent, v) == root) continue;
      ++u;
      root = cl_unite(parent, root, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o);
  if ((threadIdx.x & (WAVE - 1)) == 0 && u != 0u) atomicAdd(unions, (unsigned long long)u);
}

#endif

// after the flatten launch: the edges inside a component go, the labels start at the component's root
__global__ __launch_bounds__(OR_BLOCK) void rg_trim_kernel(const uint32_t* __restrict__ nbr, uint64_t* __restrict__ mask,
                                                           const uint8_t* __restrict__ expander,
                                                           const uint32_t* __restrict__ comp, uint32_t n,
                                                           uint32_t* __restrict__ lab) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (r >= n) return;
  if (expander[r] == 0) {
    lab[r] = RG_INF;
    return;
  }
  const uint32_t c = comp[r];
  const uint64_t m0 = mask[r];
  uint64_t m1 = m0;
  for (uint64_t m = m0; m != 0; m &= m - 1ull) {
    const int j = __builtin_ctzll(m);
    const uint32_t v = nbr[size_t(j) * n + r];
    if (expander[v] != 0 && comp[v] == c) m1 &= ~(1ull << j);
  }
  if (m1 != m0) mask[r] = m1;
  lab[r] = c;
}

// waves per SIMD (kernel-resource-usage, gfx950): see DESIGN.md row f-16
__global__ __launch_bounds__(OR_BLOCK) void rg_propagate_kernel(const uint32_t* __restrict__ nbr,
                                                                const uint64_t* __restrict__ mask,
                                                                const uint8_t* __restrict__ expander,
                                                                const uint32_t* __restrict__ comp, uint32_t n, uint32_t* lab,
                                                                uint32_t* changes) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  uint32_t ch = 0;
  if (r < n && expander[r] != 0) {
    const uint32_t c = comp[r];
    const uint32_t lu = cl_load(lab, r);
    uint32_t m = rg_min(lu, cl_load(lab, c));
    m = rg_min(m, cl_load(lab, comp[m]));  // every label here is the rank of an expander that reaches r
    m = rg_min(m, cl_load(lab, m));
    if (m < lu) {
      atomicMin(lab + r, m);
      ++ch;
    }
    if (c != r && cl_load(lab, c) > m && atomicMin(lab + c, m) > m) ++ch;
    for (uint64_t e = mask[r]; e != 0; e &= e - 1ull) {
      const uint32_t v = nbr[size_t(__builtin_ctzll(e)) * n + r];
      if (cl_load(lab, v) > m && atomicMin(lab + v, m) > m) ++ch;
    }
  }
  rg_count(ch, changes);
}

__global__ __launch_bounds__(OR_BLOCK) void rg_left_kernel(const uint32_t* __restrict__ lab, uint32_t n,
                                                           uint32_t* __restrict__ flag) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (r < n) flag[r] = lab[r] == RG_INF ? 1u : 0u;
}

// phase 2, first half of a round: no label changes in this launch
__global__ __launch_bounds__(OR_BLOCK) void rg_block_kernel(const uint32_t* __restrict__ list, uint32_t n_left,
                                                            const uint32_t* __restrict__ nbr,
                                                            const uint64_t* __restrict__ mask, uint32_t n,
                                                            const uint32_t* __restrict__ lab, uint32_t* __restrict__ stamp,
                                                            uint32_t round) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (i >= n_left) return;
  const uint32_t t = list[i];
  if (lab[t] != RG_INF) return;
  for (uint64_t e = mask[t]; e != 0; e &= e - 1ull) {
    const uint32_t v = nbr[size_t(__builtin_ctzll(e)) * n + t];
    if (v > t && lab[v] == RG_INF) stamp[v] = round;  // (every writer of a slot writes the same value)
  }
}

// ... second half: a point nobody stamped has no undecided in-neighbour of lower rank left.  An out-neighbour of higher
// rank of a point decided here was stamped by it in the first half, so it is not decided in this launch: its label stays
// RG_INF and its claim is read in a later launch only.
__global__ __launch_bounds__(OR_BLOCK) void rg_decide_kernel(const uint32_t* __restrict__ list, uint32_t n_left,
                                                             const uint32_t* __restrict__ nbr,
                                                             const uint64_t* __restrict__ mask, uint32_t n, uint32_t* lab,
                                                             const uint32_t* __restrict__ stamp, uint32_t* claim,
                                                             uint32_t round, uint32_t* decided) {
  const uint32_t i = blockIdx.x * OR_BLOCK + threadIdx.x;
  uint32_t d = 0;
  if (i < n_left) {
    const uint32_t t = list[i];
    if (cl_load(lab, t) == RG_INF && stamp[t] != round) {
      const uint32_t c = cl_load(claim, t);
      d = 1;
      if (c != RG_INF) {
        cl_store(lab, t, c);
      } else {
        cl_store(lab, t, t);
        for (uint64_t e = mask[t]; e != 0; e &= e - 1ull) {
          const uint32_t v = nbr[size_t(__builtin_ctzll(e)) * n + t];
          if (v > t && cl_load(lab, v) == RG_INF) atomicMin(claim + v, t);
        }
      }
    }
  }
  rg_count(d, decided);
}

__global__ __launch_bounds__(OR_BLOCK) void rg_size_kernel(const uint32_t* __restrict__ lab, uint32_t n, uint32_t* size) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (r >= n) return;
  const uint32_t seed = lab[r];
  if (seed < n) atomicAdd(size + seed, 1u);  // (every point has a seed once both loops have ended)
}

__global__ __launch_bounds__(OR_BLOCK) void rg_mark_kernel(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ size,
                                                           uint32_t n, uint32_t min_size, uint32_t max_size,
                                                           uint32_t* __restrict__ a) {
  const uint32_t r = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (r >= n) return;
  const uint32_t sz = size[r];
  a[r] = (lab[r] == r && sz >= min_size && sz <= max_size) ? sz : 0u;
}

// label of every original record and the key of the last sort (k for a record in no segment: behind every segment)
__global__ __launch_bounds__(OR_BLOCK) void rg_label_kernel(const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                            const uint32_t* __restrict__ rk_of_pos,
                                                            const uint32_t* __restrict__ lab, const uint32_t* __restrict__ a,
                                                            const uint32_t* __restrict__ cid, uint32_t n, uint32_t k,
                                                            int32_t* __restrict__ labels, uint32_t* __restrict__ key) {
  const uint64_t id = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  if (id >= n_orig) return;
  const uint32_t pos = rank[id];
  int32_t l = -1;
  if (pos != NO_INDEX) {
    const uint32_t seed = lab[rk_of_pos[pos]];
    if (seed < n && a[seed] != 0u) l = int32_t(cid[seed]);
  }
  if (labels) labels[id] = l;
  if (key) key[id] = l < 0 ? k : uint32_t(l);
}

}  // namespace

// The host side of pclhip_region_growing (api.hip): the parameters are validated there, `normals` is on the device.
pclhip_status region_growing(pclhip_index* ix, const void* normals, size_t stride, int k, float cos_theta, float curv_thr,
                             int curvature_test, uint32_t min_size, uint32_t max_size, int32_t* out_labels,
                             uint64_t* out_offsets, uint64_t offsets_capacity, int32_t* out_indices, uint64_t indices_capacity,
                             uint64_t* n_clusters, uint64_t* n_clustered) {
  pclhip_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = ix->n;
  const uint64_t n_orig = ix->n_orig;
  *n_clusters = 0;
  *n_clustered = 0;
  ix->rg_ms[0] = ix->rg_ms[1] = ix->rg_ms[2] = ix->rg_ms[3] = 0.0;
  ix->rg_rounds[0] = ix->rg_rounds[1] = 0;
  ix->rg_unions = 0;
  ix->rg_leftover = 0;
  PCLHIP_REQUIRE(ctx, n_orig < 0x7FFFFFFFull, "too many records");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  const bool labels_dev = out_labels != nullptr && is_device_pointer(out_labels);
  if (n == 0 || k == 0) {  // nothing is indexed, or no neighbours (region_growing.hpp:303-304): no segment
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
        set_error(ctx, "region growing: out_offsets holds fewer than n_clusters + 1 entries");
        return PCLHIP_ERR_OVERFLOW;
      }
      out_offsets[0] = 0;
    }
    return PCLHIP_OK;
  }
  DeviceScope scope(ctx);
  const char* dn = static_cast<const char*>(normals);
  RgReadBack* rb = nullptr;
  uint32_t *key0 = nullptr, *key1 = nullptr, *val0 = nullptr, *val1 = nullptr;
  uint32_t *rk_of_pos = nullptr, *pos_of_rk = nullptr, *nbr = nullptr, *parent = nullptr, *lab = nullptr;
  uint32_t *a = nullptr, *b = nullptr, *c = nullptr;  // three scratch arrays of n + 1 words
  float4* nrm = nullptr;
  uint8_t* expander = nullptr;
  uint64_t* mask = nullptr;
  uint2* part = nullptr;
  int32_t* lists = nullptr;
  float* d2 = nullptr;
  const uint64_t big = n_orig > n ? n_orig : uint64_t(n);
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rb, sizeof(RgReadBack)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&key0, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&key1, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&val0, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&val1, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rk_of_pos, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&pos_of_rk, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&nbr, size_t(n) * size_t(k) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&parent, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&lab, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&a, (size_t(n) + 1) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&b, (size_t(n) + 1) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&c, (size_t(n) + 1) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&nrm, size_t(n) * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&expander, size_t(n)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&mask, size_t(n) * 8));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((big + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&lists, size_t(n) * size_t(k) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&d2, size_t(n) * size_t(k) * 4));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(rb, 0, sizeof(RgReadBack), s));
  hipEvent_t ev[8] = {};
  for (hipEvent_t& e : ev) PCLHIP_CHECK_HIP(ctx, scope.event(&e));
  (void)hipEventRecord(ev[0], s);
  {
    // the library's own k-NN path over the index's points in kd order (the caller holds the context's recursive lock)
    const pclhip_status st = pclhip_knn(ix, ix->pts, sizeof(float4), n, k, lists, d2);
    if (st != PCLHIP_OK) return st;
  }
  (void)hipEventRecord(ev[1], s);
  // rank
  hipLaunchKernelGGL(rg_key_kernel, or_blocks(n_orig), dim3(OR_BLOCK), 0, s, dn, stride, ix->rank, n_orig, key0, &rb->nan,
                     &rb->indexed);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  uint32_t *ks = nullptr, *ids = nullptr;
  {
    const pclhip_status st = radix_sort_pairs(ctx, key0, val0, key1, val1, uint32_t(n_orig), 32, true, &ks, &ids);
    if (st != PCLHIP_OK) return st;
  }
  RgReadBack h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  if (h.indexed != n) {  // (the ranks below are positions among the distinct indexed records)
    set_error(ctx, "region growing needs an index that holds every record once (no repeated indices)");
    return PCLHIP_ERR_STATE;
  }
  PCLHIP_REQUIRE(ctx, h.nan == 0, "region growing: a NaN curvature has no place in the seed order");
  hipLaunchKernelGGL(rg_rank_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, ids, ix->rank, dn, stride, n, curv_thr,
                     curvature_test, rk_of_pos, pos_of_rk, nrm, expander);
  hipLaunchKernelGGL(rg_edges_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, lists, k, ix->rank, n_orig, rk_of_pos, pos_of_rk, nrm,
                     n, cos_theta, nbr, mask);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  // collapse
  (void)hipEventRecord(ev[2], s);
  hipLaunchKernelGGL(cluster_init_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, parent, n);
#ifndef PCLHIP_RG_NO_COLLAPSE
  hipLaunchKernelGGL(rg_collapse_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, nbr, mask, expander, n, parent, &rb->unions);
  hipLaunchKernelGGL(cluster_flatten_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, parent, n);
#endif
  hipLaunchKernelGGL(rg_trim_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, nbr, mask, expander, parent, n, lab);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  (void)hipEventRecord(ev[3], s);
  // phase 1
  uint32_t rounds1 = 0;
  for (;;) {
    if (rounds1 > n) {
      set_error(ctx, "region growing: the propagation did not settle within n + 1 rounds");
      return PCLHIP_ERR_STATE;
    }
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(&rb->counter, 0, 4, s));
    hipLaunchKernelGGL(rg_propagate_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, nbr, mask, expander, parent, n, lab,
                       &rb->counter);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    uint32_t changes = 0;
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&changes, &rb->counter, 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    ++rounds1;
    if (changes == 0) break;
  }
  (void)hipEventRecord(ev[4], s);
  // phase 2: a = the leftover flags, b = their scan and then the stamps, c = the list; the claims live in parent[]
  uint32_t* claim = parent;
  hipLaunchKernelGGL(rg_left_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, lab, n, a);
  launch_scan_u32(s, a, n, part, rb->totl, b);
  hipLaunchKernelGGL(outlier_compact_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, a, b, n, c);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t n_left = h.totl[0];
  uint32_t rounds2 = 0;
  if (n_left > 0) {
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(b, 0, size_t(n) * 4, s));
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(claim, 0xFF, size_t(n) * 4, s));
    uint32_t undecided = n_left;
    while (undecided > 0) {
      if (rounds2 > n) {
        set_error(ctx, "region growing: the leftover points were not decided within n + 1 rounds");
        return PCLHIP_ERR_STATE;
      }
      ++rounds2;
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(&rb->counter, 0, 4, s));
      hipLaunchKernelGGL(rg_block_kernel, or_blocks(n_left), dim3(OR_BLOCK), 0, s, c, n_left, nbr, mask, n, lab, b, rounds2);
      hipLaunchKernelGGL(rg_decide_kernel, or_blocks(n_left), dim3(OR_BLOCK), 0, s, c, n_left, nbr, mask, n, lab, b, claim,
                         rounds2, &rb->counter);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
      uint32_t decided = 0;
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&decided, &rb->counter, 4, hipMemcpyDeviceToHost, s));
      PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
      if (decided == 0 || decided > undecided) {
        set_error(ctx, "region growing: a leftover round decided nothing");
        return PCLHIP_ERR_STATE;
      }
      undecided -= decided;
    }
  }
  (void)hipEventRecord(ev[5], s);
  // output: a = the kept sizes by seed, b = the sizes and then the CSR offsets, c = the output number by seed
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(b, 0, (size_t(n) + 1) * 4, s));
  hipLaunchKernelGGL(rg_size_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, lab, n, b);
  hipLaunchKernelGGL(rg_mark_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, lab, b, n, min_size, max_size, a);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  uint32_t* roff = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&roff, (size_t(n) + 1) * 4));
  launch_scan_u32(s, a, n, part, rb->tot, nullptr, c, roff);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  const uint32_t nc = h.tot[0], kk = h.tot[1];
  *n_clusters = kk;
  *n_clustered = nc;
  ix->rg_unions = h.unions;
  ix->rg_rounds[0] = rounds1;
  ix->rg_rounds[1] = rounds2;
  ix->rg_leftover = n_left;
  int32_t* d_labels = out_labels;
  if (out_labels != nullptr && !labels_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_labels, size_t(n_orig) * 4));
  const bool want_indices = out_indices != nullptr && kk > 0;
  uint32_t* sorted_ids = nullptr;
  if (d_labels != nullptr || want_indices) {
    hipLaunchKernelGGL(rg_label_kernel, or_blocks(n_orig), dim3(OR_BLOCK), 0, s, ix->rank, n_orig, rk_of_pos, lab, a, c, n, kk,
                       d_labels, want_indices ? key0 : nullptr);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  if (want_indices) {
    uint32_t* ks2 = nullptr;
    const pclhip_status st =
        radix_sort_pairs(ctx, key0, val0, key1, val1, uint32_t(n_orig), cluster_bits(uint64_t(kk) + 1), true, &ks2, &sorted_ids);
    if (st != PCLHIP_OK) return st;
  }
  (void)hipEventRecord(ev[6], s);
  if (out_labels != nullptr && !labels_dev)
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_labels, d_labels, size_t(n_orig) * 4, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, ev[0], ev[6]) == hipSuccess) ix->last_kernel_ms = ms;
  if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ix->rg_ms[0] = ms;
  if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) ix->rg_ms[1] = ms;
  if (hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) ix->rg_ms[2] = ms;
  if (hipEventElapsedTime(&ms, ev[4], ev[5]) == hipSuccess) ix->rg_ms[3] = ms;
  // the counts and the labels are written: what does not fit is an error from here on
  if (out_offsets != nullptr && offsets_capacity < uint64_t(kk) + 1) {
    set_error(ctx, "region growing: out_offsets holds fewer than n_clusters + 1 entries");
    return PCLHIP_ERR_OVERFLOW;
  }
  if (out_indices != nullptr && indices_capacity < nc) {
    set_error(ctx, "region growing: out_indices holds fewer than n_clustered entries");
    return PCLHIP_ERR_OVERFLOW;
  }
  if (out_offsets != nullptr) {
    std::vector<uint32_t> off(size_t(kk) + 1);
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(off.data(), roff, (size_t(kk) + 1) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    for (uint32_t r = 0; r <= kk; ++r) out_offsets[r] = off[r];
    out_offsets[kk] = nc;
  }
  if (want_indices && nc > 0) {
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_indices, sorted_ids, size_t(nc) * 4,
                                         is_device_pointer(out_indices) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  }
  return PCLHIP_OK;
}

}  // namespace pclhip
