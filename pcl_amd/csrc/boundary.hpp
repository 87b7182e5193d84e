// boundary.hpp -- BoundaryEstimation over the index (included by radius.hip).
// Replaces pcl::BoundaryEstimation<PointInT, PointNT, PointOutT>::isBoundaryPoint and ::computeFeature
// (features/include/pcl/features/impl/boundary.hpp:87-137, 141-209; the basis: boundary.h:161-168): search surface ==
// input.  Per query q with normal n:
//   1. the neighbourhood: every indexed point with float d2 < float(r * r), q included (the relation of
//      pclhip_radius_search), or the k nearest; fewer than max(3, min_neighbors) entries: flag 0
//   2. v = unitOrthogonal of the 4-vector (nx, ny, nz, 0) by Eigen's generic rule (bnd_basis), u = n x v, in float
//   3. per neighbour p: delta = p - q in float; an all-zero delta is skipped; angle = atan2f(v . delta, u . delta); no angle
//      left: flag 0
//   4. flag = (the largest difference of consecutive sorted angles, 2 * float(pi) - last + first included) > threshold
// The reference sorts the angles.  Here nothing is sorted and no list is kept: the flag only needs "is some gap > thr".
//
// Pipeline (one stream; the read-backs: the invalid count, and with `indices` the count of distinct queries before):
//   bnd_mask_kernel      one lane per query in kd order; per hit the float angle sets one bit of a 64-bit occupancy mask
//                        (bnd_bin: a monotone float function of the angle, bin width w = 2 pi / 64).  Monotone: the bins are
//                        ordered as the angles are, so two consecutive sorted angles lie in one bin, in two neighbouring
//                        occupied bins, or on the two sides of a cyclic run of e empty bins -- and that gap lies within
//                        [e w - s, (e + 2) w + s], s the rounding of the bin edges (BND_SLACK is far above it).  With
//                        thr >= pi / 8 = 4 w a gap without an empty run never exceeds thr.  A run with e w > thr + s decides
//                        true, one with (e + 2) w < thr - s is no boundary gap; what is left (e_lo <= e <= e_hi, both from the
//                        host) is AMBIGUOUS and the lane is marked pending.  The run tests are rotate-and-AND on the mask.
//   bnd_resolve_kernel   only pending lanes walk again (a group of 64 without one is skipped); for four ambiguous runs of the
//                        lane, in named scalars, the largest angle of the bin before the run and the smallest of the bin
//                        after it: their float difference (the wrap formula where the run crosses +-pi) IS the reference's
//                        gap, compared with thr in float.  Launched ceil(max runs / 4) times, a number the host derives
//                        from thr (1 at pi / 2, 6 at pi / 8): no read-back in between.
//   bnd_knn_kernel       k mode: the same two steps over device-resident lists of pclhip_knn, one thread per point
//   bnd_emit_kernel      state of the query's position -> the caller's flag, the invalid queries counted
// Both walks are traverse<Policy, true> with a fixed bound inside for_each_query_group; a flag is a function of the set of
// angles only, so the traversal order cannot change it and two calls give the same bytes.  No wave waits for another.
//
// Deviations from the reference:
//   * a query with no neighbour at all, a non-finite record, a non-finite or zero normal: flag 0, counted in the invalid
//     count (the reference stores a NaN cast to uint8_t and clears is_dense, or sorts NaN angles)
//   * non-finite records are never neighbours; the index covers the whole unscaled cloud
//   * thr < pi / 8 is refused (the mask could no longer rule out the gaps between neighbouring bins)
#pragma once

#include "device_scan.hpp"
#include "outlier.hpp"  // OR_BLOCK, OR_WAVES, outlier_grid, or_blocks, outlier_pos_kernel, outlier_compact_kernel
#include "traverse.hpp"

namespace pclhip {
namespace {

constexpr float BND_PI = 3.14159274101257324f;         // float(M_PI)
constexpr float BND_TWO_PI = 6.28318548202514648f;     // 2 * float(M_PI)
constexpr float BND_BINS_PER_RAD = 10.1859163578813f;  // 64 / (2 pi)
constexpr int BND_BINS = 64;
constexpr double BND_BIN_WIDTH = 6.283185307179586476925 / BND_BINS;
// bnd_bin rounds twice on values below 64: its edges are off by less than 64 * 2 * 2^-24 bins = 7.5e-7 rad
constexpr double BND_SLACK = 1e-4;
constexpr uint8_t BND_FLAG = 1, BND_PENDING = 2, BND_INVALID = 4;

struct BndParams {
  float thr;
  int e_lo, e_hi;   // a cyclic run of e empty bins: e > e_hi decides true, e_lo <= e <= e_hi is ambiguous
  uint32_t min_nb;  // neighbours (the query included) below this: flag 0
};

struct BndBasis {
  float ux, uy, uz, vx, vy, vz;
};

__device__ __forceinline__ float bnd_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// getCoordinateSystemOnPlane (boundary.h:161-168): v = (nx, ny, nz, 0).unitOrthogonal() by Eigen's rule for vectors that
// are no 3-vectors -- maxi the first index of the largest |component|, sndi = (maxi == 0) ? 1 : 0, v[maxi] = -n[sndi] * inv,
// v[sndi] = n[maxi] * inv, inv = 1 / sqrt(n[sndi]^2 + n[maxi]^2) -- and u = n x v.  Selects on named scalars.
// false: the normal is not finite or zero
__device__ __forceinline__ bool bnd_basis(float nx, float ny, float nz, BndBasis& b) {
  b.ux = b.uy = b.uz = b.vx = b.vy = b.vz = 0.0f;
  if (!(isfinite(nx) && isfinite(ny) && isfinite(nz))) return false;
  if (nx == 0.0f && ny == 0.0f && nz == 0.0f) return false;
  const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
  int maxi = 0;
  float best = ax;
  if (ay > best) { maxi = 1; best = ay; }
  if (az > best) maxi = 2;
  const float nm = maxi == 0 ? nx : (maxi == 1 ? ny : nz);
  const float ns = maxi == 0 ? ny : nx;
  const float inv = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(__fmul_rn(ns, ns), __fmul_rn(nm, nm))));
  const float vm = __fmul_rn(-ns, inv), vs = __fmul_rn(nm, inv);
  b.vx = maxi == 0 ? vm : vs;
  b.vy = maxi == 0 ? vs : (maxi == 1 ? vm : 0.0f);
  b.vz = maxi == 2 ? vm : 0.0f;
  b.ux = __fsub_rn(__fmul_rn(ny, b.vz), __fmul_rn(nz, b.vy));
  b.uy = __fsub_rn(__fmul_rn(nz, b.vx), __fmul_rn(nx, b.vz));
  b.uz = __fsub_rn(__fmul_rn(nx, b.vy), __fmul_rn(ny, b.vx));
  return true;
}

// The per-neighbour step of both modes: the angle of p around q; false for an all-zero delta (q itself, a duplicate)
__device__ __forceinline__ bool bnd_angle(const BndBasis& b, float qx, float qy, float qz, float px, float py, float pz,
                                          float& angle) {
  const float dx = __fsub_rn(px, qx), dy = __fsub_rn(py, qy), dz = __fsub_rn(pz, qz);
  if (dx == 0.0f && dy == 0.0f && dz == 0.0f) return false;
  angle = atan2f(bnd_dot(b.vx, b.vy, b.vz, dx, dy, dz), bnd_dot(b.ux, b.uy, b.uz, dx, dy, dz));
  return true;
}

// 0 .. 63, monotone in the angle (an add and a multiplication by a positive constant, rounded, then clamped)
__device__ __forceinline__ int bnd_bin(float angle) {
  const float f = __fmul_rn(__fadd_rn(angle, BND_PI), BND_BINS_PER_RAD);
  return int(fminf(fmaxf(f, 0.0f), float(BND_BINS - 1)));
}

__device__ __forceinline__ uint64_t bnd_rotr(uint64_t x, int s) {
  s &= 63;
  return s != 0 ? (x >> s) | (x << (64 - s)) : x;
}

// does the occupancy mask (not 0) leave a cyclic run of at least `len` empty bins
__device__ __forceinline__ bool bnd_has_empty_run(uint64_t occ, int len) {
  if (len >= BND_BINS) return false;
  if (len <= 0) return true;
  uint64_t x = ~occ;  // bit i of x after the loop: bins i .. i + s - 1 are empty
  int s = 1;
  while (2 * s <= len) {
    x &= bnd_rotr(x, s);
    s *= 2;
  }
  x &= bnd_rotr(x, len - s);
  return x != 0;
}

// the decision of the mask pass
__device__ __forceinline__ uint8_t bnd_decide(uint64_t occ, uint32_t cnt, const BndParams& prm) {
  if (cnt == 0u) return BND_INVALID;
  if (cnt < prm.min_nb || occ == 0ull) return 0;
  if (bnd_has_empty_run(occ, prm.e_hi + 1)) return BND_FLAG;
  if (bnd_has_empty_run(occ, prm.e_lo)) return BND_PENDING;
  return 0;
}

// Up to four ambiguous runs of a lane: the bin before (b) and after (a) each, the largest angle seen in the one and the
// smallest in the other.  Named scalars only (run-time-indexed per-lane arrays go to scratch: iss.hpp).
struct BndRuns {
  int b0, b1, b2, b3, a0, a1, a2, a3;
  float hi0, hi1, hi2, hi3, lo0, lo1, lo2, lo3;
  // the ambiguous runs number first .. first + 3 in ascending bin order -> how many ambiguous runs the mask has in all
  __device__ __forceinline__ int select(uint64_t occ, int first, const BndParams& prm) {
    b0 = b1 = b2 = b3 = a0 = a1 = a2 = a3 = -1;
    hi0 = hi1 = hi2 = hi3 = -__builtin_inff();
    lo0 = lo1 = lo2 = lo3 = __builtin_inff();
    int c = 0;
    for (uint64_t m = occ; m != 0; m &= m - 1ull) {
      const int b = __builtin_ctzll(m);
      const int e = __builtin_ctzll(bnd_rotr(occ, b + 1));  // empty bins up to the next occupied one (63: b is the only one)
      if (e < prm.e_lo || e > prm.e_hi) continue;
      const int a = (b + e + 1) & 63;
      const int k = c - first;
      if (k == 0) { b0 = b; a0 = a; }
      if (k == 1) { b1 = b; a1 = a; }
      if (k == 2) { b2 = b; a2 = a; }
      if (k == 3) { b3 = b; a3 = a; }
      ++c;
    }
    return c;
  }
  __device__ __forceinline__ void update(float angle) {
    const int bin = bnd_bin(angle);
    if (bin == b0) hi0 = fmaxf(hi0, angle);
    if (bin == b1) hi1 = fmaxf(hi1, angle);
    if (bin == b2) hi2 = fmaxf(hi2, angle);
    if (bin == b3) hi3 = fmaxf(hi3, angle);
    if (bin == a0) lo0 = fminf(lo0, angle);
    if (bin == a1) lo1 = fminf(lo1, angle);
    if (bin == a2) lo2 = fminf(lo2, angle);
    if (bin == a3) lo3 = fminf(lo3, angle);
  }
  // boundary.hpp:120-133: angles[i + 1] - angles[i], and 2 * float(M_PI) - angles.back() + angles.front() for the pair
  // whose successor wraps (the bin after is not above the bin before)
  static __device__ __forceinline__ bool gap_gt(int b, int a, float hi, float lo, float thr) {
    if (b < 0) return false;
    const float gap = a > b ? __fsub_rn(lo, hi) : __fadd_rn(__fsub_rn(BND_TWO_PI, hi), lo);
    return gap > thr;
  }
  __device__ __forceinline__ bool any_gap_gt(float thr) const {
    return gap_gt(b0, a0, hi0, lo0, thr) || gap_gt(b1, a1, hi1, lo1, thr) || gap_gt(b2, a2, hi2, lo2, thr) ||
           gap_gt(b3, a3, hi3, lo3, thr);
  }
};

// Pass 1: the neighbour count and the occupancy mask of the angles
struct BndMask {
  float t;
  BndBasis bs;
  uint32_t cnt, n;
  uint64_t occ;
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
      float a;
      if (bnd_angle(bs, qx[0], qy[0], qz[0], leaf_coord<16>(s, 0, j), leaf_coord<16>(s, 1, j), leaf_coord<16>(s, 2, j), a))
        occ |= 1ull << bnd_bin(a);
    }
  }
};

// waves per SIMD (kernel-resource-usage, gfx950): see DESIGN.md row f-14
__global__ __launch_bounds__(OR_BLOCK) void bnd_mask_kernel(IndexView ix, const uint32_t* __restrict__ qpos, uint32_t nq,
                                                            float t, BndParams prm, uint64_t* __restrict__ occ,
                                                            uint8_t* __restrict__ state, uint32_t* __restrict__ n_pending) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  const int lane = threadIdx.x & (WAVE - 1);
  TraverseStats ts;
  for_each_query_group(ix, qpos, nq, [&](uint32_t pos, bool real, float4 p) {
    float4 nq4 = make_float4(0, 0, 0, 0);
    if (real) nq4 = ix.nrm[pos];
    BndMask pol;
    const bool ok = bnd_basis(nq4.x, nq4.y, nq4.z, pol.bs) && real;
    pol.t = t;
    pol.n = ix.n;
    pol.cnt = 0;
    pol.occ = 0;
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {ok};
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a query
    traverse<BndMask, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    const uint8_t st = ok ? bnd_decide(pol.occ, pol.cnt, prm) : BND_INVALID;
    const uint64_t pend = __builtin_amdgcn_ballot_w64(real && st == BND_PENDING);
    if (pend != 0 && lane == 0) atomicAdd(n_pending, uint32_t(__builtin_popcountll(pend)));
    if (!real) return;
    state[pos] = st;
    occ[pos] = pol.occ;
  });
}

// Pass 2: the exact gaps of four ambiguous runs
struct BndResolve {
  float t;
  BndBasis bs;
  BndRuns runs;
  uint32_t n;
  bool active;
  static constexpr int QPL = 1;
  static constexpr bool LANE_SPARSE = true;
  static constexpr bool NEEDS_W = false;
  __device__ __forceinline__ float worst(int) const { return active ? t : -1.0f; }
  __device__ __forceinline__ void leaf_lane(const float* buf, uint32_t slot, uint32_t leaf_id, const float* qx,
                                            const float* qy, const float* qz) {
    if (leaf_id == NO_INDEX || !active) return;
    const float4* s = reinterpret_cast<const float4*>(buf) + slot;
    uint32_t mask = leaf_hits_lt<16>(s, qx[0], qy[0], qz[0], t);
    const uint32_t base = leaf_id * uint32_t(LEAF);
    if (n - base < uint32_t(LEAF)) mask &= (1u << (n - base)) - 1u;
    while (mask != 0) {
      const uint32_t j = uint32_t(__builtin_ctz(mask));
      mask &= mask - 1u;
      float a;
      if (bnd_angle(bs, qx[0], qy[0], qz[0], leaf_coord<16>(s, 0, j), leaf_coord<16>(s, 1, j), leaf_coord<16>(s, 2, j), a))
        runs.update(a);
    }
  }
};

__global__ __launch_bounds__(OR_BLOCK) void bnd_resolve_kernel(IndexView ix, const uint32_t* __restrict__ qpos, uint32_t nq,
                                                               float t, BndParams prm, int first,
                                                               const uint64_t* __restrict__ occ, uint8_t* __restrict__ state) {
  __shared__ WaveLdsBoxT<3072> wl_s[OR_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  load_top_cache(ix, topbox_s);
  TraverseStats ts;
  for_each_query_group(ix, qpos, nq, [&](uint32_t pos, bool real, float4 p) {
    const bool pending = real && state[pos] == BND_PENDING;
    if (__builtin_amdgcn_ballot_w64(pending) == 0) return;
    BndResolve pol;
    float4 nq4 = make_float4(0, 0, 1, 0);
    if (pending) nq4 = ix.nrm[pos];
    (void)bnd_basis(nq4.x, nq4.y, nq4.z, pol.bs);  // (a pending lane's normal passed this test in the mask pass)
    pol.t = t;
    pol.n = ix.n;
    pol.active = pending;
    const int total = pol.runs.select(pending ? occ[pos] : 0ull, first, prm);
    const float qx[1] = {p.x}, qy[1] = {p.y}, qz[1] = {p.z};
    const bool vv[1] = {pending};
    const uint32_t start = uniform_u32(pos / LEAF);  // lane 0 always holds a query
    traverse<BndResolve, true>(ix, qx, qy, qz, vv, pol, wl_s[threadIdx.x / WAVE], topbox_s, ts, start);
    if (!pending) return;
    if (pol.runs.any_gap_gt(prm.thr)) state[pos] = BND_FLAG;
    else if (total <= first + 4) state[pos] = 0;  // every ambiguous run has been looked at
  });
}

// k mode: the lists of pclhip_knn over the index's own points, list `pos` = the neighbours of the point at sorted position
// pos as original ids (< 0: no such neighbour).  One thread per point, the mask step and then every resolve step.
__global__ __launch_bounds__(OR_BLOCK) void bnd_knn_kernel(IndexView ix, const int32_t* __restrict__ lists, int k,
                                                           const uint32_t* __restrict__ rank, uint64_t n_orig, BndParams prm,
                                                           uint8_t* __restrict__ state, uint32_t* __restrict__ n_pending) {
  const uint32_t pos = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (pos >= ix.n) return;
  const float4 q = ix.pts[pos], nq4 = ix.nrm[pos];
  BndBasis bs;
  if (!bnd_basis(nq4.x, nq4.y, nq4.z, bs)) {
    state[pos] = BND_INVALID;
    return;
  }
  const int32_t* list = lists + size_t(pos) * size_t(k);
  uint32_t cnt = 0;
  uint64_t occ = 0;
  for (int j = 0; j < k; ++j) {
    const int32_t id = list[j];
    if (id < 0 || uint64_t(id) >= n_orig) continue;
    const uint32_t pp = rank[id];
    if (pp == NO_INDEX) continue;
    ++cnt;
    const float4 c = ix.pts[pp];
    float a;
    if (bnd_angle(bs, q.x, q.y, q.z, c.x, c.y, c.z, a)) occ |= 1ull << bnd_bin(a);
  }
  uint8_t st = bnd_decide(occ, cnt, prm);
  if (st == BND_PENDING) {
    atomicAdd(n_pending, 1u);
    st = 0;
    int total = 1;
    for (int first = 0; first < total && st == 0; first += 4) {
      BndRuns runs;
      total = runs.select(occ, first, prm);
      for (int j = 0; j < k; ++j) {
        const int32_t id = list[j];
        if (id < 0 || uint64_t(id) >= n_orig) continue;
        const uint32_t pp = rank[id];
        if (pp == NO_INDEX) continue;
        const float4 c = ix.pts[pp];
        float a;
        if (bnd_angle(bs, q.x, q.y, q.z, c.x, c.y, c.z, a)) runs.update(a);
      }
      if (runs.any_gap_gt(prm.thr)) st = BND_FLAG;
    }
  }
  state[pos] = st;
}

// flag of entry j <- the state of record idx[j] (or j); a record the index dropped is invalid.  `fill`: every query is
// invalid (nobody has a neighbour)
__global__ __launch_bounds__(OR_BLOCK) void bnd_emit_kernel(const uint8_t* __restrict__ state, const int32_t* __restrict__ idx,
                                                            uint64_t m, const uint32_t* __restrict__ rank, uint64_t n_orig,
                                                            int fill, uint8_t* __restrict__ out,
                                                            unsigned long long* __restrict__ invalid) {
  const uint64_t j = uint64_t(blockIdx.x) * OR_BLOCK + threadIdx.x;
  if (j >= m) return;
  const int64_t id = idx ? int64_t(idx[j]) : int64_t(j);
  uint32_t pos = NO_INDEX;
  if (id >= 0 && uint64_t(id) < n_orig) pos = rank[id];
  const uint8_t st = (pos != NO_INDEX && fill == 0) ? state[pos] : BND_INVALID;
  out[j] = (st & BND_FLAG) != 0 ? 1 : 0;
  if ((st & BND_INVALID) != 0) atomicAdd(invalid, 1ull);
}

}  // namespace

// The host side of pclhip_boundary (api.hip): t is the float square of the radius (k == 0) or k >= 1 asks for k mode.
pclhip_status boundary_compute(pclhip_index* ix, const int32_t* indices, uint64_t n_indices, float t, int k, float thr,
                               uint32_t min_nb, uint8_t* out_flags, uint64_t* out_invalid) {
  pclhip_ctx* ctx = ix->ctx;
  hipStream_t s = ctx->stream;
  const uint64_t m64 = indices ? n_indices : ix->n_orig;
  PCLHIP_REQUIRE(ctx, m64 < 0x7FFFFFFFull, "too many queries");
  const uint32_t n = ix->n;
  const uint32_t m = uint32_t(m64);
  if (out_invalid) *out_invalid = 0;
  ix->boundary_pass_ms[0] = ix->boundary_pass_ms[1] = 0.0;
  ix->boundary_pending = 0;
  if (m == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  DeviceScope scope(ctx);
  BndParams prm;
  prm.thr = thr;
  prm.min_nb = min_nb < 3u ? 3u : min_nb;
  {
    const double lo = std::ceil((double(thr) - BND_SLACK) / BND_BIN_WIDTH - 2.0);
    const double hi = std::floor((double(thr) + BND_SLACK) / BND_BIN_WIDTH);
    prm.e_lo = int(std::min(std::max(lo, 1.0), 1000.0));
    prm.e_hi = int(std::min(std::max(hi, 0.0), 1000.0));
  }
  // resolve launches: an ambiguous run and the occupied bin before it take e_lo + 1 bins, four runs per launch
  const int max_runs = prm.e_lo < BND_BINS ? BND_BINS / (prm.e_lo + 1) : 0;
  const int launches = prm.e_lo <= std::min(prm.e_hi, BND_BINS - 1) ? (std::max(max_runs, 1) + 3) / 4 : 0;
  const void* d_idx_v = nullptr;
  if (indices) {
    void* owned = nullptr;
    const pclhip_status st = to_device(ctx, indices, size_t(m) * 4, &d_idx_v, &owned);
    if (st != PCLHIP_OK) return st;
    scope.mem.push_back(owned);
  }
  const int32_t* d_idx = static_cast<const int32_t*>(d_idx_v);
  struct ReadBack {
    unsigned long long invalid;
    uint32_t tot_q[4];
    uint32_t bad;
    uint32_t pending;
  };
  ReadBack* rb = nullptr;
  uint64_t* occ = nullptr;
  uint8_t* state = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rb, sizeof(ReadBack)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&occ, size_t(n) * 8));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&state, size_t(n)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(rb, 0, sizeof(ReadBack), s));
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr, e4 = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.event(&e0));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e1));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e2));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e3));
  PCLHIP_CHECK_HIP(ctx, scope.event(&e4));
  (void)hipEventRecord(e0, s);
  uint32_t* qpos = nullptr;
  uint32_t nq = n;
  if (indices) {
    // the positions asked for, ascending: the queries stay in kd order (fpfh.hpp)
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
  const IndexView v = ix->view();
  const bool nobody = k == 0 && !(t > 0.0f);  // nothing lies within d2 < 0: every query is invalid
  (void)hipEventRecord(e1, s);
  if (k > 0 && n > 0) {
    int32_t* lists = nullptr;
    float* d2 = nullptr;
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&lists, size_t(n) * size_t(k) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&d2, size_t(n) * size_t(k) * 4));
    // the library's own k-NN path over the index's points in kd order (the caller holds the context's recursive lock)
    const pclhip_status st = pclhip_knn(ix, ix->pts, sizeof(float4), n, k, lists, d2);
    if (st != PCLHIP_OK) return st;
    (void)hipEventRecord(e1, s);
    hipLaunchKernelGGL(bnd_knn_kernel, or_blocks(n), dim3(OR_BLOCK), 0, s, v, lists, k, ix->rank, ix->n_orig, prm, state,
                       &rb->pending);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(e2, s);
    (void)hipEventRecord(e3, s);
  } else {
    if (nq > 0 && !nobody) {
      PCLHIP_LAUNCH_FED(ctx, bnd_mask_kernel, dim3(outlier_grid(ctx, bnd_mask_kernel, nq)), dim3(OR_BLOCK), 0, s, v, qpos, nq,
                        t, prm, occ, state, &rb->pending);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    }
    (void)hipEventRecord(e2, s);
    if (nq > 0 && !nobody) {
      for (int r = 0; r < launches; ++r) {
        PCLHIP_LAUNCH_FED(ctx, bnd_resolve_kernel, dim3(outlier_grid(ctx, bnd_resolve_kernel, nq)), dim3(OR_BLOCK), 0, s, v,
                          qpos, nq, t, prm, 4 * r, occ, state);
        PCLHIP_CHECK_HIP(ctx, hipGetLastError());
      }
    }
    (void)hipEventRecord(e3, s);
  }
  const bool out_dev = is_device_pointer(out_flags);
  uint8_t* d_out = out_flags;
  if (!out_dev) PCLHIP_CHECK_HIP(ctx, scope.alloc(&d_out, size_t(m)));
  hipLaunchKernelGGL(bnd_emit_kernel, or_blocks(m), dim3(OR_BLOCK), 0, s, state, d_idx, uint64_t(m), ix->rank, ix->n_orig,
                     nobody ? 1 : 0, d_out, &rb->invalid);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  (void)hipEventRecord(e4, s);
  ReadBack h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rb, sizeof h, hipMemcpyDeviceToHost, s));  // the invalid count
  if (!out_dev) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_flags, d_out, size_t(m), hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, e0, e4) == hipSuccess) ix->last_kernel_ms = ms;
  if (hipEventElapsedTime(&ms, e1, e2) == hipSuccess) ix->boundary_pass_ms[0] = ms;
  if (hipEventElapsedTime(&ms, e2, e3) == hipSuccess) ix->boundary_pass_ms[1] = ms;
  ix->boundary_pending = h.pending;
  if (out_invalid) *out_invalid = h.invalid;
  return PCLHIP_OK;
}

}  // namespace pclhip
