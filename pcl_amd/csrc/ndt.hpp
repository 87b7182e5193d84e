// ndt.hpp -- NormalDistributionsTransform (registration/include/pcl/registration/ndt.h, impl/ndt.hpp) over the voxel
// Gaussians of ndt_cells.hpp.  Included by radius.hip: the derivative pass is a radius traversal of the index over the
// cells' centroids (NeighborSearchMethod::RADIUS, target_cells_.radiusSearch(x', resolution_)).
//
// One launch per evaluation (computeDerivatives, impl/ndt.hpp:209-304; computeHessian, :514-571):
//   ndt_eval_kernel<G, H>   per source point (kd order, 64 per wave): x' = T x in float (Transformer::se3 order, fused:
//                           no transformed cloud is stored); the walk only COLLECTS the cells with float
//                           d2 < float(r * r) into the thread's list (NdtCollect; at most 27 by geometry, 32 slots, one
//                           coalesced column per thread of the grid in global memory -- written and read back by the same
//                           thread, it stays in L2); behind the walk the pair loop gathers each cell's 72-byte record and
//                           adds the pair's score / gradient / upper Hessian triangle (nf::pair_terms) to 29 per-thread
//                           doubles.  The accumulators are not touched during the walk; the walk's state is dead in the
//                           pair loop.  Three variants as the reference has them: <1,1> score + gradient + Hessian,
//                           <1,0> the line search's trials, <0,1> computeHessian.
//   sums                    per thread in traversal order over a FIXED share of the groups (GroupSchedule without the
//                           dynamic tail: which wave serves which group does not depend on timing), then the
//                           fixed-order block sums of block_sums.hpp (rows of 32 doubles): a variant gives the bits of
//                           the full pass for its part.
// The serial step (6x6 SVD solve, More-Thuente, convergence test: ndt_forms.hpp, host_math.cpp) runs on the host between
// passes: one read-back of the sums per evaluation, nothing else crosses.
#pragma once

#include <chrono>

#include "block_sums.hpp"
#include "icp_xform.hpp"
#include "ndt_forms.hpp"
#include "traverse.hpp"

struct pclhip_ndt {
  pclhip_ctx* ctx = nullptr;
  // target: a device copy of the records, its voxel Gaussians and the index over their centroids (cached per
  // resolution / min_points_per_voxel / min_covar_eigvalue_mult)
  void* tgt = nullptr;
  size_t tgt_stride = 0;
  uint64_t tgt_n = 0;
  pclhip::NdtCells cells;
  pclhip_index* cell_index = nullptr;
  bool cells_built = false;
  float cells_res = 0.0f;
  uint32_t cells_min_pts = 0;
  double cells_mult = 0.0;
  // source: a device copy of the records and the points in kd order (w = original index)
  void* src = nullptr;
  size_t src_stride = 0;
  uint64_t src_n = 0;
  float4* src_sorted = nullptr;
  // evaluation state
  uint32_t* lists = nullptr;    // [NDT_LIST_CAP][blocks * NDT_BLOCK]
  pclhip::BlockSums<32> sums;   // (NDT_ROW) rows of an evaluation; sums.blocks is the evaluation's grid
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  int evals[3] = {0, 0, 0};     // full, gradient, Hessian passes of the last align
  double eval_ms[3] = {0, 0, 0};
  uint64_t last_pairs = 0;
  pclhip_ndt_trace* trace = nullptr;
  int trace_capacity = 0;
  float final_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // getFitnessScore: an index over the target's points and an ICP registration on it, made on first use
  pclhip_index* tgt_index = nullptr;
  pclhip_icp* icp = nullptr;
  bool icp_source_set = false;
};

namespace pclhip {
namespace {

constexpr int NDT_BLOCK = 256;
constexpr int NDT_WAVES = NDT_BLOCK / WAVE;
constexpr int NDT_LIST_CAP = 32;
constexpr int NDT_NS = nf::kNdtSums + 1;  // + the number of points whose list overflowed (must be 0)
constexpr int NDT_ROW = 32;               // doubles per block row (pclhip_ndt::sums)
static_assert(NDT_NS <= NDT_ROW, "a row holds every sum");

// collects the cells within the radius: l[3 * LEAF + j] is the centroid's position among the cells
struct NdtCollect {
  static constexpr int QPL = 1;
  float r2;
  uint32_t cnt;
  bool active;
  uint32_t* list;   // this thread's column
  uint32_t stride;  // threads of the grid
  __device__ __forceinline__ float worst(int) const { return r2; }
  __device__ __forceinline__ void push(uint32_t id) {
    if (cnt < uint32_t(NDT_LIST_CAP)) list[size_t(cnt) * stride] = id;
    ++cnt;
  }
  __device__ __forceinline__ void leaf(const float* l, uint32_t, const float* qx, const float* qy, const float* qz) {
    const v2f qx2 = {qx[0], qx[0]}, qy2 = {qy[0], qy[0]}, qz2 = {qz[0], qz[0]};
#pragma unroll
    for (int j = 0; j < LEAF / 2; ++j) {
      const v2f r = pair_dist(l, j, qx2, qy2, qz2);
      if (active && r.x < r2) push(__float_as_uint(l[3 * LEAF + 2 * j]));
      if (active && r.y < r2) push(__float_as_uint(l[3 * LEAF + 2 * j + 1]));
    }
  }
};

template <bool WITH_G, bool WITH_H>
__global__ __launch_bounds__(NDT_BLOCK, 2) void ndt_eval_kernel(IndexView ix, const float4* __restrict__ src, uint32_t n, Mat34 T,
                                                                float r2, const double* __restrict__ cells, uint32_t ncells,
                                                                nf::NdtAngles A, double d1, double d2,
                                                                uint32_t* __restrict__ lists, double* __restrict__ partials) {
  __shared__ WaveLdsBoxT<LEAF_BATCH * LEAF_FLOATS * 4> wl_s[NDT_WAVES];
  __shared__ Box topbox_s[TOPCACHE_BOXES];
  __shared__ double red_s[NDT_WAVES][NDT_NS];
  load_top_cache(ix, topbox_s);
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  double acc[NDT_NS];
#pragma unroll
  for (int s = 0; s < NDT_NS; ++s) acc[s] = 0.0;
  NdtCollect pol;
  pol.r2 = r2;
  pol.stride = gridDim.x * NDT_BLOCK;
  pol.list = lists + size_t(blockIdx.x) * NDT_BLOCK + threadIdx.x;
  const uint32_t ngroups = (n + WAVE - 1) / WAVE;
  const GroupSchedule sched(ngroups);
  TraverseStats ts;
  for (uint32_t gl = sched.first(); gl < sched.end(); gl += sched.step()) {
    const uint32_t g = sched.global(gl);
    if (g >= ngroups) break;
    const uint32_t i = g * WAVE + lane;
    float4 p = make_float4(0, 0, 0, 0);
    const bool real = i < n;
    if (real) p = src[i];
    const float tx = xform_row(T.m[0], T.m[1], T.m[2], T.m[3], p.x, p.y, p.z, 1);
    const float ty = xform_row(T.m[4], T.m[5], T.m[6], T.m[7], p.x, p.y, p.z, 1);
    const float tz = xform_row(T.m[8], T.m[9], T.m[10], T.m[11], p.x, p.y, p.z, 1);
    const bool vv[1] = {real && isfinite(tx) && isfinite(ty) && isfinite(tz)};
    const float qx[1] = {tx}, qy[1] = {ty}, qz[1] = {tz};
    pol.cnt = 0;
    pol.active = vv[0];
    traverse(ix, qx, qy, qz, vv, pol, wl_s[wave], topbox_s, ts);
    const uint32_t m = pol.cnt < uint32_t(NDT_LIST_CAP) ? pol.cnt : uint32_t(NDT_LIST_CAP);
    acc[nf::kNdtSums - 1] += double(pol.cnt);
    if (pol.cnt > uint32_t(NDT_LIST_CAP)) acc[NDT_NS - 1] += 1.0;
    const double x[3] = {double(p.x), double(p.y), double(p.z)};
    const double xp[3] = {double(tx), double(ty), double(tz)};
    for (uint32_t k = 0; k < m; ++k) {
      const uint32_t id = pol.list[size_t(k) * pol.stride];
      if (id >= ncells) continue;
      const double* c = cells + size_t(id) * nf::kNdtCellDoubles;
      const double xt[3] = {xp[0] - c[0], xp[1] - c[1], xp[2] - c[2]};
      const double C[6] = {c[3], c[4], c[5], c[6], c[7], c[8]};
      nf::pair_terms<WITH_G, WITH_H>(x, xt, C, A, d1, d2, acc);
    }
  }
  // The wave step of block_sums.hpp, written out (red_s is touched behind the walk only).  Through wave_rows the helper's
  // loop is unrolled before it is inlined here, and the register allocation of this kernel moves with it: <1,1> 248 -> 250
  // VGPRs, <0,1> 238 -> 237, the accumulators' copies in another place.
#pragma unroll
  for (int s = 0; s < NDT_NS; ++s) {
    const double v = wave_sum_d(acc[s]);
    if (lane == 0) red_s[wave][s] = v;
  }
  block_store<NDT_NS, NDT_WAVES, NDT_ROW>(red_s, partials);
}

void ndt_drop_fitness(pclhip_ndt* N, bool target_too) {
  if (N->icp) {
    pclhip_icp_destroy(N->icp);
    N->icp = nullptr;
    N->icp_source_set = false;
  }
  if (target_too && N->tgt_index) {
    pclhip_index_destroy(N->tgt_index);
    N->tgt_index = nullptr;
  }
}

void ndt_drop_cells(pclhip_ndt* N) {
  if (N->cell_index) pclhip_index_destroy(N->cell_index);
  N->cell_index = nullptr;
  ndt_free_cells(N->ctx, &N->cells);
  N->cells_built = false;
}

// the voxel Gaussians and their index for these parameters (cached); *ms: wall time of a build, 0 when cached
pclhip_status ndt_ensure_cells(pclhip_ndt* N, const pclhip_ndt_params* P, double* ms) {
  pclhip_ctx* ctx = N->ctx;
  if (ms) *ms = 0.0;
  PCLHIP_REQUIRE(ctx, N->tgt != nullptr || N->tgt_n == 0, "no input target dataset was given");
  PCLHIP_REQUIRE(ctx, P->resolution > 0.0f, "resolution must be positive");
  const uint32_t min_pts = uint32_t(P->min_points_per_voxel < 3 ? 3 : P->min_points_per_voxel);  // voxel_grid_covariance.h:214-225
  if (N->cells_built && N->cells_res == P->resolution && N->cells_min_pts == min_pts &&
      N->cells_mult == P->min_covar_eigvalue_mult)
    return PCLHIP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  ndt_drop_cells(N);
  if (N->tgt_n > 0) {
    pclhip_status st = ndt_build_cells(ctx, N->tgt, N->tgt_stride, N->tgt_n, P->resolution, min_pts, P->min_covar_eigvalue_mult,
                                       &N->cells);
    // a leaf too small for int32 voxel ids: the reference's filter warns and leaves no voxel
    // (voxel_grid_covariance.hpp:83-88), the registration is then "not searchable"
    if (st != PCLHIP_OK && st != PCLHIP_ERR_OVERFLOW) return st;
    if (N->cells.count > 0) {
      st = build_index_from_float4(ctx, N->cells.centroid, N->cells.count, &N->cell_index);
      if (st != PCLHIP_OK) {
        ndt_drop_cells(N);
        return st;
      }
    }
  }
  N->cells_built = true;
  N->cells_res = P->resolution;
  N->cells_min_pts = min_pts;
  N->cells_mult = P->min_covar_eigvalue_mult;
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PCLHIP_OK;
}

// one evaluation pass: variant 0 score + gradient + Hessian, 1 score + gradient, 2 Hessian.  out: NDT_NS sums
pclhip_status ndt_eval(pclhip_ndt* N, const pclhip_ndt_params* P, int variant, const float T[16], const nf::NdtAngles& A,
                       double d1, double d2, double* out) {
  pclhip_ctx* ctx = N->ctx;
  for (int s = 0; s < NDT_NS; ++s) out[s] = 0.0;
  ++N->evals[variant];
  const uint32_t n = uint32_t(N->src_n);
  if (n == 0 || N->cells.count == 0) return PCLHIP_OK;
  const Mat34 M = mat34_of(T);
  const double rr = double(P->resolution) * double(P->resolution);
  const float r2 = float(rr);  // kdtree_flann.hpp:398
  const IndexView v = N->cell_index->view();
  const dim3 grid(N->sums.blocks), block(NDT_BLOCK);
  (void)hipEventRecord(N->ev_a, ctx->stream);
  if (variant == 0)
    hipLaunchKernelGGL((ndt_eval_kernel<true, true>), grid, block, 0, ctx->stream, v, N->src_sorted, n, M, r2, N->cells.rec,
                       N->cells.count, A, d1, d2, N->lists, N->sums.partials);
  else if (variant == 1)
    hipLaunchKernelGGL((ndt_eval_kernel<true, false>), grid, block, 0, ctx->stream, v, N->src_sorted, n, M, r2, N->cells.rec,
                       N->cells.count, A, d1, d2, N->lists, N->sums.partials);
  else
    hipLaunchKernelGGL((ndt_eval_kernel<false, true>), grid, block, 0, ctx->stream, v, N->src_sorted, n, M, r2, N->cells.rec,
                       N->cells.count, A, d1, d2, N->lists, N->sums.partials);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  const pclhip_status st = N->sums.read(ctx, NDT_NS, out, N->ev_b);
  if (st != PCLHIP_OK) return st;
  float ms = 0;
  if (hipEventElapsedTime(&ms, N->ev_a, N->ev_b) == hipSuccess) N->eval_ms[variant] += ms;
  if (out[NDT_NS - 1] != 0.0) {
    set_error(ctx, "NormalDistributionsTransform: a point met more than 32 cells within the resolution");
    return PCLHIP_ERR_STATE;
  }
  N->last_pairs = uint64_t(out[nf::kNdtSums - 1]);
  return PCLHIP_OK;
}

void ndt_unpack(const double* sums, double* score, double g[6], double H[36]) {
  *score = sums[0];
  for (int i = 0; i < 6; ++i) g[i] = sums[1 + i];
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) H[6 * i + j] = H[6 * j + i] = sums[7 + nf::tri21(i, j)];
}

struct NdtState {  // what computeStepLengthMT reads and leaves behind
  double score;
  double g[6];
  double H[36];
  float final_T[16];
};

// computeStepLengthMT (impl/ndt.hpp:778-934); *trials: iterations of its loop
pclhip_status ndt_step_length(pclhip_ndt* N, const pclhip_ndt_params* P, double d1, double d2, const double x[6], double dir[6],
                              double step_init, double step_max, double step_min, NdtState& S, double* step, int* trials) {
  *trials = 0;
  const double phi_0 = -S.score;
  double d_phi_0 = 0.0;
  for (int k = 0; k < 6; ++k) d_phi_0 += S.g[k] * dir[k];
  d_phi_0 = -d_phi_0;
  if (d_phi_0 >= 0) {
    if (d_phi_0 == 0) {
      *step = 0.0;
      return PCLHIP_OK;
    }
    d_phi_0 *= -1;
    for (int k = 0; k < 6; ++k) dir[k] *= -1;
  }
  const double mu = 1.e-4, nu = 0.9;
  nf::MtInterval I;
  I.a_l = I.a_u = 0.0;
  I.f_l = I.f_u = phi_0 - phi_0 - mu * d_phi_0 * 0.0;  // psi(0)
  I.g_l = I.g_u = d_phi_0 - mu * d_phi_0;
  bool interval_converged = (step_max - step_min) < 0, open_interval = true;
  double a_t = step_init;
  a_t = step_max < a_t ? step_max : a_t;
  a_t = a_t < step_min ? step_min : a_t;
  double x_t[6], sums[NDT_NS];
  nf::NdtAngles A;
  const auto evaluate = [&](int variant) -> pclhip_status {
    for (int k = 0; k < 6; ++k) x_t[k] = x[k] + dir[k] * a_t;
    nf::convert_transform(x_t, S.final_T);
    nf::angle_tables(x_t, A);
    const pclhip_status st = ndt_eval(N, P, variant, S.final_T, A, d1, d2, sums);
    if (st != PCLHIP_OK) return st;
    double Hd[36];
    ndt_unpack(sums, &S.score, S.g, variant == 0 ? S.H : Hd);
    return PCLHIP_OK;
  };
  pclhip_status st = evaluate(0);
  if (st != PCLHIP_OK) return st;
  const auto slope = [&]() {
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += S.g[k] * dir[k];
    return -s;
  };
  double phi_t = -S.score, d_phi_t = slope();
  double psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t, d_psi_t = d_phi_t - mu * d_phi_0;
  int it = 0;
  while (!interval_converged && it < 10 && (psi_t > 0 || d_phi_t > -nu * d_phi_0)) {
    a_t = open_interval ? nf::mt_trial_value(I, a_t, psi_t, d_psi_t) : nf::mt_trial_value(I, a_t, phi_t, d_phi_t);
    a_t = step_max < a_t ? step_max : a_t;
    a_t = a_t < step_min ? step_min : a_t;
    st = evaluate(1);
    if (st != PCLHIP_OK) return st;
    phi_t = -S.score;
    d_phi_t = slope();
    psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t;
    d_psi_t = d_phi_t - mu * d_phi_0;
    if (open_interval && (psi_t <= 0 && d_psi_t >= 0)) {
      open_interval = false;
      I.f_l += phi_0 - mu * d_phi_0 * I.a_l;
      I.g_l += mu * d_phi_0;
      I.f_u += phi_0 - mu * d_phi_0 * I.a_u;
      I.g_u += mu * d_phi_0;
    }
    interval_converged = open_interval ? nf::mt_update_interval(I, a_t, psi_t, d_psi_t) : nf::mt_update_interval(I, a_t, phi_t, d_phi_t);
    ++it;
  }
  if (it) {  // computeHessian at the accepted trial (:926-931)
    st = ndt_eval(N, P, 2, S.final_T, A, d1, d2, sums);
    if (st != PCLHIP_OK) return st;
    double sc, gd[6];
    ndt_unpack(sums, &sc, gd, S.H);
  }
  *trials = it;
  *step = a_t;
  return PCLHIP_OK;
}

pclhip_status ndt_copy_records(pclhip_ctx* ctx, const void* points, size_t stride, uint64_t n, void** dst) {
  dev_free_if(ctx, *dst);
  *dst = nullptr;
  if (n == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, dst, size_t(n) * stride));
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(*dst, points, size_t(n) * stride, hipMemcpyDefault, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PCLHIP_OK;
}

}  // namespace
}  // namespace pclhip

using namespace pclhip;

extern "C" {

void pclhip_ndt_params_default(pclhip_ndt_params* p) {
  if (!p) return;
  // ndt.h:110-113, 675-682; impl/ndt.hpp:75-76; voxel_grid_covariance.h:571-574; registration.h (rotation epsilon 0)
  p->resolution = 1.0f;
  p->step_size = 0.1;
  p->outlier_ratio = 0.55;
  p->transformation_epsilon = 0.1;
  p->transformation_rotation_epsilon = 0.0;
  p->max_iterations = 35;
  p->min_points_per_voxel = 6;
  p->min_covar_eigvalue_mult = 0.01;
  p->neighborhood_search_method = PCLHIP_NDT_RADIUS;
}

pclhip_status pclhip_ndt_create(pclhip_ctx* ctx, pclhip_ndt** out) {
  if (!ctx || !out) return PCLHIP_ERR_INVALID;
  *out = nullptr;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  pclhip_ndt* N = new pclhip_ndt();
  N->ctx = ctx;
  if (N->sums.create(ctx) != hipSuccess || hipEventCreate(&N->ev_a) != hipSuccess || hipEventCreate(&N->ev_b) != hipSuccess) {
    set_error(ctx, "allocation failed in pclhip_ndt_create");
    pclhip_ndt_destroy(N);
    return PCLHIP_ERR_HIP;
  }
  *out = N;
  return PCLHIP_OK;
}

void pclhip_ndt_destroy(pclhip_ndt* N) {
  if (!N) return;
  pclhip_ctx* ctx = N->ctx;
  (void)hipStreamSynchronize(ctx->stream);
  ndt_drop_fitness(N, true);
  ndt_drop_cells(N);
  dev_free_if(ctx, N->tgt);
  dev_free_if(ctx, N->src);
  dev_free_if(ctx, N->src_sorted);
  dev_free_if(ctx, N->lists);
  N->sums.release(ctx);
  if (N->ev_a) (void)hipEventDestroy(N->ev_a);
  if (N->ev_b) (void)hipEventDestroy(N->ev_b);
  delete N;
}

pclhip_status pclhip_ndt_set_target(pclhip_ndt* N, const void* points, size_t stride, uint64_t n) {
  if (!N || (!points && n)) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = N->ctx;
  PCLHIP_REQUIRE(ctx, stride >= 12 && stride % 4 == 0, "stride must be a multiple of 4 and >= 12 bytes");
  PCLHIP_REQUIRE(ctx, n < 0x7FFFFFFFull, "cloud too large for int32 indices");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  ndt_drop_cells(N);  // ndt.h:121-141: a new target rebuilds the voxel grid
  ndt_drop_fitness(N, true);
  N->tgt_n = 0;
  const pclhip_status st = ndt_copy_records(ctx, points, stride, n, &N->tgt);
  if (st != PCLHIP_OK) return st;
  N->tgt_stride = stride;
  N->tgt_n = n;
  return PCLHIP_OK;
}

pclhip_status pclhip_ndt_set_source(pclhip_ndt* N, const void* points, size_t stride, uint64_t n) {
  if (!N || (!points && n)) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = N->ctx;
  PCLHIP_REQUIRE(ctx, stride >= 12 && stride % 4 == 0, "stride must be a multiple of 4 and >= 12 bytes");
  PCLHIP_REQUIRE(ctx, n < 0x7FFFFFFFull, "cloud too large for int32 indices");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  ndt_drop_fitness(N, false);
  N->src_n = 0;
  dev_free_if(ctx, N->src_sorted);
  dev_free_if(ctx, N->lists);
  N->src_sorted = nullptr;
  N->lists = nullptr;
  pclhip_status st = ndt_copy_records(ctx, points, stride, n, &N->src);
  if (st != PCLHIP_OK) return st;
  N->src_stride = stride;
  if (n == 0) return PCLHIP_OK;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &N->src_sorted, size_t(n) * sizeof(float4)));
  uint32_t n_finite = 0;
  float lo[3], hi[3];
  st = spatial_order(ctx, N->src, stride, n, nullptr, 0, N->src_sorted, uint32_t(n), &n_finite, lo, hi, true, nullptr);
  if (st != PCLHIP_OK) return st;
  // two blocks per CU at most (the kernels are bounded to two waves per SIMD); the same grid for the three variants:
  // a variant's sums then have the bits of the full pass
  const uint32_t ngroups = uint32_t((n + WAVE - 1) / WAVE);
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ndt_eval_kernel<true, true>, NDT_BLOCK, 0) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    per_cu = 2;
  }
  const uint64_t want = (uint64_t(ngroups) + NDT_WAVES - 1) / NDT_WAVES;
  const uint64_t cap = uint64_t(per_cu) * uint64_t(ctx->num_cus > 0 ? ctx->num_cus : 1);
  const int blocks = int(want < cap ? (want > 0 ? want : 1) : cap);
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &N->lists, size_t(blocks) * NDT_BLOCK * NDT_LIST_CAP * sizeof(uint32_t)));
  PCLHIP_CHECK_HIP(ctx, N->sums.resize(ctx, blocks));
  N->src_n = n;
  return PCLHIP_OK;
}

pclhip_status pclhip_ndt_set_trace(pclhip_ndt* N, pclhip_ndt_trace* buf, int capacity) {
  if (!N || capacity < 0 || (capacity > 0 && !buf)) return PCLHIP_ERR_INVALID;
  N->trace = buf;
  N->trace_capacity = capacity;
  return PCLHIP_OK;
}

// NormalDistributionsTransform::computeTransformation (impl/ndt.hpp:79-207) behind Registration::align
pclhip_status pclhip_ndt_align(pclhip_ndt* N, const pclhip_ndt_params* P, const float guess_in[16], pclhip_ndt_result* res) {
  if (!N || !P || !res) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = N->ctx;
  PCLHIP_REQUIRE(ctx, N->src_n > 0, "no input source dataset was given");
  if (P->neighborhood_search_method != PCLHIP_NDT_RADIUS) {
    set_error(ctx, "NormalDistributionsTransform: only the RADIUS neighbourhood is built (DIRECT27/26/7/1 are not)");
    return PCLHIP_ERR_STATE;
  }
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  std::memset(res, 0, sizeof *res);
  const auto t0 = std::chrono::steady_clock::now();
  pclhip_status st = ndt_ensure_cells(N, P, &res->cells_ms);
  if (st != PCLHIP_OK) return st;
  for (int v = 0; v < 3; ++v) {
    N->evals[v] = 0;
    N->eval_ms[v] = 0.0;
  }
  const float* guess = guess_in ? guess_in : kIdentity16;
  NdtState S;
  std::memcpy(S.final_T, kIdentity16, sizeof S.final_T);  // Registration::align: final_transformation_ = Identity
  float Tk[16];
  std::memcpy(Tk, kIdentity16, sizeof Tk);
  int nr = 0, ntrace = 0;
  bool converged = false;
  double score = 0.0;
  res->num_cells = N->cells.count;
  if (N->cells.count > 0) {  // else "Voxel grid is not searchable" (:86-90)
    double d1, d2;
    nf::gauss_constants(P->resolution, P->outlier_ratio, &d1, &d2);
    bool is_ident = true;
    for (int k = 0; k < 16; ++k) is_ident = is_ident && guess[k] == kIdentity16[k];
    if (!is_ident) std::memcpy(S.final_T, guess, sizeof S.final_T);
    double x[6];
    nf::euler_from(S.final_T, x);
    nf::NdtAngles A;
    nf::angle_tables(x, A);
    double sums[NDT_NS];
    st = ndt_eval(N, P, 0, S.final_T, A, d1, d2, sums);
    if (st != PCLHIP_OK) return st;
    ndt_unpack(sums, &S.score, S.g, S.H);
    while (!converged) {
      double delta[6], neg_g[6];
      for (int k = 0; k < 6; ++k) neg_g[k] = -S.g[k];
      ndt_newton_direction(S.H, neg_g, delta);
      double dn = 0.0;
      for (int k = 0; k < 6; ++k) dn += delta[k] * delta[k];
      dn = std::sqrt(dn);
      if (dn == 0 || dn != dn) {
        converged = dn == 0;
        break;
      }
      for (int k = 0; k < 6; ++k) delta[k] /= dn;
      int trials = 0;
      st = ndt_step_length(N, P, d1, d2, x, delta, dn, P->step_size, P->transformation_epsilon / 2, S, &dn, &trials);
      if (st != PCLHIP_OK) return st;
      for (int k = 0; k < 6; ++k) delta[k] *= dn;
      nf::convert_transform(delta, Tk);
      for (int k = 0; k < 6; ++k) x[k] += delta[k];
      const double cos_angle = 0.5 * double((Tk[0] + Tk[5] + Tk[10]) - 1.0f);
      const double tsq = double((Tk[3] * Tk[3] + Tk[7] * Tk[7]) + Tk[11] * Tk[11]);
      ++nr;
      if (ntrace < N->trace_capacity) {
        pclhip_ndt_trace& t = N->trace[ntrace++];
        t.step_length = dn;
        t.line_search_trials = trials;
        t.reserved = 0;
        t.score = S.score;
        std::memcpy(t.transformation, S.final_T, sizeof S.final_T);
      }
      const double te = P->transformation_epsilon, re = P->transformation_rotation_epsilon;
      if (nr >= P->max_iterations || ((te > 0 && tsq <= te) && (re > 0 && cos_angle >= re)) ||
          ((te <= 0) && (re > 0 && cos_angle >= re)) || ((te > 0 && tsq <= te) && (re <= 0)))
        converged = true;
    }
    score = S.score;
  }
  std::memcpy(res->final_transformation, S.final_T, sizeof S.final_T);
  std::memcpy(N->final_T, S.final_T, sizeof S.final_T);
  std::memcpy(res->last_transformation, Tk, sizeof Tk);
  res->nr_iterations = nr;
  res->converged = converged ? 1 : 0;
  res->score = score;
  res->transformation_likelihood = score / double(N->src_n);
  res->num_pairs = N->last_pairs;
  res->evaluations_full = N->evals[0];
  res->evaluations_gradient = N->evals[1];
  res->evaluations_hessian = N->evals[2];
  res->eval_ms_full = N->eval_ms[0];
  res->eval_ms_gradient = N->eval_ms[1];
  res->eval_ms_hessian = N->eval_ms[2];
  res->trace_count = ntrace;
  res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PCLHIP_OK;
}

pclhip_status pclhip_ndt_evaluate(pclhip_ndt* N, const pclhip_ndt_params* P, const double x[6], int variant, double* score,
                                  double g[6], double H[36], uint64_t* pairs) {
  if (!N || !P || !x || !score || !g || !H) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = N->ctx;
  PCLHIP_REQUIRE(ctx, variant >= 0 && variant <= 2, "variant: 0 full, 1 score + gradient, 2 Hessian");
  PCLHIP_REQUIRE(ctx, N->src_n > 0, "no input source dataset was given");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  pclhip_status st = ndt_ensure_cells(N, P, nullptr);
  if (st != PCLHIP_OK) return st;
  double d1, d2, sums[NDT_NS];
  nf::gauss_constants(P->resolution, P->outlier_ratio, &d1, &d2);
  float T[16];
  nf::convert_transform(x, T);
  nf::NdtAngles A;
  nf::angle_tables(x, A);
  st = ndt_eval(N, P, variant, T, A, d1, d2, sums);
  if (st != PCLHIP_OK) return st;
  ndt_unpack(sums, score, g, H);
  if (pairs) *pairs = N->last_pairs;
  return PCLHIP_OK;
}

pclhip_status pclhip_ndt_cells(pclhip_ndt* N, const pclhip_ndt_params* P, uint64_t* count, float* centroids, double* means,
                               double* cov, double* icov, int32_t* npoints, int32_t* voxel_ids, uint8_t* valid,
                               uint64_t capacity) {
  if (!N || !P || !count) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = N->ctx;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  pclhip_status st = ndt_ensure_cells(N, P, nullptr);
  if (st != PCLHIP_OK) return st;
  const size_t m = N->cells.count;
  *count = m;
  if (m == 0 || !(centroids || means || cov || icov || npoints || voxel_ids || valid)) return PCLHIP_OK;
  if (capacity < m) {
    set_error(ctx, "pclhip_ndt_cells: capacity too small (count holds the required size)");
    return PCLHIP_ERR_OVERFLOW;
  }
  std::vector<float> c4(m * 4);
  std::vector<double> rec(m * nf::kNdtCellDoubles);
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(c4.data(), N->cells.centroid, m * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(rec.data(), N->cells.rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (cov) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(cov, N->cells.cov, m * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (npoints) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(npoints, N->cells.npoints, m * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (voxel_ids) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(voxel_ids, N->cells.voxel, m * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (valid) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(valid, N->cells.valid, m, hipMemcpyDeviceToHost, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < m; ++i) {
    const double* r = &rec[i * nf::kNdtCellDoubles];
    if (centroids)
      for (int k = 0; k < 3; ++k) centroids[3 * i + k] = c4[4 * i + k];
    if (means)
      for (int k = 0; k < 3; ++k) means[3 * i + k] = r[k];
    if (icov) {
      const double* c = r + 3;
      const double full[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
      for (int k = 0; k < 9; ++k) icov[9 * i + k] = full[k];
    }
  }
  return PCLHIP_OK;
}

pclhip_status pclhip_ndt_fitness_score(pclhip_ndt* N, const float T[16], double max_range, double* score, uint64_t* nr) {
  if (!N || !score) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = N->ctx;
  PCLHIP_REQUIRE(ctx, N->tgt_n > 0 && N->src_n > 0, "the fitness score needs a target and a source");
  pclhip_status st = PCLHIP_OK;
  if (!N->tgt_index) {
    st = pclhip_index_build(ctx, N->tgt, N->tgt_stride, N->tgt_n, nullptr, 0, &N->tgt_index);
    if (st != PCLHIP_OK) return st;
  }
  if (!N->icp) {
    st = pclhip_icp_create(N->tgt_index, &N->icp);
    if (st != PCLHIP_OK) return st;
  }
  if (!N->icp_source_set) {
    st = pclhip_icp_set_source(N->icp, N->src, N->src_stride, N->src_n);
    if (st != PCLHIP_OK) return st;
    N->icp_source_set = true;
  }
  return pclhip_icp_fitness_score(N->icp, T ? T : N->final_T, max_range, score, nr);
}

}  // extern "C"
