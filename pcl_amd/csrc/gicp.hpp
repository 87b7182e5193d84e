// gicp.hpp -- GeneralizedIterativeClosestPoint::computeTransformation with the Newton solver
// (registration/include/pcl/registration/impl/gicp.hpp:370-477, 768-930).  Included by search.hip (the 1-NN search of an
// outer iteration is that file's seeded / stand-off ICP search with the transform fused in).
//
// Per outer iteration:
//   search      the working copy is reset to the guess-moved source, moved by transformation_ (Transformer order) and
//               matched (launch_icp_iterate, search only)
//   pack        gicp_pack_kernel: per pair the Mahalanobis matrix M = (R C_src R^T + C_tgt)^-1 (double, kept per source
//               point when det == 0), the pair written to one 80-byte record in source slot order (unmatched slots: a
//               zero record, which adds exactly nothing), and the 60 sums of dfddf that do not depend on x + the count
//   Newton      gicp_eval_kernel<10>: f at all ten line-search candidates x - 2^-j delta, and the 12 gradient sums at
//               alpha = 1; gicp_eval_kernel<1> (the gradient pass) only when a smaller alpha wins, or for x0
// Every pass streams the pair records once; the serial part (Hessian assembly, 6x6 eigen-solve, alpha, the gradient and
// delta tests: gicp_forms.hpp) runs on the host between passes.  Sums: per thread in a fixed order, then the fixed-order
// block sums of block_sums.hpp (rows of 64 doubles).
// From search.hip itself, which must have defined them above its #include of this file: the launch geometry BLOCK and
// WAVES_PER_BLOCK, and the launchers launch_icp_iterate and launch_gicp_covariances (declared in pclhip_internal.hpp).
#pragma once

#include <cfloat>
#include <chrono>

#include "block_sums.hpp"
#include "gicp_forms.hpp"
#include "icp_xform.hpp"

struct pclhip_gicp {
  pclhip_ctx* ctx = nullptr;
  pclhip_index* target = nullptr;
  pclhip_icp* icp = nullptr;           // search state on the target (working copy, matches, seeds)
  uint64_t n_src_orig = 0;
  double* src_cov = nullptr;           // [n_src_orig * 9] by original source index (NaN where none)
  double* tgt_cov = nullptr;           // [target->n_orig * 9] by original target index
  bool src_cov_user = false, tgt_cov_user = false;
  float4* moved = nullptr;             // [icp->n] the source moved by the guess, slot order
  double* mstore = nullptr;            // [icp->n * 6] Mahalanobis matrix per source slot (mahalanobis_)
  void* pairs = nullptr;               // [icp->n] GicpPair
  pclhip::BlockSums<64> sums;          // rows of the pack / evaluation passes
  bool have_pairs = false;
  double cached[pclhip::gf::kGicpCached] = {};  // of the last outer iteration
  pclhip_gicp_trace* trace = nullptr;
  int trace_capacity = 0;
  float final_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  int passes = 0;                      // evaluation passes of the last align
  hipEvent_t ev_a = nullptr, ev_b = nullptr;  // around every pack / evaluation pass (+ its finalize)
  double pack_ms = 0, eval_ms = 0;     // GPU time of those passes in the last align
};

namespace pclhip {

struct GicpPair {
  float4 p;      // source point moved by the guess (xyz)
  float4 q;      // matched target point (xyz)
  double m[6];   // M: m00 m01 m02 m11 m12 m22
};
static_assert(sizeof(GicpPair) == 80, "pair record");

struct GicpR {
  double r[9];
};
struct GicpXforms {
  Mat34 t[gf::kGicpCandidates];
};

__global__ __launch_bounds__(BLOCK) void gicp_move_kernel(const float4* __restrict__ src, uint32_t n, Mat34 g,
                                                          float4* __restrict__ moved, float4* __restrict__ cur) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = src[i];
  float4 o;  // transformPointCloud(output, output, guess): Transformer order
  o.x = xform_row(g.m[0], g.m[1], g.m[2], g.m[3], p.x, p.y, p.z, 1);
  o.y = xform_row(g.m[4], g.m[5], g.m[6], g.m[7], p.x, p.y, p.z, 1);
  o.z = xform_row(g.m[8], g.m[9], g.m[10], g.m[11], p.x, p.y, p.z, 1);
  o.w = p.w;
  moved[i] = o;
  cur[i] = o;
}

// the pairs of an outer iteration (impl/gicp.hpp:858-876) and the x-independent sums of dfddf (:660-679)
__global__ __launch_bounds__(BLOCK) void gicp_pack_kernel(IndexView ix, const float4* __restrict__ moved, uint32_t n,
                                                          const uint32_t* __restrict__ match_pos,
                                                          const double* __restrict__ src_cov,
                                                          const double* __restrict__ tgt_cov, GicpR R,
                                                          double* __restrict__ mstore, GicpPair* __restrict__ pairs,
                                                          double* __restrict__ partials) {
  double acc[gf::kGicpCached];
#pragma unroll
  for (int s = 0; s < gf::kGicpCached; ++s) acc[s] = 0.0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t pos = match_pos[i];
    GicpPair pr;
    if (pos == NO_INDEX) {
      pr.p = make_float4(0, 0, 0, 0);
      pr.q = pr.p;
#pragma unroll
      for (int k = 0; k < 6; ++k) pr.m[k] = 0.0;
      pairs[i] = pr;
      continue;
    }
    const float4 p = moved[i];
    const float4 q = ix.pts[pos];
    const double* c1 = src_cov + size_t(__float_as_uint(p.w)) * 9;
    const double* c2 = tgt_cov + size_t(__float_as_uint(q.w)) * 9;  // the match's original index rides in its point
    double C1[9], C2[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      C1[k] = c1[k];
      C2[k] = c2[k];
    }
    // R * C1 * R^T + C2 (Eigen: (R * C1) * R^T, each element a left-to-right dot product)
    double RC[9], A[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) RC[3 * r + c] = R.r[3 * r] * C1[c] + R.r[3 * r + 1] * C1[3 + c] + R.r[3 * r + 2] * C1[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        A[3 * r + c] = (RC[3 * r] * R.r[3 * c] + RC[3 * r + 1] * R.r[3 * c + 1] + RC[3 * r + 2] * R.r[3 * c + 2]) + C2[3 * r + c];
    double m[6];
    if (gf::invert3x3_sym(A, m) != 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) mstore[size_t(i) * 6 + k] = m[k];
    } else {  // the matrix held for this source point stays (identity the first time)
#pragma unroll
      for (int k = 0; k < 6; ++k) m[k] = mstore[size_t(i) * 6 + k];
    }
    pr.p = make_float4(p.x, p.y, p.z, 0.0f);
    pr.q = make_float4(q.x, q.y, q.z, 0.0f);
#pragma unroll
    for (int k = 0; k < 6; ++k) pr.m[k] = m[k];
    pairs[i] = pr;
    const double pb[3] = {double(p.x), double(p.y), double(p.z)};
    const double pp[6] = {pb[0] * pb[0], pb[0] * pb[1], pb[0] * pb[2], pb[1] * pb[1], pb[1] * pb[2], pb[2] * pb[2]};
    acc[0] += 1.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[1 + k] += m[k];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[7 + 6 * c + k] += pb[c] * m[k];
#pragma unroll
    for (int l = 0; l < 6; ++l)
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[25 + 6 * l + k] += m[k] * pp[l];
  }
  block_rows<gf::kGicpCached, WAVES_PER_BLOCK, 64>(acc, partials);
}

// f at NC transforms and, for the first, the 12 gradient sums (OptimizationFunctorWithIndices, impl/gicp.hpp:480-640):
// d = (T p)_float - q widened to double, Md, d'Md, p (Md)'
template <int NC>
__global__ __launch_bounds__(BLOCK) void gicp_eval_kernel(const GicpPair* __restrict__ pairs, uint32_t n, GicpXforms X,
                                                          double* __restrict__ partials) {
  constexpr int NS = NC + 12;
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const GicpPair pr = pairs[i];
    const double M00 = pr.m[0], M01 = pr.m[1], M02 = pr.m[2], M11 = pr.m[3], M12 = pr.m[4], M22 = pr.m[5];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float* t = X.t[j].m;
      const float tx = xform_row(t[0], t[1], t[2], t[3], pr.p.x, pr.p.y, pr.p.z, 0);
      const float ty = xform_row(t[4], t[5], t[6], t[7], pr.p.x, pr.p.y, pr.p.z, 0);
      const float tz = xform_row(t[8], t[9], t[10], t[11], pr.p.x, pr.p.y, pr.p.z, 0);
      const double d0 = double(__fsub_rn(tx, pr.q.x)), d1 = double(__fsub_rn(ty, pr.q.y)), d2 = double(__fsub_rn(tz, pr.q.z));
      const double md0 = M00 * d0 + M01 * d1 + M02 * d2;
      const double md1 = M01 * d0 + M11 * d1 + M12 * d2;
      const double md2 = M02 * d0 + M12 * d1 + M22 * d2;
      acc[j] += d0 * md0 + d1 * md1 + d2 * md2;
      if (j == 0) {
        const double pb[3] = {double(pr.p.x), double(pr.p.y), double(pr.p.z)};
        acc[NC + 0] += md0;
        acc[NC + 1] += md1;
        acc[NC + 2] += md2;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          acc[NC + 3 + 3 * r + 0] += pb[r] * md0;
          acc[NC + 3 + 3 * r + 1] += pb[r] * md1;
          acc[NC + 3 + 3 * r + 2] += pb[r] * md2;
        }
      }
    }
  }
  block_rows<NS, WAVES_PER_BLOCK, 64>(acc, partials);
}

__global__ void gicp_scatter_cov_kernel(const float4* __restrict__ pts, uint32_t n, const double* __restrict__ cov_sorted,
                                        uint64_t n_orig, double* __restrict__ dense) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = __float_as_uint(pts[i].w);
  if (o >= n_orig) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) dense[size_t(o) * 9 + k] = cov_sorted[size_t(i) * 9 + k];
}

__global__ void gicp_fetch_m_kernel(const float4* __restrict__ moved, uint32_t n, const double* __restrict__ mstore,
                                    uint64_t n_orig, double* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = __float_as_uint(moved[i].w);
  if (o >= n_orig) return;
  const double* m = mstore + size_t(i) * 6;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[size_t(o) * 9 + 3 * r + c] = m[gf::sym6(r, c)];
}

namespace {

// f at x - 2^-j delta for j < nc (nc = 1: at x itself) + the gradient sums at the first; out: nc + 12 doubles
pclhip_status gicp_eval(pclhip_gicp* G, int nc, const double (*xs)[6], double* out) {
  pclhip_ctx* ctx = G->ctx;
  GicpXforms X;
  for (int j = 0; j < nc; ++j) {
    float T[16];
    gf::apply_state(xs[j], T);
    X.t[j] = mat34_of(T);
  }
  const uint32_t n = G->icp->n;
  (void)hipEventRecord(G->ev_a, ctx->stream);
  if (nc == 1)
    hipLaunchKernelGGL(gicp_eval_kernel<1>, dim3(G->sums.blocks), dim3(BLOCK), 0, ctx->stream,
                       static_cast<const GicpPair*>(G->pairs), n, X, G->sums.partials);
  else
    hipLaunchKernelGGL(gicp_eval_kernel<gf::kGicpCandidates>, dim3(G->sums.blocks), dim3(BLOCK), 0, ctx->stream,
                       static_cast<const GicpPair*>(G->pairs), n, X, G->sums.partials);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  ++G->passes;
  const pclhip_status st = G->sums.read(ctx, nc + 12, out, G->ev_b);  // (synchronises: the pass's events are complete)
  float ms = 0;
  if (st == PCLHIP_OK && hipEventElapsedTime(&ms, G->ev_a, G->ev_b) == hipSuccess) G->eval_ms += ms;
  return st;
}

// dfddf at x: f / m, g, H from the cached sums and one gradient pass
pclhip_status gicp_dfddf(pclhip_gicp* G, const double x[6], double* f, double g[6], double H[36], double* E13 = nullptr) {
  double e[13];
  const double xs[1][6] = {{x[0], x[1], x[2], x[3], x[4], x[5]}};
  pclhip_status st = gicp_eval(G, 1, xs, e);
  if (st != PCLHIP_OK) return st;
  gf::assemble(G->cached, e, x, f, g, H);
  if (E13) std::memcpy(E13, e, sizeof e);
  return PCLHIP_OK;
}

pclhip_status gicp_alloc_source_state(pclhip_gicp* G) {
  pclhip_ctx* ctx = G->ctx;
  const uint32_t n = G->icp->n;
  dev_free_if(ctx, G->moved);
  dev_free_if(ctx, G->mstore);
  dev_free_if(ctx, G->pairs);
  G->moved = nullptr;
  G->mstore = nullptr;
  G->pairs = nullptr;
  const size_t nn = n ? n : 1;
  int blocks = int((uint64_t(n) + BLOCK - 1) / BLOCK);
  if (blocks > ctx->num_cus * 4) blocks = ctx->num_cus * 4;  // four workgroups (four waves per SIMD) per CU
  if (blocks < 1) blocks = 1;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &G->moved, nn * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &G->mstore, nn * 6 * sizeof(double)));
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &G->pairs, nn * sizeof(GicpPair)));
  PCLHIP_CHECK_HIP(ctx, G->sums.resize(ctx, blocks));
  // mahalanobis_.resize(N, Identity) (impl/gicp.hpp:773)
  std::vector<double> ident(nn * 6);
  for (size_t i = 0; i < nn; ++i) {
    double* m = &ident[i * 6];
    m[0] = m[3] = m[5] = 1.0;
    m[1] = m[2] = m[4] = 0.0;
  }
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(G->mstore, ident.data(), nn * 6 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  G->have_pairs = false;
  return PCLHIP_OK;
}

// computeCovariances (impl/gicp.hpp:70-147) of an index, by original point index
pclhip_status gicp_index_covariances(pclhip_index* ix, int k, double eps, uint64_t n_orig, double* dense) {
  pclhip_ctx* ctx = ix->ctx;
  if (uint64_t(k) > ix->n) {
    set_error(ctx, "GeneralizedIterativeClosestPoint: number of points in cloud is less than k_correspondences");
    return PCLHIP_ERR_INVALID;
  }
  PCLHIP_REQUIRE(ctx, k >= 1 && k <= 32, "k_correspondences must be in 1..32 on this path (reference default 20)");
  double* cov_sorted = nullptr;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &cov_sorted, size_t(ix->n ? ix->n : 1) * 9 * sizeof(double)));
  pclhip_status st = launch_gicp_covariances(ix, k, eps, cov_sorted);
  if (st == PCLHIP_OK) {
    (void)hipMemsetAsync(dense, 0xFF, size_t(n_orig) * 9 * sizeof(double), ctx->stream);  // NaN where no point
    hipLaunchKernelGGL(gicp_scatter_cov_kernel, dim3((ix->n + 255) / 256 + 1), dim3(256), 0, ctx->stream, ix->pts, ix->n,
                       cov_sorted, n_orig, dense);
    const hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, cov_sorted);
    PCLHIP_CHECK_HIP(ctx, e);
    PCLHIP_CHECK_HIP(ctx, es);
    return PCLHIP_OK;
  }
  (void)hipStreamSynchronize(ctx->stream);
  dev_free(ctx, cov_sorted);
  return st;
}

pclhip_status gicp_user_covariances(pclhip_gicp* G, const double* cov, uint64_t n, double** slot) {
  pclhip_ctx* ctx = G->ctx;
  dev_free_if(ctx, *slot);
  *slot = nullptr;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, slot, size_t(n ? n : 1) * 9 * sizeof(double)));
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(*slot, cov, size_t(n) * 9 * sizeof(double), hipMemcpyDefault, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PCLHIP_OK;
}

}  // namespace
}  // namespace pclhip

using namespace pclhip;

extern "C" {

void pclhip_gicp_params_default(pclhip_gicp_params* p) {
  if (!p) return;
  // registration/include/pcl/registration/gicp.h:136-152, 386-431
  p->max_iterations = 200;
  p->transformation_epsilon = 5e-4;
  p->rotation_epsilon = 2e-3;
  p->max_correspondence_distance = 5.0;
  p->min_number_correspondences = 4;
  p->k_correspondences = 20;
  p->gicp_epsilon = 1e-3;
  p->max_inner_iterations = 20;
  p->translation_gradient_tolerance = 1e-2;
  p->rotation_gradient_tolerance = 1e-2;
}

pclhip_status pclhip_gicp_create(pclhip_index* target, pclhip_gicp** out) {
  if (!target || !out) return PCLHIP_ERR_INVALID;
  *out = nullptr;
  pclhip_ctx* ctx = target->ctx;
  pclhip_icp* icp = nullptr;
  pclhip_status st = pclhip_icp_create(target, &icp);
  if (st != PCLHIP_OK) return st;
  pclhip_gicp* G = new pclhip_gicp();
  G->ctx = ctx;
  G->target = target;
  G->icp = icp;
  icp->order_override = 1;   // transformPointCloud: Transformer order
  icp->search_only = true;   // the GICP passes replace the ICP accumulation
  if (G->sums.create(ctx) != hipSuccess || hipEventCreate(&G->ev_a) != hipSuccess || hipEventCreate(&G->ev_b) != hipSuccess) {
    set_error(ctx, "allocation failed in pclhip_gicp_create");
    pclhip_gicp_destroy(G);
    return PCLHIP_ERR_HIP;
  }
  *out = G;
  return PCLHIP_OK;
}

void pclhip_gicp_destroy(pclhip_gicp* G) {
  if (!G) return;
  pclhip_ctx* ctx = G->ctx;
  (void)hipStreamSynchronize(ctx->stream);
  dev_free_if(ctx, G->src_cov);
  dev_free_if(ctx, G->tgt_cov);
  dev_free_if(ctx, G->moved);
  dev_free_if(ctx, G->mstore);
  dev_free_if(ctx, G->pairs);
  G->sums.release(ctx);
  if (G->ev_a) (void)hipEventDestroy(G->ev_a);
  if (G->ev_b) (void)hipEventDestroy(G->ev_b);
  if (G->icp) pclhip_icp_destroy(G->icp);
  delete G;
}

pclhip_status pclhip_gicp_set_source(pclhip_gicp* G, const void* points, size_t stride_bytes, uint64_t n) {
  if (!G || (!points && n)) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = G->ctx;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  pclhip_status st = pclhip_icp_set_source(G->icp, points, stride_bytes, n);
  if (st != PCLHIP_OK) return st;
  G->n_src_orig = n;
  dev_free_if(ctx, G->src_cov);  // setInputSource drops the source covariances (gicp.h:160-166)
  G->src_cov = nullptr;
  G->src_cov_user = false;
  return gicp_alloc_source_state(G);
}

pclhip_status pclhip_gicp_set_source_covariances(pclhip_gicp* G, const double* cov, uint64_t n) {
  if (!G || !cov) return PCLHIP_ERR_INVALID;
  PCLHIP_REQUIRE(G->ctx, G->icp->src_cur != nullptr && n == G->n_src_orig, "one covariance per source point, after the source");
  pclhip_status st = gicp_user_covariances(G, cov, n, &G->src_cov);
  G->src_cov_user = st == PCLHIP_OK;
  return st;
}

pclhip_status pclhip_gicp_set_target_covariances(pclhip_gicp* G, const double* cov, uint64_t n) {
  if (!G || !cov) return PCLHIP_ERR_INVALID;
  PCLHIP_REQUIRE(G->ctx, n == G->target->n_orig, "one covariance per target point");
  pclhip_status st = gicp_user_covariances(G, cov, n, &G->tgt_cov);
  G->tgt_cov_user = st == PCLHIP_OK;
  return st;
}

pclhip_status pclhip_gicp_set_trace(pclhip_gicp* G, pclhip_gicp_trace* buf, int capacity) {
  if (!G || capacity < 0 || (capacity > 0 && !buf)) return PCLHIP_ERR_INVALID;
  G->trace = buf;
  G->trace_capacity = capacity;
  return PCLHIP_OK;
}

// GeneralizedIterativeClosestPoint::computeTransformation (impl/gicp.hpp:768-930) with
// estimateRigidTransformationNewton (:370-477)
pclhip_status pclhip_gicp_align(pclhip_gicp* G, const pclhip_gicp_params* P, const float guess_in[16],
                                pclhip_gicp_result* res) {
  if (!G || !P || !res) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = G->ctx;
  pclhip_icp* icp = G->icp;
  PCLHIP_REQUIRE(ctx, icp->src_cur != nullptr, "no source cloud set");
  PCLHIP_REQUIRE(ctx, P->max_inner_iterations >= 1 && P->rotation_epsilon > 0 && P->transformation_epsilon > 0,
                 "invalid GICP parameters");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  std::memset(res, 0, sizeof *res);
  const float* guess = guess_in ? guess_in : kIdentity16;
  const auto t0 = std::chrono::steady_clock::now();
  // covariances once, cached (:775-784)
  double cov_ms = 0.0;
  if (G->tgt_cov == nullptr || G->src_cov == nullptr) {
    const auto c0 = std::chrono::steady_clock::now();
    if (G->tgt_cov == nullptr) {
      PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &G->tgt_cov, size_t(G->target->n_orig ? G->target->n_orig : 1) * 9 * sizeof(double)));
      pclhip_status st = gicp_index_covariances(G->target, P->k_correspondences, P->gicp_epsilon, G->target->n_orig, G->tgt_cov);
      if (st != PCLHIP_OK) {
        dev_free_if(ctx, G->tgt_cov);
        G->tgt_cov = nullptr;
        return st;
      }
    }
    if (G->src_cov == nullptr) {
      pclhip_index* six = nullptr;
      pclhip_status st = build_index_from_float4(ctx, icp->src_sorted0, icp->n_finite, &six);
      if (st != PCLHIP_OK) return st;
      PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &G->src_cov, size_t(G->n_src_orig ? G->n_src_orig : 1) * 9 * sizeof(double)));
      st = gicp_index_covariances(six, P->k_correspondences, P->gicp_epsilon, G->n_src_orig, G->src_cov);
      pclhip_index_destroy(six);
      if (st != PCLHIP_OK) {
        dev_free_if(ctx, G->src_cov);
        G->src_cov = nullptr;
        return st;
      }
    }
    cov_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  }
  // output moved by the guess (:795), the working copy reset to it before every search
  pclhip_status st = pclhip_icp_reset(icp);
  if (st != PCLHIP_OK) return st;
  const uint32_t n = icp->n;
  if (n > 0) {
    hipLaunchKernelGGL(gicp_move_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, icp->src_sorted0, n,
                       mat34_of(guess), G->moved, icp->src_cur);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  const double md2 = P->max_correspondence_distance * P->max_correspondence_distance;
  const bool use_max = md2 < double(FLT_MAX);
  float fmax2 = FLT_MAX;
  if (use_max) {  // largest float <= md2 (the reference compares in double)
    fmax2 = float(md2);
    if (double(fmax2) > md2) fmax2 = std::nextafterf(fmax2, 0.0f);
  }
  float Tk[16], Tprev[16];
  std::memcpy(Tk, kIdentity16, sizeof Tk);
  std::memcpy(Tprev, kIdentity16, sizeof Tprev);
  int nr = 0, newton_total = 0, alpha_one = 0, steps = 0, ntrace = 0;
  bool converged = false;
  uint64_t last_m = 0;
  G->passes = 0;
  G->pack_ms = G->eval_ms = 0;
  double search_ms = 0.0;
  while (!converged) {
    // R of the double product transformation_ * guess (:836-843)
    GicpR R;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double a = 0.0;
        for (int k = 0; k < 4; ++k) a += double(Tk[4 * i + k]) * double(guess[4 * k + j]);
        R.r[3 * i + j] = a;
      }
    if (nr > 0 && n > 0)
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(icp->src_cur, G->moved, size_t(n) * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    st = launch_icp_iterate(icp, Tk, fmax2, use_max, PCLHIP_ICP_POINT_TO_POINT);
    if (st != PCLHIP_OK) return st;
    if (n > 0) {
      (void)hipEventRecord(G->ev_a, ctx->stream);
      hipLaunchKernelGGL(gicp_pack_kernel, dim3(G->sums.blocks), dim3(BLOCK), 0, ctx->stream, G->target->view(), G->moved, n,
                         icp->match_pos, G->src_cov, G->tgt_cov, R, G->mstore, static_cast<GicpPair*>(G->pairs),
                         G->sums.partials);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
      st = G->sums.read(ctx, gf::kGicpCached, G->cached, G->ev_b);
      if (st != PCLHIP_OK) return st;
      float pms = 0;
      if (hipEventElapsedTime(&pms, G->ev_a, G->ev_b) == hipSuccess) G->pack_ms += pms;
      float ms = 0;
      if (hipEventElapsedTime(&ms, icp->ev0, icp->ev1) == hipSuccess) search_ms += ms;
    } else {
      std::memset(G->cached, 0, sizeof G->cached);
    }
    G->have_pairs = true;
    last_m = uint64_t(G->cached[0]);
    std::memcpy(Tprev, Tk, sizeof Tk);  // previous_transformation_ = transformation_ (:879)
    if (last_m < uint64_t(P->min_number_correspondences > 0 ? P->min_number_correspondences : 0))
      break;  // NotEnoughPointsException: the loop ends without converging (:897-901)
    // estimateRigidTransformationNewton
    double x[6], g[6], H[36], f = 0.0;
    gf::state_from(Tk, x);
    st = gicp_dfddf(G, x, &f, g, H);
    if (st != PCLHIP_OK) return st;
    int inner = 0;
    do {
      ++inner;
      double delta[6];
      gf::newton_step(H, g, delta);
      double xs[gf::kGicpCandidates][6];
      double alpha = 1.0;
      for (int j = 0; j < gf::kGicpCandidates; ++j, alpha /= 2)
        for (int k = 0; k < 6; ++k) xs[j][k] = x[k] - alpha * delta[k];
      double e[gf::kGicpCandidates + 12];
      st = gicp_eval(G, gf::kGicpCandidates, xs, e);
      if (st != PCLHIP_OK) return st;
      ++steps;
      int won = -1;
      for (int j = 0; j < gf::kGicpCandidates; ++j)
        if (e[j] / G->cached[0] < f) {
          won = j;
          break;
        }
      if (won < 0) break;  // no progress
      std::memcpy(x, xs[won], sizeof x);
      if (won == 0) {
        ++alpha_one;
        double E[13];
        E[0] = e[0];
        for (int k = 0; k < 12; ++k) E[1 + k] = e[gf::kGicpCandidates + k];
        gf::assemble(G->cached, E, x, &f, g, H);
      } else {
        st = gicp_dfddf(G, x, &f, g, H);
        if (st != PCLHIP_OK) return st;
      }
      const double gt = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
      const double gr = std::sqrt(g[3] * g[3] + g[4] * g[4] + g[5] * g[5]);
      if (gt < P->translation_gradient_tolerance && gr < P->rotation_gradient_tolerance) break;
    } while (inner < P->max_inner_iterations);
    newton_total += inner;
    gf::apply_state(x, Tk);  // transformation_matrix.setIdentity(); applyState (:475-476)
    double delta = 0.0;  // :884-896
    for (int k = 0; k < 4; ++k)
      for (int l = 0; l < 4; ++l) {
        const double ratio = (k < 3 && l < 3) ? 1.0 / P->rotation_epsilon : 1.0 / P->transformation_epsilon;
        const double c = ratio * double(std::fabs(Tprev[4 * k + l] - Tk[4 * k + l]));
        if (c > delta) delta = c;
      }
    ++nr;
    if (ntrace < G->trace_capacity) {
      pclhip_gicp_trace& t = G->trace[ntrace++];
      t.correspondences = last_m;
      t.inner_iterations = inner;
      t.f = f;
      std::memcpy(t.transformation, Tk, sizeof Tk);
    }
    if (nr >= P->max_iterations || delta < 1) {
      converged = true;
      std::memcpy(Tprev, Tk, sizeof Tk);
    }
  }
  cf::mat4_mul_f32(Tprev, guess, res->final_transformation);  // final = previous_transformation_ * guess (:905)
  std::memcpy(G->final_T, res->final_transformation, sizeof G->final_T);
  std::memcpy(res->last_transformation, Tk, sizeof Tk);
  res->nr_iterations = nr;
  res->converged = converged ? 1 : 0;
  res->num_correspondences = last_m;
  res->newton_iterations = newton_total;
  res->newton_steps_alpha_one = alpha_one;
  res->newton_steps = steps;
  res->eval_passes = G->passes;
  res->trace_count = ntrace;
  res->covariance_ms = cov_ms;
  res->search_ms = search_ms;
  res->pack_ms = G->pack_ms;
  res->eval_ms = G->eval_ms;
  res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PCLHIP_OK;
}

pclhip_status pclhip_gicp_evaluate(pclhip_gicp* G, const double x[6], double* f, double g[6], double H[36]) {
  if (!G || !x || !f || !g || !H) return PCLHIP_ERR_INVALID;
  PCLHIP_REQUIRE(G->ctx, G->have_pairs && G->cached[0] > 0, "no pairs: align first");
  PCLHIP_CHECK_HIP(G->ctx, hipSetDevice(G->ctx->device));
  return gicp_dfddf(G, x, f, g, H);
}

pclhip_status pclhip_gicp_mahalanobis(pclhip_gicp* G, double* out) {
  if (!G || !out) return PCLHIP_ERR_INVALID;
  pclhip_ctx* ctx = G->ctx;
  PCLHIP_REQUIRE(ctx, G->mstore != nullptr, "no source cloud set");
  const uint32_t n = G->icp->n;
  const size_t bytes = size_t(G->n_src_orig) * 9 * sizeof(double);
  double* d = nullptr;
  PCLHIP_CHECK_HIP(ctx, dev_malloc(ctx, &d, bytes ? bytes : 8));
  (void)hipMemsetAsync(d, 0xFF, bytes, ctx->stream);
  if (n > 0)
    hipLaunchKernelGGL(gicp_fetch_m_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, G->moved, n, G->mstore,
                       G->n_src_orig, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, bytes, hipMemcpyDefault, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  dev_free(ctx, d);
  PCLHIP_CHECK_HIP(ctx, e);
  PCLHIP_CHECK_HIP(ctx, es);
  return PCLHIP_OK;
}

pclhip_status pclhip_gicp_fitness_score(pclhip_gicp* G, const float T[16], double max_range, double* score, uint64_t* nr) {
  if (!G || !score) return PCLHIP_ERR_INVALID;
  return pclhip_icp_fitness_score(G->icp, T ? T : G->final_T, max_range, score, nr);
}

}  // extern "C"
