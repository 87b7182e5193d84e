// sac_models.hpp -- the plane models of SACSegmentation beyond SACMODEL_PLANE: the gate per hypothesis of
// SACMODEL_PERPENDICULAR_PLANE, SACMODEL_PARALLEL_PLANE and SACMODEL_NORMAL_PARALLEL_PLANE (sample_consensus/.../impl/
// sac_model_perpendicular_plane.hpp:93-119, sac_model_parallel_plane.hpp:92-115, sac_model_normal_parallel_plane.hpp:48-78)
// and the distance of SACMODEL_NORMAL_PLANE (impl/sac_model_normal_plane.hpp:48-101,128-162, the standard path); the
// semantics are stated in include/pclhip.h.  Included by radius.hip after sac.hpp, whose gather, hypothesis, count, flag,
// list, moment and refit kernels it uses; the call itself (sac_segment_run) serves pclhip_sac_segment_plane as well.
//
// Beyond the plane's launches, per call:
//   sac_normals_gather_kernel  the point set's normals once: normalised (Eigen's normalized(), float) and the weight
//                              ndw * (1 - curvature) in double; a NaN in either makes the weight NaN (never an inlier)
// per batch:
//   sac_prepare_kernel         one thread per hypothesis: the gate's bit and the normalised plane normal; an invalid
//                              hypothesis gets d = NaN in the scoring array, so the scoring passes pass over it as over a
//                              skipped one (the trace keeps its d)
//   sac_normal_count_kernel    models 11 and 16, the shape of sac_count_kernel: SACN_P points of a lane in registers with
//                              their unit normals and weights, wave-uniform hypothesis reads, ballots into per-hypothesis
//                              counters.  Per pair t = (1 - w) d_euclid in double and an interval [lo, hi] of the folded
//                              angle from a float polynomial (below), then
//                                w hi + t < thr                   in
//                                w lo + t >= thr                  out
//                              and the double acos for the lanes that are left: their slots are bits of a lane mask, and a
//                              wave none of whose lanes has a bit skips that code (one copy of it, not one per slot).
// Why the screen never changes a flag: rounding is monotonic.  With w >= 0 and lo <= d_normal <= hi,
// fl(fl(w lo) + t) <= fl(fl(w d_normal) + t) <= fl(fl(w hi) + t), so a bound below thr puts the exact value below thr and
// a bound at or above it puts the exact value there: no error term enters.  What has to hold is lo <= d_normal <= hi for
// the d_normal of the exact path (the device's double acos, folded).  The interval: 0 <= d_normal <= HI = pi/2 + 150 ulp;
// and acos(x) = sqrt(1 - x) (a0 + a1 x + a2 x^2 + a3 x^3) + e(x) on [0, 1] (Abramowitz & Stegun 4.4.45) at x = min(|rad|, 1).
// The handbook gives |e| <= 5e-5; the largest error is 6.76e-5, at x = 0 (pi/2 - a0), and the float evaluation (one sqrtf,
// seven roundings of values <= 1.6) adds less than 1e-6: tests/test_sac_models_restatement.py walks the float polynomial
// over [0, 1] and holds it below SACN_D - 2e-6, SACN_D = 7.5e-5 being the interval's half width.  The double acos and
// the fold min(a, pi - a) = acos(|rad|) add less than 1e-14.  A weight outside [0, 1] takes the exact path always, and so
// does a NaN dot.
#pragma once

#include "sac.hpp"

namespace pclhip {
namespace {

constexpr int SACN_P = 8;                       // points a lane keeps (10 registers each: point, unit normal, w, 1 - w)
constexpr int SACN_TILE = SAC_BLOCK * SACN_P;
constexpr double SACN_HI = 1.5707963267949;     // pi/2 = 1.5707963267948966...: above every folded angle
constexpr float SACN_D = 7.5e-5f;               // half width of the polynomial's interval

struct SacGate {
  int model;
  int angle_on;        // eps_angle > 0
  int dist_on;         // model 16 with eps_dist > 0
  float ax, ay, az;
  double eps_angle;
  double sin_cos;      // |sin(eps_angle)| for model 15, |cos(eps_angle)| for model 16 (the host's)
  double dfo, eps_dist;
};

// the one order of a float sum of three products (include/pclhip.h)
__host__ __device__ inline float sac_dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(az, bz)), __fmul_rn(ay, by));
}

// Eigen's normalized(): v / sqrt(|v|^2) when |v|^2 > 0, else v
__device__ inline void sac_normalized(float& x, float& y, float& z) {
  const float q = sac_dot3(x, y, z, x, y, z);
  if (q > 0.0f) {
    const float r = sqrtf(q);
    x = __fdiv_rn(x, r); y = __fdiv_rn(y, r); z = __fdiv_rn(z, r);
  }
}

// getAngle3D (common/include/pcl/common/impl/common.hpp:47-56) of two normalised vectors' float dot, folded
__device__ inline double sac_folded_angle(float rad) {
  double r = double(rad);
  if (r < -1.0) r = -1.0;
  else if (r > 1.0) r = 1.0;
  const double a = acos(r);
  const double b = M_PI - a;
  return b < a ? b : a;
}

// isModelValid of (a, b, c, d); (ux, uy, uz): normalized((a, b, c))
__device__ inline bool sac_gate_valid(const SacGate& g, float ux, float uy, float uz, float d) {
  if (g.angle_on) {
    if (g.model == PCLHIP_SACMODEL_PERPENDICULAR_PLANE) {
      float ax = g.ax, ay = g.ay, az = g.az;
      sac_normalized(ax, ay, az);
      if (sac_folded_angle(sac_dot3(ax, ay, az, ux, uy, uz)) > g.eps_angle) return false;
    } else if (g.model == PCLHIP_SACMODEL_PARALLEL_PLANE) {
      if (double(__builtin_fabsf(sac_dot3(g.ax, g.ay, g.az, ux, uy, uz))) > g.sin_cos) return false;
    } else if (g.model == PCLHIP_SACMODEL_NORMAL_PARALLEL_PLANE) {
      if (double(__builtin_fabsf(sac_dot3(g.ax, g.ay, g.az, ux, uy, uz))) < g.sin_cos) return false;
    }
  }
  if (g.dist_on && fabs(double(-d) - g.dfo) > g.eps_dist) return false;
  return true;
}

// acos on [0, 1] to 6.8e-5 (Abramowitz & Stegun 4.4.45), in float: the screen's centre
__device__ inline float sac_acos_poly(float x) {
  float p = -0.0187293f * x + 0.0742610f;
  p = p * x + -0.2121144f;
  p = p * x + 1.5707288f;
  return sqrtf(1.0f - x) * p;
}

// the distance test of impl/sac_model_normal_plane.hpp:82-94 from its float parts
__device__ inline bool sac_normal_inlier(float rad, double de, double w, double om, double thr) {
  return fabs(w * sac_folded_angle(rad) + om * de) < thr;
}

__global__ __launch_bounds__(SAC_BLOCK) void sac_normals_gather_kernel(const char* __restrict__ rec, size_t stride,
                                                                       uint64_t n_rec, const int32_t* __restrict__ idx,
                                                                       uint32_t n, double ndw, float4* __restrict__ nn,
                                                                       double* __restrict__ wt) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t r = idx ? int64_t(idx[i]) : int64_t(i);
  float x = __builtin_nanf(""), y = x, z = x;
  double w = __builtin_nan("");
  if (r >= 0 && uint64_t(r) < n_rec) {  // (an index outside the cloud: sac_gather_kernel has flagged it)
    const float* p = reinterpret_cast<const float*>(rec + size_t(r) * stride);
    x = p[0]; y = p[1]; z = p[2];
    w = ndw * (1.0 - double(p[3]));
    sac_normalized(x, y, z);
    if (!(x == x && y == y && z == z)) w = __builtin_nan("");
  }
  nn[i] = make_float4(x, y, z, 0.0f);
  wt[i] = w;
}

// rec: the batch's trace records (null for given coefficients).  valid[t], unit[t]; models[t].w = NaN when invalid.
__global__ __launch_bounds__(SAC_BLOCK) void sac_prepare_kernel(SacGate g, uint32_t H,
                                                                const pclhip_sac_plane_trace* __restrict__ rec,
                                                                float4* __restrict__ models, float4* __restrict__ unit,
                                                                uint32_t* __restrict__ valid) {
  const uint32_t t = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (t >= H) return;
  float4 m = models[t];
  if (rec != nullptr) m.w = rec[t].coefficients[3];
  float ux = m.x, uy = m.y, uz = m.z;
  sac_normalized(ux, uy, uz);
  const bool ok = !(rec != nullptr && rec[t].skipped != 0) && sac_gate_valid(g, ux, uy, uz, m.w);
  unit[t] = make_float4(ux, uy, uz, 0.0f);
  valid[t] = ok ? 1u : 0u;
  if (!ok) models[t].w = __builtin_nanf("");
}

// the gate on the coefficients the device holds (before a selection): st->invalid
__global__ void sac_gate_held_kernel(SacGate g, SacDev* __restrict__ st) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float ux = st->coef[0], uy = st->coef[1], uz = st->coef[2];
  sac_normalized(ux, uy, uz);
  st->invalid = sac_gate_valid(g, ux, uy, uz, st->coef[3]) ? 0u : 1u;
}

#ifdef PCLHIP_SAC_SCREEN_STATS
__device__ unsigned long long sac_exact_pairs;  // pairs that took the double acos (scripts/sac_models_timing.py's build)
#endif

// countWithinDistance of H normal-plane models at once.  counts[] is zero before the launch.
__global__ __launch_bounds__(SAC_BLOCK) void sac_normal_count_kernel(const float4* __restrict__ pts,
                                                                     const float4* __restrict__ nn,
                                                                     const double* __restrict__ wt, uint32_t n,
                                                                     const float4* __restrict__ models,
                                                                     const float4* __restrict__ unit, uint32_t H,
                                                                     double thr, uint32_t* __restrict__ counts) {
  __shared__ uint32_t cnt_s[SAC_MAX_BATCH];
  for (uint32_t h = threadIdx.x; h < H; h += SAC_BLOCK) cnt_s[h] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint32_t tiles = (n + SACN_TILE - 1) / SACN_TILE;
  const float nanf_ = __builtin_nanf("");
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // slot k of lane l is point base + k * 64 + l (coalesced); past the end: a NaN weight, never inside
    const uint32_t base = tile * uint32_t(SACN_TILE) + wave * uint32_t(SACN_P * WAVE) + lane;
    float px[SACN_P], py[SACN_P], pz[SACN_P], nx[SACN_P], ny[SACN_P], nz[SACN_P];
    double w[SACN_P], om[SACN_P];
    [[maybe_unused]] uint32_t exact_only = 0u;  // bit k: the weight of slot k lies outside [0, 1]
#pragma unroll
    for (int k = 0; k < SACN_P; ++k) {
      const uint32_t i = base + uint32_t(k) * WAVE;
      float4 q = make_float4(nanf_, nanf_, nanf_, 0.0f), u = q;
      double wk = __builtin_nan("");
      if (i < n) { q = pts[i]; u = nn[i]; wk = wt[i]; }
      px[k] = q.x; py[k] = q.y; pz[k] = q.z;
      nx[k] = u.x; ny[k] = u.y; nz[k] = u.z;
      w[k] = wk; om[k] = 1.0 - wk;
      if (wk == wk && !(wk >= 0.0 && wk <= 1.0)) exact_only |= 1u << k;
    }
    for (uint32_t h0 = 0; h0 < H; h0 += WAVE) {
      const uint32_t hn = H - h0 < uint32_t(WAVE) ? H - h0 : uint32_t(WAVE);
      uint32_t mine = 0u;  // lane j: the wave's count of hypothesis h0 + j
      for (uint32_t j = 0; j < hn; ++j) {
        const float4 m = models[h0 + j];  // (the same for the wave: scalar loads)
        if (!(__builtin_fabsf(m.w) <= FLT_MAX)) continue;  // skipped, invalid, or a d that is not finite: counts 0
        const float4 c = unit[h0 + j];
        uint32_t inbits = 0u, askbits = 0u;  // bit k: slot k is inside; slot k needs the double acos
#pragma unroll
        for (int k = 0; k < SACN_P; ++k) {
          const float e = __fadd_rn(sac_dot3(m.x, m.y, m.z, px[k], py[k], pz[k]), m.w);
          const double t = om[k] * double(__builtin_fabsf(e));
#ifdef PCLHIP_SAC_NO_SCREEN
          askbits |= 1u << k;
#else
          const float rad = sac_dot3(nx[k], ny[k], nz[k], c.x, c.y, c.z);
          const float p = sac_acos_poly(fminf(__builtin_fabsf(rad), 1.0f));
          const double lo = double(fmaxf(p - SACN_D, 0.0f));
          const double hi = fmin(double(p + SACN_D), SACN_HI);
          const bool bounded = ((exact_only >> k) & 1u) == 0u && rad == rad;
          const bool in = bounded && w[k] * hi + t < thr;
          const bool out = bounded && w[k] * lo + t >= thr;
          inbits |= in ? 1u << k : 0u;
          askbits |= !in && !out && t == t ? 1u << k : 0u;  // (a NaN t: a NaN distance, outside)
#endif
        }
        while (__builtin_amdgcn_ballot_w64(askbits != 0u) != 0ull) {  // rare with the screen: one slot of a lane per turn
          if (askbits != 0u) {
            const int sel = __builtin_ctz(askbits);
            askbits &= askbits - 1u;
            float sx = 0.0f, sy = 0.0f, sz = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f;
            double sw = 0.0;
#pragma unroll
            for (int k = 0; k < SACN_P; ++k) {
              if (k == sel) { sx = px[k]; sy = py[k]; sz = pz[k]; tx = nx[k]; ty = ny[k]; tz = nz[k]; sw = w[k]; }
            }
            const float e = __fadd_rn(sac_dot3(m.x, m.y, m.z, sx, sy, sz), m.w);
            const bool in = sac_normal_inlier(sac_dot3(tx, ty, tz, c.x, c.y, c.z), double(__builtin_fabsf(e)), sw, 1.0 - sw, thr);
            inbits |= in ? 1u << sel : 0u;
#ifdef PCLHIP_SAC_SCREEN_STATS
            atomicAdd(&sac_exact_pairs, 1ull);
#endif
          }
        }
        uint32_t cw = 0u;
#pragma unroll
        for (int k = 0; k < SACN_P; ++k) cw += uint32_t(__popcll(__builtin_amdgcn_ballot_w64(((inbits >> k) & 1u) != 0u)));
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

// selectWithinDistance of the normal models as flags by position, with the coefficients the device holds
__global__ __launch_bounds__(SAC_BLOCK) void sac_normal_flag_kernel(const float4* __restrict__ pts,
                                                                    const float4* __restrict__ nn,
                                                                    const double* __restrict__ wt, uint32_t n,
                                                                    const SacDev* __restrict__ st, double thr,
                                                                    uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float a = st->coef[0], b = st->coef[1], c = st->coef[2], d = st->coef[3];
  float ux = a, uy = b, uz = c;
  sac_normalized(ux, uy, uz);
  const float4 p = pts[i], u = nn[i];
  const double w = wt[i];
  const double de = double(__builtin_fabsf(__fadd_rn(sac_dot3(a, b, c, p.x, p.y, p.z), d)));
  const bool in = sac_normal_inlier(sac_dot3(u.x, u.y, u.z, ux, uy, uz), de, w, 1.0 - w, thr);
  flag[i] = st->invalid == 0u && in ? 1u : 0u;
}

// what a call holds beyond the plane's
struct SacModel {
  SacGate gate;
  bool gated = false;    // a gate is on
  bool normal = false;   // models 11 and 16: the distance with the normals
  float4* nn = nullptr;  // the point set's unit normals and weights
  double* wt = nullptr;
  float4* unit = nullptr;    // per batch: the hypotheses' unit normals, the gate's bits
  uint32_t* valid = nullptr;
  bool prepares() const { return gated || normal; }
};

// the model's parameters checked, the normals staged, the batch arrays (cap hypotheses)
pclhip_status sac_model_setup(pclhip_ctx* ctx, DeviceScope& scope, const pclhip_sac_model_params* MP, const void* normals,
                              size_t nstride, uint64_t n_rec, const SacCloud& pc, int cap, SacModel* M) {
  hipStream_t s = ctx->stream;
  const int t = MP->model_type;
  PCLHIP_REQUIRE(ctx, t == PCLHIP_SACMODEL_PLANE || t == PCLHIP_SACMODEL_PERPENDICULAR_PLANE || t == PCLHIP_SACMODEL_NORMAL_PLANE ||
                      t == PCLHIP_SACMODEL_PARALLEL_PLANE || t == PCLHIP_SACMODEL_NORMAL_PARALLEL_PLANE,
                 "the model type must be SACMODEL_PLANE (0), PERPENDICULAR_PLANE (9), NORMAL_PLANE (11), PARALLEL_PLANE (15) or "
                 "NORMAL_PARALLEL_PLANE (16)");
  M->normal = t == PCLHIP_SACMODEL_NORMAL_PLANE || t == PCLHIP_SACMODEL_NORMAL_PARALLEL_PLANE;
  const bool has_axis = t == PCLHIP_SACMODEL_PERPENDICULAR_PLANE || t == PCLHIP_SACMODEL_PARALLEL_PLANE ||
                        t == PCLHIP_SACMODEL_NORMAL_PARALLEL_PLANE;
  SacGate& g = M->gate;
  std::memset(&g, 0, sizeof g);
  g.model = t;
  g.angle_on = has_axis && MP->eps_angle > 0.0 ? 1 : 0;
  g.dist_on = t == PCLHIP_SACMODEL_NORMAL_PARALLEL_PLANE && MP->eps_dist > 0.0 ? 1 : 0;
  g.ax = MP->axis[0]; g.ay = MP->axis[1]; g.az = MP->axis[2];
  g.eps_angle = MP->eps_angle;
  g.sin_cos = t == PCLHIP_SACMODEL_PARALLEL_PLANE ? std::fabs(std::sin(MP->eps_angle)) : std::fabs(std::cos(MP->eps_angle));
  g.dfo = MP->distance_from_origin;
  g.eps_dist = MP->eps_dist;
  M->gated = g.angle_on != 0 || g.dist_on != 0;
  PCLHIP_REQUIRE(ctx, !g.angle_on || g.ax != 0.0f || g.ay != 0.0f || g.az != 0.0f, "eps_angle > 0 needs an axis that is not zero");
  PCLHIP_REQUIRE(ctx, !M->normal || normals != nullptr || n_rec == 0, "this model type needs the normals");
  if (M->normal) PCLHIP_REQUIRE(ctx, nstride >= 16 && nstride % 4 == 0, "normals stride must be a multiple of 4 and >= 16 bytes");
  if (M->prepares()) {
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&M->unit, size_t(cap) * sizeof(float4)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&M->valid, size_t(cap) * 4));
  }
  if (M->normal && pc.n > 0) {
    const void* dn = nullptr;
    void* owned = nullptr;
    pclhip_status rc = to_device(ctx, normals, size_t(n_rec) * nstride, &dn, &owned);
    if (rc != PCLHIP_OK) return rc;
    if (owned) scope.mem.push_back(owned);
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&M->nn, size_t(pc.n) * sizeof(float4)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&M->wt, size_t(pc.n) * sizeof(double)));
    hipLaunchKernelGGL(sac_normals_gather_kernel, sac_blocks_of(pc.n), dim3(SAC_BLOCK), 0, s, static_cast<const char*>(dn), nstride,
                       n_rec, pc.idx, pc.n, MP->normal_distance_weight, M->nn, M->wt);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  return PCLHIP_OK;
}

uint32_t sac_normal_count_grid(const pclhip_ctx* ctx, uint32_t n) {
  static int per_cu = 0;
  if (per_cu == 0) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, sac_normal_count_kernel, SAC_BLOCK, 0) != hipSuccess || v < 1) {
      (void)hipGetLastError();
      v = 4;
    }
    per_cu = v;
  }
  const uint64_t tiles = (uint64_t(n) + SACN_TILE - 1) / SACN_TILE;
  const uint64_t most = uint64_t(per_cu) * uint64_t(ctx->num_cus > 0 ? ctx->num_cus : 1);
  return uint32_t(tiles < most ? (tiles > 0 ? tiles : 1) : most);
}

// the gate and the scoring pass of H hypotheses in `models`; counts[] is zero before it on the stream
void sac_score(const pclhip_ctx* ctx, const SacModel& M, const SacCloud& pc, const pclhip_sac_plane_trace* rec, float4* models,
               uint32_t H, double threshold, uint32_t* counts, hipEvent_t ea, hipEvent_t eb) {
  hipStream_t s = ctx->stream;
  if (M.prepares())
    hipLaunchKernelGGL(sac_prepare_kernel, sac_blocks_of(H), dim3(SAC_BLOCK), 0, s, M.gate, H, rec, models, M.unit, M.valid);
  if (ea) (void)hipEventRecord(ea, s);
  if (M.normal)
    hipLaunchKernelGGL(sac_normal_count_kernel, dim3(sac_normal_count_grid(ctx, pc.n)), dim3(SAC_BLOCK), 0, s, pc.pts, M.nn, M.wt,
                       pc.n, models, M.unit, H, threshold, counts);
  else
    hipLaunchKernelGGL(sac_count_kernel, dim3(sac_count_grid(ctx, pc.n)), dim3(SAC_BLOCK), 0, s, pc.pts, pc.n, models, H,
                       float(threshold), counts);
  if (eb) (void)hipEventRecord(eb, s);
}

// SACSegmentation::segment for every model (MP null: SACMODEL_PLANE); `fn` names the entry point in messages
pclhip_status sac_segment_run(pclhip_ctx* ctx, const char* fn, const void* cloud, uint64_t n_rec, size_t stride,
                              const void* normals, size_t nstride, const int32_t* indices, uint64_t n_indices,
                              const pclhip_sac_plane_params* P, const pclhip_sac_model_params* MP, float out_coeff[4],
                              int32_t* out_inliers, uint64_t inliers_capacity, uint64_t* out_n_inliers, int32_t* out_outliers,
                              uint64_t outliers_capacity, uint64_t* out_n_outliers, pclhip_sac_plane_stats* out_stats) {
  if (!ctx || !P || !out_coeff || !out_n_inliers) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *out_n_inliers = 0;
  if (out_n_outliers) *out_n_outliers = 0;
  for (int i = 0; i < 4; ++i) out_coeff[i] = 0.0f;
  pclhip_sac_plane_stats stats;
  std::memset(&stats, 0, sizeof stats);
  stats.best_trial = -1;
  if (out_stats) *out_stats = stats;
  ctx->sac_trace.clear();
  ctx->sac_trace_valid.clear();
  pclhip_status rc = sac_checked_params(ctx, cloud, n_rec, stride, indices, n_indices);
  if (rc != PCLHIP_OK) return rc;
  PCLHIP_REQUIRE(ctx, P->max_iterations >= 0 && P->max_iterations <= 100000000, "max_iterations must be in 0 .. 1e8");
  PCLHIP_REQUIRE(ctx, P->probability >= 0.0 && P->probability <= 1.0, "the probability must be in [0, 1]");
  PCLHIP_REQUIRE(ctx, P->batch_size >= 0 && P->batch_size <= SAC_MAX_BATCH, "batch_size must be in 0 .. 1024");
  PCLHIP_REQUIRE(ctx, (out_inliers != nullptr || inliers_capacity == 0) && (out_outliers != nullptr || outliers_capacity == 0),
                 "a capacity without a buffer");
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DeviceScope scope(ctx);
  hipEvent_t ev_call[2] = {nullptr, nullptr};
  PCLHIP_CHECK_HIP(ctx, scope.event(&ev_call[0]));
  PCLHIP_CHECK_HIP(ctx, scope.event(&ev_call[1]));
  (void)hipEventRecord(ev_call[0], s);
  SacDev* st = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&st, sizeof(SacDev)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(st, 0, sizeof(SacDev), s));
  SacCloud pc;
  if ((rc = sac_stage(ctx, scope, cloud, n_rec, stride, indices, n_indices, st, &pc)) != PCLHIP_OK) return rc;
  const uint32_t n = pc.n;
  const float thr = float(P->distance_threshold);
  const int cap = P->batch_size > 0 ? P->batch_size : SAC_MAX_BATCH;
  SacModel M;
  if (MP != nullptr && (rc = sac_model_setup(ctx, scope, MP, normals, nstride, n_rec, pc, cap, &M)) != PCLHIP_OK) return rc;

  // ---- the trials ----
  sac::Replay rp;
  rp.start(P->max_iterations, P->probability, n > 0 ? n : 1);
  pclhip_sac_plane_trace best_rec;
  std::memset(&best_rec, 0, sizeof best_rec);
  std::vector<hipEvent_t> ev_count;
  if (n >= 3) {  // (fewer points: getSamples finds no sample, ransac.hpp:120-124)
    pclhip_sac_plane_trace* rec = nullptr;
    float4* models = nullptr;
    uint32_t* counts = nullptr;
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&rec, size_t(cap) * sizeof(pclhip_sac_plane_trace)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&models, size_t(cap) * sizeof(float4)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&counts, size_t(cap) * 4));
    std::vector<pclhip_sac_plane_trace> hrec(static_cast<size_t>(cap));
    std::vector<uint32_t> hcnt(static_cast<size_t>(cap)), hval(static_cast<size_t>(cap), 1u);
    uint64_t t0 = 0;
    int B = P->batch_size > 0 ? P->batch_size : SAC_AUTO_BATCH;
    bool first = true;
    while (!rp.done) {
      // no batch holds more trials than the loop can still score: one pass covers a call that meets no skip
      const int64_t left = int64_t(P->max_iterations) + 1 - rp.iterations;
      const uint32_t nit = uint32_t(left < B ? (left > 0 ? left : 1) : B);
      hipEvent_t ea = nullptr, eb = nullptr;
      PCLHIP_CHECK_HIP(ctx, scope.event(&ea));
      PCLHIP_CHECK_HIP(ctx, scope.event(&eb));
      hipLaunchKernelGGL(sac_hypothesis_kernel, sac_blocks_of(nit), dim3(SAC_BLOCK), 0, s, P->seed, uint32_t(t0), nit, n, pc.pts,
                         rec, models);
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, size_t(nit) * 4, s));
      sac_score(ctx, M, pc, rec, models, nit, P->distance_threshold, counts, ea, eb);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
      ev_count.push_back(ea);
      ev_count.push_back(eb);
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hrec.data(), rec, size_t(nit) * sizeof(pclhip_sac_plane_trace), hipMemcpyDeviceToHost, s));
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hcnt.data(), counts, size_t(nit) * 4, hipMemcpyDeviceToHost, s));
      if (M.prepares()) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hval.data(), M.valid, size_t(nit) * 4, hipMemcpyDeviceToHost, s));
      SacDev hst;
      if (first) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hst, st, sizeof hst, hipMemcpyDeviceToHost, s));
      PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
      if (first) PCLHIP_REQUIRE(ctx, hst.bad_index == 0u, "an entry of indices lies outside the cloud");
      first = false;
      ++stats.batches;
      for (uint32_t t = 0; t < nit; ++t) {
        const bool valid = M.prepares() ? hval[t] != 0u : hrec[t].skipped == 0;
        hrec[t].count = valid ? hcnt[t] : 0u;
        const uint32_t before = rp.best;
        const bool more = rp.feed(hrec[t].skipped != 0, hrec[t].count);  // (an invalid trial: an iteration that counts 0)
        if (rp.best != before) best_rec = hrec[t];
        if (ctx->sac_trace.size() < SAC_TRACE_MAX) {
          ctx->sac_trace.push_back(hrec[t]);
          ctx->sac_trace_valid.push_back(valid ? 1 : 0);
        }
        if (!more) break;
      }
      t0 += nit;
      if (P->batch_size == 0 && B < SAC_MAX_BATCH) B *= 2;
      if (t0 + uint64_t(SAC_MAX_BATCH) >= 0xFFFFFFFFull) break;  // (the draw counter holds 32 bits)
    }
  } else if (n > 0) {
    SacDev hst;
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hst, st, sizeof hst, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    PCLHIP_REQUIRE(ctx, hst.bad_index == 0u, "an entry of indices lies outside the cloud");
  }
  stats.trials = rp.trials;
  stats.iterations = rp.iterations;
  stats.skipped = rp.skipped;
  stats.best_trial = int(rp.best_trial);
  stats.best_count = rp.best;

  // ---- the lists ----
  const bool found = rp.best_trial >= 0;
  uint64_t n_in = 0;
  SacDev hst;
  std::memset(&hst, 0, sizeof hst);
  int32_t *inl = nullptr, *outl = nullptr;
  if (found) {
    uint32_t *flag = nullptr, *excl = nullptr, *pos = nullptr;
    uint2* part = nullptr;
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&flag, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&excl, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((uint64_t(n) + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
    const bool inl_dev = out_inliers && is_device_pointer(out_inliers) && inliers_capacity >= n;
    const bool outl_dev = out_outliers && is_device_pointer(out_outliers) && outliers_capacity >= n;
    if (inl_dev) inl = out_inliers; else PCLHIP_CHECK_HIP(ctx, scope.alloc(&inl, size_t(n) * 4));
    if (out_outliers || out_n_outliers) {
      if (outl_dev) outl = out_outliers; else PCLHIP_CHECK_HIP(ctx, scope.alloc(&outl, size_t(n) * 4));
    }
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(st->coef, best_rec.coefficients, 16, hipMemcpyHostToDevice, s));
    auto select = [&]() {
      (void)hipMemsetAsync(st->tot, 0, 16, s);
      if (M.gated) hipLaunchKernelGGL(sac_gate_held_kernel, dim3(1), dim3(WAVE), 0, s, M.gate, st);
      if (M.normal)
        hipLaunchKernelGGL(sac_normal_flag_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, pc.pts, M.nn, M.wt, n, st,
                           P->distance_threshold, flag);
      else
        hipLaunchKernelGGL(sac_flag_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, pc.pts, n, st, thr, flag);
      launch_scan_u32(s, flag, n, part, st->tot, excl);
    };
    select();
    if (P->optimize_coefficients && rp.best > 3u) {
      // the first selection has rp.best inliers by construction: the same expression on the same points
      const uint32_t m = rp.best;
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&pos, size_t(m) * 4));
      uint32_t mblocks = (m + SAC_BLOCK - 1) / SAC_BLOCK;
      if (mblocks > uint32_t(SAC_MOMENT_BLOCKS)) mblocks = uint32_t(SAC_MOMENT_BLOCKS);
      double *partials = nullptr, *sums = nullptr;
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&partials, size_t(mblocks) * 9 * sizeof(double)));
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&sums, 9 * sizeof(double)));
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(pos, 0, size_t(m) * 4, s));
      hipLaunchKernelGGL(sac_positions_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, flag, excl, n, pos, m);
      hipLaunchKernelGGL(sac_moments_kernel, dim3(mblocks), dim3(SAC_BLOCK), 0, s, pc.pts, pos, m, partials);
      hipLaunchKernelGGL(block_sums_finalize_kernel<9>, dim3(9), dim3(WAVE), 0, s, partials, int(mblocks), sums);
      hipLaunchKernelGGL(sac_refit_kernel, dim3(1), dim3(WAVE), 0, s, sums, pc.pts, pos, m, st);
      select();
    }
    hipLaunchKernelGGL(sac_lists_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, flag, excl, n, pc.idx, inl, outl);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hst, st, sizeof hst, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    n_in = hst.tot[0];
    for (int i = 0; i < 4; ++i) out_coeff[i] = hst.coef[i];
    stats.refined = int(hst.refined);
  }
  const uint64_t n_out = uint64_t(n) - n_in;
  *out_n_inliers = n_in;
  if (out_n_outliers) *out_n_outliers = n_out;
  const bool short_in = out_inliers != nullptr && inliers_capacity < n_in;
  const bool short_out = out_outliers != nullptr && outliers_capacity < n_out;
  if (!short_in && !short_out) {
    if (found) {
      if ((rc = sac_copy_out(ctx, out_inliers, inl, n_in)) != PCLHIP_OK) return rc;
      if ((rc = sac_copy_out(ctx, out_outliers, outl, n_out)) != PCLHIP_OK) return rc;
    } else if (out_outliers != nullptr && n > 0) {  // no model: everything is left over
      uint32_t *flag = nullptr, *excl = nullptr;
      int32_t* all = nullptr;
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&flag, size_t(n) * 4));
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&excl, size_t(n) * 4));
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&all, size_t(n) * 4));
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(flag, 0, size_t(n) * 4, s));
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(excl, 0, size_t(n) * 4, s));
      hipLaunchKernelGGL(sac_lists_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, flag, excl, n, pc.idx,
                         static_cast<int32_t*>(nullptr), all);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
      if ((rc = sac_copy_out(ctx, out_outliers, all, n_out)) != PCLHIP_OK) return rc;
    }
  }
  (void)hipEventRecord(ev_call[1], s);
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  for (size_t p = 0; p + 1 < ev_count.size(); p += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev_count[p], ev_count[p + 1]) == hipSuccess) stats.count_ms += ms;
  }
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev_call[0], ev_call[1]) == hipSuccess) stats.total_ms = ms;
  if (out_stats) *out_stats = stats;
  if (short_in || short_out) {
    set_error(ctx, std::string(fn) + ": capacity too small (the counts hold the required sizes)");
    return PCLHIP_ERR_OVERFLOW;
  }
  return PCLHIP_OK;
}

}  // namespace
}  // namespace pclhip

extern "C" {

void pclhip_sac_model_params_default(pclhip_sac_model_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->model_type = PCLHIP_SACMODEL_PLANE;
  p->normal_distance_weight = 0.1;
}

pclhip_status pclhip_sac_segment_model(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const void* normals,
                                       size_t nstride, const int32_t* indices, uint64_t n_indices,
                                       const pclhip_sac_plane_params* P, const pclhip_sac_model_params* MP, float out_coeff[4],
                                       int32_t* out_inliers, uint64_t inliers_capacity, uint64_t* out_n_inliers,
                                       int32_t* out_outliers, uint64_t outliers_capacity, uint64_t* out_n_outliers,
                                       pclhip_sac_plane_stats* out_stats) {
  if (!MP) return PCLHIP_ERR_INVALID;
  return pclhip::sac_segment_run(ctx, "pclhip_sac_segment_model", cloud, n_rec, stride, normals, nstride, indices, n_indices, P, MP,
                                 out_coeff, out_inliers, inliers_capacity, out_n_inliers, out_outliers, outliers_capacity,
                                 out_n_outliers, out_stats);
}

pclhip_status pclhip_sac_model_evaluate(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const void* normals,
                                        size_t nstride, const int32_t* indices, uint64_t n_indices, double threshold,
                                        const pclhip_sac_model_params* MP, const float* coeffs, int n_models,
                                        uint32_t* out_counts, uint8_t* out_valid) {
  using namespace pclhip;
  if (!ctx || !MP || n_models < 0 || (n_models > 0 && (!coeffs || !out_counts))) return PCLHIP_ERR_INVALID;
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
  SacModel M;
  if ((rc = sac_model_setup(ctx, scope, MP, normals, nstride, n_rec, pc, SAC_MAX_BATCH, &M)) != PCLHIP_OK) return rc;
  for (int m = 0; m < n_models; ++m) out_counts[m] = 0u;
  if (out_valid) for (int m = 0; m < n_models; ++m) out_valid[m] = 1;
  if (n_models == 0) return PCLHIP_OK;
  if (pc.n > 0) {
    SacDev h;
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    PCLHIP_REQUIRE(ctx, h.bad_index == 0u, "an entry of indices lies outside the cloud");
  }
  float4* models = nullptr;
  uint32_t* counts = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&models, size_t(SAC_MAX_BATCH) * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&counts, size_t(SAC_MAX_BATCH) * 4));
  std::vector<uint32_t> hval(static_cast<size_t>(SAC_MAX_BATCH));
  for (int m0 = 0; m0 < n_models; m0 += SAC_MAX_BATCH) {
    const uint32_t H = uint32_t(n_models - m0 < SAC_MAX_BATCH ? n_models - m0 : SAC_MAX_BATCH);
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(models, coeffs + size_t(m0) * 4, size_t(H) * sizeof(float4), hipMemcpyHostToDevice, s));
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, size_t(H) * 4, s));
    if (pc.n > 0) {
      sac_score(ctx, M, pc, nullptr, models, H, threshold, counts, nullptr, nullptr);
    } else if (M.prepares()) {  // (no point: the gate's bits alone)
      hipLaunchKernelGGL(sac_prepare_kernel, sac_blocks_of(H), dim3(SAC_BLOCK), 0, s, M.gate, H,
                         static_cast<const pclhip_sac_plane_trace*>(nullptr), models, M.unit, M.valid);
    }
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_counts + m0, counts, size_t(H) * 4, hipMemcpyDeviceToHost, s));
    if (out_valid && M.prepares()) PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hval.data(), M.valid, size_t(H) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    if (out_valid && M.prepares()) for (uint32_t h = 0; h < H; ++h) out_valid[m0 + h] = hval[h] != 0u ? 1 : 0;
  }
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_last_model_trace(pclhip_ctx* ctx, pclhip_sac_model_trace* buf, uint64_t capacity, uint64_t* count) {
  if (!ctx || !count || (capacity > 0 && !buf)) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *count = ctx->sac_trace.size();
  const uint64_t m = capacity < *count ? capacity : *count;
  for (uint64_t t = 0; t < m; ++t) {
    const pclhip_sac_plane_trace& r = ctx->sac_trace[t];
    pclhip_sac_model_trace& o = buf[t];
    for (int i = 0; i < 3; ++i) o.samples[i] = r.samples[i];
    o.skipped = r.skipped;
    for (int i = 0; i < 4; ++i) o.coefficients[i] = r.coefficients[i];
    o.count = r.count;
    o.valid = int(ctx->sac_trace_valid[t]);
  }
  return PCLHIP_OK;
}

#ifdef PCLHIP_SAC_SCREEN_STATS
// pairs that took the double acos since the last call of this function (scripts/sac_models_timing.py's own build)
PCLHIP_API unsigned long long pclhip_sac_exact_pairs_take(void) {
  unsigned long long v = 0, zero = 0;
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(pclhip::sac_exact_pairs), sizeof v);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(pclhip::sac_exact_pairs), &zero, sizeof zero);
  return v;
}
#endif

}  // extern "C"
