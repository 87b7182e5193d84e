// sac_cylinder.hpp -- SampleConsensusModelCylinder under RandomSampleConsensus (sample_consensus/.../impl/
// sac_model_cylinder.hpp:49-140,182-265,268-309,453-489, sample_consensus/src/sac_model_cylinder.cpp:42-143, impl/ransac.hpp:
// 56-217, common/.../distances.h:75-80, common/impl/common.hpp:58-68) and the one call that does what SACSegmentation::segment
// does with them (segmentation/.../impl/sac_segmentation.hpp:79-133); the semantics are stated in include/pclhip.h.  Included
// by radius.hip after sac_models.hpp, whose gather, scan, position and list kernels and float helpers it uses.
//
// Per call: sac_gather_kernel, sac_normals_gather_kernel (the unit normals of the point set).  Per batch of trials:
//   sac_cylinder_hypothesis_kernel  one thread per trial: the two draws, the cylinder of two oriented points in the reference's
//                                   Vector4f order, the skip flag, the trace record
//   sac_cylinder_prepare_kernel     one thread per hypothesis: the gate's bit, and what the scoring pass reads: (line_pt,
//                                   radius) and the re-normalised line_dir as two float4 (radius NaN: not scored)
//   sac_cylinder_count_kernel       points x hypotheses, the shape of sac_normal_count_kernel.  Tier 1: the Euclidean exit as
//                                   ONE float compare, e >= e_out, where e_out is the least float whose
//                                   (1 - ndw) * double(e) exceeds the threshold (found by bisection over the float's bits,
//                                   sac_cylinder_e_out: the product is monotone in e, so the set is an upper interval and
//                                   the compare is exact).  Tier 2: the pairs left (inside the shell) run as bits of a lane
//                                   mask through one copy of sac_cylinder_inlier.
// After the replay: sac_cylinder_gate_held_kernel, sac_cylinder_flag_kernel, scan, lists; the refit between two selections:
//   sac_cylinder_centroid_kernel + sac_cylinder_frame_kernel   the reference's frame (ref_pt, ref_dir, u, v), in double
//   sac_cylinder_lm_pass_kernel     over the inlier positions: sum f^2, J^T f (5), J^T J (15) per block (block_sums.hpp's order)
//   sac_cylinder_lm_step_kernel     one thread: Levenberg-Marquardt's state (damped 5x5 Cholesky, gain ratio, accept / reject,
//                                   the stop flag); pass + step pairs are enqueued in chunks, the host reads the stop flag once
//                                   per chunk and the kernels behind a stop do nothing
//   sac_cylinder_lm_finish_kernel   the coefficients from the accepted unknowns, or the unrefined ones
#pragma once

#include <limits>

#include "sac_models.hpp"

namespace pclhip {
namespace {

constexpr int SACC_P = 8;                        // points a lane keeps (6 registers each: point, unit normal)
constexpr int SACC_TILE = SAC_BLOCK * SACC_P;
constexpr int SACC_LM_CAP = 100;                 // Levenberg-Marquardt steps at most
constexpr int SACC_LM_CHUNK = 10;                // pass + step pairs between two reads of the stop flag
constexpr int SACC_NS = 21;                      // sums of a pass: f^2, J^T f, the upper triangle of J^T J

struct SacCylGate {
  int angle_on;        // eps_angle > 0
  float ax, ay, az;
  double eps_angle;
  double rmin, rmax;   // -DBL_MAX / DBL_MAX: not set
};

struct SacCylDev {     // device-resident results of a call
  float coef[7];       // the winner's coefficients, then the refined ones
  uint32_t refined;
  uint32_t invalid;    // the coefficients fail the gate: the selection is empty
  uint32_t lm_iterations;
  uint32_t pad[2];
};

struct SacCylLM {      // the refit's state
  double ref_pt[3], ref_dir[3], u[3], v[3];
  double x[5], xe[5];            // the accepted unknowns; the ones the next pass evaluates
  double cost, g[5], H[15];      // sum f^2, J^T f, J^T J at x
  double delta[5];               // xe - x
  double lambda, nu;
  uint32_t stop, iters, accepted, failed, first, pad;
};

// the order of a float sum of three products of Eigen::Vector3f (include/pclhip.h): x x' + (y y' + z z')
__host__ __device__ inline float sac_dot3v(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fmul_rn(ax, bx), __fadd_rn(__fmul_rn(ay, by), __fmul_rn(az, bz)));
}

// Eigen's normalized() of a Vector3f
__device__ inline void sac_normalized3v(float& x, float& y, float& z) {
  const float q = sac_dot3v(x, y, z, x, y, z);
  if (q > 0.0f) {
    const float r = sqrtf(q);
    x = __fdiv_rn(x, r); y = __fdiv_rn(y, r); z = __fdiv_rn(z, r);
  }
}

// isModelValid (impl/sac_model_cylinder.hpp:453-489) of (.., dx, dy, dz, radius)
__device__ inline bool sac_cylinder_gate_valid(const SacCylGate& g, float dx, float dy, float dz, float radius) {
  if (g.angle_on) {
    float ax = g.ax, ay = g.ay, az = g.az;
    sac_normalized3v(ax, ay, az);
    sac_normalized3v(dx, dy, dz);
    if (sac_folded_angle(sac_dot3v(ax, ay, az, dx, dy, dz)) > g.eps_angle) return false;  // :460-473
  }
  if (g.rmin != -DBL_MAX && double(radius) < g.rmin) return false;  // :475
  if (g.rmax != DBL_MAX && double(radius) > g.rmax) return false;   // :481
  return true;
}

// |dist(point, axis) - radius| in float (impl/sac_model_cylinder.hpp:206-210); A = (line_pt, radius), B = the unit line_dir.
// (dirx, diry, dirz): the vector from the axis to the point
__device__ inline float sac_cylinder_e(float px, float py, float pz, const float4& A, const float4& B, float& dirx, float& diry,
                                       float& dirz) {
  const float fx = __fsub_rn(px, A.x), fy = __fsub_rn(py, A.y), fz = __fsub_rn(pz, A.z);  // diff = pt - line_pt
  const float t = sac_dot3v(fx, fy, fz, B.x, B.y, B.z);
  dirx = __fsub_rn(fx, __fmul_rn(t, B.x));  // dir = diff - (diff . line_dir) line_dir
  diry = __fsub_rn(fy, __fmul_rn(t, B.y));
  dirz = __fsub_rn(fz, __fmul_rn(t, B.z));
  return __builtin_fabsf(__fsub_rn(sqrtf(sac_dot3v(dirx, diry, dirz, dirx, diry, dirz)), A.w));
}

// the float dot of the point's unit normal with normalized(dir) (:215-216)
__device__ inline float sac_cylinder_rad(float nx, float ny, float nz, float dirx, float diry, float dirz) {
  sac_normalized3v(dirx, diry, dirz);
  return sac_dot3v(nx, ny, nz, dirx, diry, dirz);
}

// the ONE distance test of counting and both selections (:206-221); (nx, ny, nz): the point's unit normal; om = 1.0 - ndw
__device__ inline bool sac_cylinder_inlier(float px, float py, float pz, float nx, float ny, float nz, const float4& A,
                                           const float4& B, double ndw, double om, double thr) {
  float dx, dy, dz;
  const float e = sac_cylinder_e(px, py, pz, A, B, dx, dy, dz);
  const double wed = om * double(e);
  if (wed > thr) return false;  // :211
  const double d_normal = sac_folded_angle(sac_cylinder_rad(nx, ny, nz, dx, dy, dz));
  return fabs(ndw * d_normal + wed) < thr;
}

// computeModelCoefficients (:75-140) of the points at positions s0, s1 with their RAW normal records -> c[7]; true: skip
__device__ inline bool sac_cylinder_from_samples(const float4* __restrict__ pts, const char* __restrict__ nrec, size_t nstride,
                                                 uint64_t n_rec, const int32_t* __restrict__ idx, int s0, int s1, double rmin,
                                                 double rmax, float c[7]) {
  const float4 p1 = pts[s0], p2 = pts[s1];
  float n1[3], n2[3];
  const int64_t r1 = idx ? int64_t(idx[s0]) : int64_t(s0), r2 = idx ? int64_t(idx[s1]) : int64_t(s1);
  for (int i = 0; i < 3; ++i) {
    n1[i] = r1 >= 0 && uint64_t(r1) < n_rec ? reinterpret_cast<const float*>(nrec + size_t(r1) * nstride)[i] : __builtin_nanf("");
    n2[i] = r2 >= 0 && uint64_t(r2) < n_rec ? reinterpret_cast<const float*>(nrec + size_t(r2) * nstride)[i] : __builtin_nanf("");
  }
  // isSampleGood (:59-68)
  bool skip = __builtin_fabsf(__fsub_rn(p1.x, p2.x)) <= FLT_EPSILON && __builtin_fabsf(__fsub_rn(p1.y, p2.y)) <= FLT_EPSILON &&
              __builtin_fabsf(__fsub_rn(p1.z, p2.z)) <= FLT_EPSILON;
  // w = n1 + p1 - p2, line_dir = n1 x n2 (:96-97)
  const float wx = __fsub_rn(__fadd_rn(n1[0], p1.x), p2.x), wy = __fsub_rn(__fadd_rn(n1[1], p1.y), p2.y),
              wz = __fsub_rn(__fadd_rn(n1[2], p1.z), p2.z);
  float lx = __fsub_rn(__fmul_rn(n1[1], n2[2]), __fmul_rn(n1[2], n2[1]));
  float ly = __fsub_rn(__fmul_rn(n1[2], n2[0]), __fmul_rn(n1[0], n2[2]));
  float lz = __fsub_rn(__fmul_rn(n1[0], n2[1]), __fmul_rn(n1[1], n2[0]));
  const float b = sac_dot3(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]);  // :99-103
  const float cc = sac_dot3(n2[0], n2[1], n2[2], n2[0], n2[1], n2[2]);
  const float d = sac_dot3(n1[0], n1[1], n1[2], wx, wy, wz);
  const float e = sac_dot3(n2[0], n2[1], n2[2], wx, wy, wz);
  const float den = sac_dot3(lx, ly, lz, lx, ly, lz);
  const float sc = double(den) < 1e-8 ? 0.0f : __fdiv_rn(__fsub_rn(__fmul_rn(b, e), __fmul_rn(cc, d)), den);  // :106-113
  const float qx = __fadd_rn(__fadd_rn(p1.x, n1[0]), __fmul_rn(sc, n1[0]));  // line_pt = p1 + n1 + sc n1 (:116)
  const float qy = __fadd_rn(__fadd_rn(p1.y, n1[1]), __fmul_rn(sc, n1[1]));
  const float qz = __fadd_rn(__fadd_rn(p1.z, n1[2]), __fmul_rn(sc, n1[2]));
  sac_normalized(lx, ly, lz);  // :117
  // sqrPointToLineDistance (distances.h:75-80): |line_dir x (line_pt - p)|^2 / |line_dir|^2, a float quotient
  const float l2 = sac_dot3(lx, ly, lz, lx, ly, lz);
  double root[2];
  for (int k = 0; k < 2; ++k) {
    const float4 p = k == 0 ? p1 : p2;
    const float ux = __fsub_rn(qx, p.x), uy = __fsub_rn(qy, p.y), uz = __fsub_rn(qz, p.z);
    const float cx = __fsub_rn(__fmul_rn(ly, uz), __fmul_rn(lz, uy));
    const float cy = __fsub_rn(__fmul_rn(lz, ux), __fmul_rn(lx, uz));
    const float cz = __fsub_rn(__fmul_rn(lx, uy), __fmul_rn(ly, ux));
    root[k] = sqrt(double(__fdiv_rn(sac_dot3(cx, cy, cz, cx, cy, cz), l2)));
  }
  const float radius = float(0.5 * (root[0] + root[1]));  // :129-131
  if (double(radius) > rmax || double(radius) < rmin) skip = true;  // :133
  c[0] = qx; c[1] = qy; c[2] = qz; c[3] = lx; c[4] = ly; c[5] = lz; c[6] = radius;
  return skip;
}

__global__ __launch_bounds__(SAC_BLOCK) void sac_cylinder_hypothesis_kernel(uint64_t seed, uint32_t it0, uint32_t nit, uint32_t n,
                                                                            const float4* __restrict__ pts,
                                                                            const char* __restrict__ nrec, size_t nstride,
                                                                            uint64_t n_rec, const int32_t* __restrict__ idx,
                                                                            double rmin, double rmax,
                                                                            pclhip_sac_cylinder_trace* __restrict__ rec) {
  const uint32_t t = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (t >= nit) return;
  int s[scp::MAX_SAMPLES];
  scp::select_samples(seed, it0 + t, 2, int(n), s);
  float c[7];
  const bool skip = sac_cylinder_from_samples(pts, nrec, nstride, n_rec, idx, s[0], s[1], rmin, rmax, c);
  pclhip_sac_cylinder_trace& r = rec[t];
  r.samples[0] = s[0]; r.samples[1] = s[1];
  r.skipped = skip ? 1 : 0;
  for (int i = 0; i < 7; ++i) r.coefficients[i] = c[i];
  r.count = 0u;
  r.valid = 0;
}

// computeModelCoefficients of a given sample: the point set is the sample, positions 0 and 1.  One thread.
__global__ void sac_cylinder_model_kernel(const float4* __restrict__ pts, const char* __restrict__ nrec, size_t nstride,
                                          uint64_t n_rec, const int32_t* __restrict__ idx, double rmin, double rmax,
                                          pclhip_sac_cylinder_trace* __restrict__ rec) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float c[7];
  const bool skip = sac_cylinder_from_samples(pts, nrec, nstride, n_rec, idx, 0, 1, rmin, rmax, c);
  rec->samples[0] = 0; rec->samples[1] = 1;
  rec->skipped = skip ? 1 : 0;
  for (int i = 0; i < 7; ++i) rec->coefficients[i] = c[i];
  rec->count = 0u;
  rec->valid = 0;
}

// rec: the batch's trace records; null: coeffs holds H septuples.  valid[t], A[t] = (line_pt, radius; NaN when not scored),
// B[t] = the unit line_dir (:198-200)
__global__ __launch_bounds__(SAC_BLOCK) void sac_cylinder_prepare_kernel(SacCylGate g, uint32_t H,
                                                                         const pclhip_sac_cylinder_trace* __restrict__ rec,
                                                                         const float* __restrict__ coeffs, float4* __restrict__ A,
                                                                         float4* __restrict__ B, uint32_t* __restrict__ valid) {
  const uint32_t t = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (t >= H) return;
  const float* c = rec != nullptr ? rec[t].coefficients : coeffs + size_t(t) * 7;
  float dx = c[3], dy = c[4], dz = c[5];
  const bool ok = !(rec != nullptr && rec[t].skipped != 0) && sac_cylinder_gate_valid(g, dx, dy, dz, c[6]);
  sac_normalized3v(dx, dy, dz);
  A[t] = make_float4(c[0], c[1], c[2], ok ? c[6] : __builtin_nanf(""));
  B[t] = make_float4(dx, dy, dz, 0.0f);
  valid[t] = ok ? 1u : 0u;
}

// the gate on the coefficients the device holds (before a selection): cy->invalid
__global__ void sac_cylinder_gate_held_kernel(SacCylGate g, SacCylDev* __restrict__ cy) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  cy->invalid = sac_cylinder_gate_valid(g, cy->coef[3], cy->coef[4], cy->coef[5], cy->coef[6]) ? 0u : 1u;
}

#ifdef PCLHIP_SACC_STATS
__device__ unsigned long long sacc_exact_pairs;  // pairs that reached tier 2 (scripts/sac_cylinder_timing.py's build)
#endif

// countWithinDistance of H cylinders at once.  counts[] is zero before the launch.  e_out: NaN for no tier 1.
__global__ __launch_bounds__(SAC_BLOCK) void sac_cylinder_count_kernel(const float4* __restrict__ pts,
                                                                       const float4* __restrict__ nn, uint32_t n,
                                                                       const float4* __restrict__ A, const float4* __restrict__ B,
                                                                       uint32_t H, double ndw, double om, double thr, float e_out,
                                                                       uint32_t* __restrict__ counts) {
  __shared__ uint32_t cnt_s[SAC_MAX_BATCH];
  for (uint32_t h = threadIdx.x; h < H; h += SAC_BLOCK) cnt_s[h] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint32_t tiles = (n + SACC_TILE - 1) / SACC_TILE;
  const float nanf_ = __builtin_nanf("");
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // slot k of lane l is point base + k * 64 + l (coalesced); past the end: NaN, never inside
    const uint32_t base = tile * uint32_t(SACC_TILE) + wave * uint32_t(SACC_P * WAVE) + lane;
    float px[SACC_P], py[SACC_P], pz[SACC_P], nx[SACC_P], ny[SACC_P], nz[SACC_P];
#pragma unroll
    for (int k = 0; k < SACC_P; ++k) {
      const uint32_t i = base + uint32_t(k) * WAVE;
      float4 q = make_float4(nanf_, nanf_, nanf_, 0.0f), u = q;
      if (i < n) { q = pts[i]; u = nn[i]; }
      px[k] = q.x; py[k] = q.y; pz[k] = q.z;
      nx[k] = u.x; ny[k] = u.y; nz[k] = u.z;
    }
    for (uint32_t h0 = 0; h0 < H; h0 += WAVE) {
      const uint32_t hn = H - h0 < uint32_t(WAVE) ? H - h0 : uint32_t(WAVE);
      uint32_t mine = 0u;  // lane j: the wave's count of hypothesis h0 + j
      for (uint32_t j = 0; j < hn; ++j) {
        const float4 a = A[h0 + j];  // (the same for the wave: scalar loads)
        if (!(__builtin_fabsf(a.w) <= FLT_MAX)) continue;  // skipped, invalid, or a radius that is not finite: counts 0
        const float4 b = B[h0 + j];
        uint32_t inbits = 0u, askbits = 0u;  // bit k: slot k is inside; slot k takes the exact function
#ifdef PCLHIP_SACC_NO_SCREEN
        askbits = (1u << SACC_P) - 1u;
#else
#pragma unroll
        for (int k = 0; k < SACC_P; ++k) {
          float dx, dy, dz;
          const float e = sac_cylinder_e(px[k], py[k], pz[k], a, b, dx, dy, dz);
          askbits |= e >= e_out ? 0u : 1u << k;  // (a NaN e asks: the exact function rejects it)
        }
#endif
        while (__builtin_amdgcn_ballot_w64(askbits != 0u) != 0ull) {  // one slot of a lane per turn
          if (askbits != 0u) {
            const int sel = __builtin_ctz(askbits);
            askbits &= askbits - 1u;
            float sx = 0.0f, sy = 0.0f, sz = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f;
#pragma unroll
            for (int k = 0; k < SACC_P; ++k) {
              if (k == sel) { sx = px[k]; sy = py[k]; sz = pz[k]; tx = nx[k]; ty = ny[k]; tz = nz[k]; }
            }
            inbits |= sac_cylinder_inlier(sx, sy, sz, tx, ty, tz, a, b, ndw, om, thr) ? 1u << sel : 0u;
#ifdef PCLHIP_SACC_STATS
            atomicAdd(&sacc_exact_pairs, 1ull);
#endif
          }
        }
        uint32_t cw = 0u;
#pragma unroll
        for (int k = 0; k < SACC_P; ++k) cw += uint32_t(__popcll(__builtin_amdgcn_ballot_w64(((inbits >> k) & 1u) != 0u)));
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

// the held coefficients as the scoring pass reads them
__device__ inline void sac_cylinder_held(const SacCylDev* __restrict__ cy, float4& A, float4& B) {
  float dx = cy->coef[3], dy = cy->coef[4], dz = cy->coef[5];
  sac_normalized3v(dx, dy, dz);
  A = make_float4(cy->coef[0], cy->coef[1], cy->coef[2], cy->coef[6]);
  B = make_float4(dx, dy, dz, 0.0f);
}

// selectWithinDistance (:182-227) as flags by position, with the coefficients the device holds
__global__ __launch_bounds__(SAC_BLOCK) void sac_cylinder_flag_kernel(const float4* __restrict__ pts,
                                                                      const float4* __restrict__ nn, uint32_t n,
                                                                      const SacCylDev* __restrict__ cy, double ndw, double om,
                                                                      double thr, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  float4 A, B;
  sac_cylinder_held(cy, A, B);
  const float4 p = pts[i], u = nn[i];
  flag[i] = cy->invalid == 0u && sac_cylinder_inlier(p.x, p.y, p.z, u.x, u.y, u.z, A, B, ndw, om, thr) ? 1u : 0u;
}

// getDistancesToModel (:143-179): no early exit
__global__ __launch_bounds__(SAC_BLOCK) void sac_cylinder_distance_kernel(const float4* __restrict__ pts,
                                                                          const float4* __restrict__ nn, uint32_t n,
                                                                          const SacCylDev* __restrict__ cy, double ndw, double om,
                                                                          double* __restrict__ out) {
  const uint32_t i = blockIdx.x * SAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  float4 A, B;
  sac_cylinder_held(cy, A, B);
  const float4 p = pts[i], u = nn[i];
  float dx, dy, dz;
  const float e = sac_cylinder_e(p.x, p.y, p.z, A, B, dx, dy, dz);
  const double wed = om * double(e);
  out[i] = fabs(ndw * sac_folded_angle(sac_cylinder_rad(u.x, u.y, u.z, dx, dy, dz)) + wed);
}

// ---- the refit (sample_consensus/src/sac_model_cylinder.cpp:42-143), in double ----

// the inliers' coordinate sums; pos_list null: positions 0 .. m-1
__global__ __launch_bounds__(SAC_BLOCK) void sac_cylinder_centroid_kernel(const float4* __restrict__ pts,
                                                                          const uint32_t* __restrict__ pos_list, uint32_t m,
                                                                          double* __restrict__ partials) {
  double acc[3] = {0.0, 0.0, 0.0};
  const uint32_t threads = gridDim.x * SAC_BLOCK;
  for (uint32_t e = blockIdx.x * SAC_BLOCK + threadIdx.x; e < m; e += threads) {
    const float4 p = pts[pos_list ? pos_list[e] : e];
    acc[0] += double(p.x); acc[1] += double(p.y); acc[2] += double(p.z);
  }
  block_rows<3, SAC_WAVES, 3>(acc, partials);
}

// the frame (:107-124) and the start (:128-129): one thread
__global__ void sac_cylinder_frame_kernel(const double* __restrict__ sums, uint32_t m, const SacCylDev* __restrict__ cy,
                                          SacCylLM* __restrict__ lm) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double lp[3], ld[3], u[3];
  for (int i = 0; i < 3; ++i) { lp[i] = double(cy->coef[i]); ld[i] = double(cy->coef[3 + i]); }
  const double q = ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2];
  if (q > 0.0) { const double r = sqrt(q); ld[0] /= r; ld[1] /= r; ld[2] /= r; }
  double t = 0.0;
  for (int i = 0; i < 3; ++i) t += (sums[i] / double(m) - lp[i]) * ld[i];
  for (int i = 0; i < 3; ++i) lp[i] += t * ld[i];  // :113-114
  const double ax = fabs(ld[0]), ay = fabs(ld[1]), az = fabs(ld[2]);
  const int pick = ax < ay ? (ax < az ? 0 : 2) : 1;  // :117-121
  for (int i = 0; i < 3; ++i) u[i] = i == pick ? 1.0 : 0.0;
  const double du = ld[pick];
  for (int i = 0; i < 3; ++i) u[i] -= du * ld[i];
  const double uq = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
  if (uq > 0.0) { const double r = sqrt(uq); u[0] /= r; u[1] /= r; u[2] /= r; }
  for (int i = 0; i < 3; ++i) { lm->ref_pt[i] = lp[i]; lm->ref_dir[i] = ld[i]; lm->u[i] = u[i]; }
  lm->v[0] = ld[1] * u[2] - ld[2] * u[1];
  lm->v[1] = ld[2] * u[0] - ld[0] * u[2];
  lm->v[2] = ld[0] * u[1] - ld[1] * u[0];
  for (int i = 0; i < 5; ++i) { lm->x[i] = 0.0; lm->xe[i] = 0.0; lm->delta[i] = 0.0; lm->g[i] = 0.0; }
  lm->x[4] = lm->xe[4] = double(cy->coef[6]);
  for (int i = 0; i < 15; ++i) lm->H[i] = 0.0;
  lm->cost = 0.0;
  lm->lambda = 1e-3;
  lm->nu = 2.0;
  lm->stop = 0u; lm->iters = 0u; lm->accepted = 0u; lm->failed = 0u; lm->first = 1u; lm->pad = 0u;
}

// the residual f = |(line_pt - p) x normalized(line_dir)| - |r| (:63-73) and its Jacobian (:80-99) at lm->xe, summed
__global__ __launch_bounds__(SAC_BLOCK) void sac_cylinder_lm_pass_kernel(const float4* __restrict__ pts,
                                                                         const uint32_t* __restrict__ pos_list, uint32_t m,
                                                                         const SacCylLM* __restrict__ lm,
                                                                         double* __restrict__ partials) {
  if (lm->stop != 0u) return;  // (the same for every thread)
  double acc[SACC_NS];
#pragma unroll
  for (int i = 0; i < SACC_NS; ++i) acc[i] = 0.0;
  double lp[3], ld[3], u[3], v[3];
  for (int i = 0; i < 3; ++i) {
    u[i] = lm->u[i]; v[i] = lm->v[i];
    lp[i] = lm->ref_pt[i] + lm->xe[0] * u[i] + lm->xe[1] * v[i];
    ld[i] = lm->ref_dir[i] + lm->xe[2] * u[i] + lm->xe[3] * v[i];
  }
  const double sqr = ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2];
  const double ar = fabs(lm->xe[4]), jr = lm->xe[4] > 0.0 ? -1.0 : 1.0;
  const uint32_t threads = gridDim.x * SAC_BLOCK;
  for (uint32_t e = blockIdx.x * SAC_BLOCK + threadIdx.x; e < m; e += threads) {
    const float4 p = pts[pos_list ? pos_list[e] : e];
    const double bx = lp[0] - double(p.x), by = lp[1] - double(p.y), bz = lp[2] - double(p.z);
    const double cx = ld[1] * bz - ld[2] * by, cy = ld[2] * bx - ld[0] * bz, cz = ld[0] * by - ld[1] * bx;
    const double dist = sqrt((cx * cx + cy * cy + cz * cz) / sqr);
    const double dir_b = ld[0] * bx + ld[1] * by + ld[2] * bz;
    const double dx = bx - dir_b * ld[0] / sqr, dy = by - dir_b * ld[1] / sqr, dz = bz - dir_b * ld[2] / sqr;
    const double du = (dx * u[0] + dy * u[1] + dz * u[2]) / dist, dv = (dx * v[0] + dy * v[1] + dz * v[2]) / dist;
    const double J[5] = {du, dv, -du * dir_b / sqr, -dv * dir_b / sqr, jr};
    const double f = dist - ar;
    acc[0] += f * f;
    int k = 6;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      acc[1 + a] += J[a] * f;
#pragma unroll
      for (int b = a; b < 5; ++b) acc[k++] += J[a] * J[b];
    }
  }
  block_rows<SACC_NS, SAC_WAVES, SACC_NS>(acc, partials);
}

// 5x5: (H + lambda diag(H)) d = -g by Cholesky; false when a pivot is not positive
__device__ inline bool sac_cylinder_solve(const double* H, const double* g, double lambda, double d[5]) {
  double L[5][5];
  int k = 0;
  for (int a = 0; a < 5; ++a)
    for (int b = a; b < 5; ++b) { L[a][b] = L[b][a] = H[k]; ++k; }
  for (int a = 0; a < 5; ++a) L[a][a] += lambda * (L[a][a] > 1e-300 ? L[a][a] : 1e-300);
  for (int j = 0; j < 5; ++j) {
    double s = L[j][j];
    for (int c = 0; c < j; ++c) s -= L[j][c] * L[j][c];
    if (!(s > 0.0) || !(s <= DBL_MAX)) return false;
    const double r = sqrt(s);
    L[j][j] = r;
    for (int i = j + 1; i < 5; ++i) {
      double t = L[i][j];
      for (int c = 0; c < j; ++c) t -= L[i][c] * L[j][c];
      L[i][j] = t / r;
    }
  }
  double y[5];
  for (int i = 0; i < 5; ++i) {
    double t = -g[i];
    for (int c = 0; c < i; ++c) t -= L[i][c] * y[c];
    y[i] = t / L[i][i];
  }
  for (int i = 4; i >= 0; --i) {
    double t = y[i];
    for (int c = i + 1; c < 5; ++c) t -= L[c][i] * d[c];
    d[i] = t / L[i][i];
  }
  return true;
}

// Levenberg-Marquardt on the sums of the pass at lm->xe: one thread
__global__ void sac_cylinder_lm_step_kernel(const double* __restrict__ sums, SacCylLM* __restrict__ lm) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || lm->stop != 0u) return;
  bool finite = true;
  for (int i = 0; i < SACC_NS; ++i) finite = finite && fabs(sums[i]) <= DBL_MAX;
  if (!finite && lm->first != 0u) { lm->failed = 1u; lm->stop = 1u; return; }
  bool take = false;
  if (lm->first != 0u) {
    take = true;
    lm->first = 0u;
  } else {
    ++lm->iters;
    // what the damped model promised for this step against what the pass found (both for 0.5 sum f^2)
    double pred = 0.0;
    int k = 0;
    for (int a = 0; a < 5; ++a) {
      const double D = lm->H[k] > 1e-300 ? lm->H[k] : 1e-300;
      pred += 0.5 * lm->delta[a] * (lm->lambda * D * lm->delta[a] - lm->g[a]);
      k += 5 - a;
    }
    const double act = 0.5 * (lm->cost - sums[0]);
    if (finite && act > 0.0 && pred > 0.0) {
      const double rho = act / pred, c = 2.0 * rho - 1.0, f = 1.0 - c * c * c;
      take = true;
      ++lm->accepted;
      lm->lambda *= f > 1.0 / 3.0 ? f : 1.0 / 3.0;
      lm->nu = 2.0;
    } else {
      lm->lambda *= lm->nu;
      lm->nu *= 2.0;
    }
  }
  if (take) {
    for (int i = 0; i < 5; ++i) { lm->x[i] = lm->xe[i]; lm->g[i] = sums[1 + i]; }
    for (int i = 0; i < 15; ++i) lm->H[i] = sums[6 + i];
    lm->cost = sums[0];
  }
  // stop: no residual; a gradient orthogonal to the residual to 1e-12 (|g_a| <= 1e-12 sqrt(H_aa sum f^2)); the cap
  bool flat = true;
  int k = 0;
  for (int a = 0; a < 5; ++a) {
    if (!(fabs(lm->g[a]) <= 1e-12 * sqrt(lm->H[k] * lm->cost))) flat = false;
    k += 5 - a;
  }
  if (lm->cost == 0.0 || flat || lm->iters >= uint32_t(SACC_LM_CAP) || lm->lambda > 1e16) { lm->stop = 1u; return; }
  double d[5];
  while (!sac_cylinder_solve(lm->H, lm->g, lm->lambda, d)) {
    lm->lambda *= lm->nu;
    lm->nu *= 2.0;
    if (!(lm->lambda <= 1e16)) { lm->failed = 1u; lm->stop = 1u; return; }  // the largest damping
  }
  // stop: a step below 1e-12 of the unknowns' scales (the radius for a, b and r; 1 for the direction's c, d)
  const double rs = fabs(lm->x[4]);
  if (fabs(d[0]) <= 1e-12 * rs && fabs(d[1]) <= 1e-12 * rs && fabs(d[4]) <= 1e-12 * rs && fabs(d[2]) <= 1e-12 &&
      fabs(d[3]) <= 1e-12) {
    lm->stop = 1u;
    return;
  }
  for (int i = 0; i < 5; ++i) {
    lm->delta[i] = d[i];
    lm->xe[i] = lm->x[i] + d[i];
    if (!(fabs(lm->xe[i]) <= DBL_MAX)) { lm->failed = 1u; lm->stop = 1u; }
  }
}

// :131-139 and impl/sac_model_cylinder.hpp:304-308; without an accepted step the coefficients stay
__global__ void sac_cylinder_lm_finish_kernel(const SacCylLM* __restrict__ lm, SacCylDev* __restrict__ cy) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  cy->lm_iterations = lm->iters;
  if (lm->failed != 0u || lm->accepted == 0u) return;
  float c[7];
  for (int i = 0; i < 3; ++i) {
    c[i] = float(lm->ref_pt[i] + lm->x[0] * lm->u[i] + lm->x[1] * lm->v[i]);
    c[3 + i] = float(lm->ref_dir[i] + lm->x[2] * lm->u[i] + lm->x[3] * lm->v[i]);
  }
  sac_normalized3v(c[3], c[4], c[5]);
  c[6] = float(fabs(lm->x[4]));
  for (int i = 0; i < 7; ++i)
    if (!(__builtin_fabsf(c[i]) <= FLT_MAX)) return;
  for (int i = 0; i < 7; ++i) cy->coef[i] = c[i];
  cy->refined = 1u;
}

// ---- the host side ----

// the least float e >= 0 with om * double(e) > thr, by bisection over the bits; NaN when there is none or no tier 1
// (ndw outside [0, 1]): e >= NaN is false for every e
float sac_cylinder_e_out(double ndw, double om, double thr) {
  const float none = std::numeric_limits<float>::quiet_NaN();
  if (!(ndw >= 0.0 && ndw <= 1.0)) return none;
  auto out = [&](uint32_t bits) {
    float e;
    std::memcpy(&e, &bits, 4);
    return om * double(e) > thr;
  };
  uint32_t lo = 0u, hi = 0x7F800000u;  // +0 .. +inf
  if (!out(hi)) return none;
  if (out(lo)) return 0.0f;
  while (hi - lo > 1u) {  // out(lo) false, out(hi) true
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (out(mid)) hi = mid; else lo = mid;
  }
  float e;
  std::memcpy(&e, &hi, 4);
  return e;
}

struct SacCyl {  // what a cylinder call holds
  SacCloud pc;
  SacDev* st = nullptr;        // bad_index, the scan's totals
  SacCylDev* cy = nullptr;
  SacCylGate gate;
  const char* nrec = nullptr;  // the normal records on the device
  size_t nstride = 0;
  uint64_t n_rec = 0;
  float4* nn = nullptr;        // the point set's unit normals
  double ndw = 0.1, om = 0.9;
};

pclhip_status sac_cylinder_gate_of(pclhip_ctx* ctx, const pclhip_sac_cylinder_params* CP, SacCylGate* g) {
  PCLHIP_REQUIRE(ctx, !(CP->radius_min > CP->radius_max), "radius_min must not exceed radius_max");
  std::memset(g, 0, sizeof *g);
  g->angle_on = CP->eps_angle > 0.0 ? 1 : 0;
  g->ax = CP->axis[0]; g->ay = CP->axis[1]; g->az = CP->axis[2];
  g->eps_angle = CP->eps_angle;
  g->rmin = CP->radius_min;
  g->rmax = CP->radius_max;
  PCLHIP_REQUIRE(ctx, !g->angle_on || g->ax != 0.0f || g->ay != 0.0f || g->az != 0.0f, "eps_angle > 0 needs an axis that is not zero");
  return PCLHIP_OK;
}

// the parameters checked, the point set and its unit normals staged, the indices checked (one synchronisation)
pclhip_status sac_cylinder_setup(pclhip_ctx* ctx, DeviceScope& scope, const void* cloud, uint64_t n_rec, size_t stride,
                                 const void* normals, size_t nstride, bool need_normals, const int32_t* indices,
                                 uint64_t n_indices, const pclhip_sac_cylinder_params* CP, SacCyl* K) {
  hipStream_t s = ctx->stream;
  pclhip_status rc = sac_checked_params(ctx, cloud, n_rec, stride, indices, n_indices);
  if (rc != PCLHIP_OK) return rc;
  if ((rc = sac_cylinder_gate_of(ctx, CP, &K->gate)) != PCLHIP_OK) return rc;
  if (need_normals) {
    PCLHIP_REQUIRE(ctx, normals != nullptr || n_rec == 0, "the cylinder model needs the normals, one record per record of the cloud");
    PCLHIP_REQUIRE(ctx, nstride >= 16 && nstride % 4 == 0, "normals stride must be a multiple of 4 and >= 16 bytes");
  }
  K->ndw = CP->normal_distance_weight;
  K->om = 1.0 - CP->normal_distance_weight;
  K->nstride = nstride;
  K->n_rec = n_rec;
  PCLHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&K->st, sizeof(SacDev)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(K->st, 0, sizeof(SacDev), s));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&K->cy, sizeof(SacCylDev)));
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(K->cy, 0, sizeof(SacCylDev), s));
  if ((rc = sac_stage(ctx, scope, cloud, n_rec, stride, indices, n_indices, K->st, &K->pc)) != PCLHIP_OK) return rc;
  if (K->pc.n == 0) return PCLHIP_OK;
  if (need_normals) {
    const void* dn = nullptr;
    void* owned = nullptr;
    if ((rc = to_device(ctx, normals, size_t(n_rec) * nstride, &dn, &owned)) != PCLHIP_OK) return rc;
    if (owned) scope.mem.push_back(owned);
    K->nrec = static_cast<const char*>(dn);
    double* wt = nullptr;  // (the normal plane's weights, not read here: the cylinder's weight is the plain ndw, :170)
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&K->nn, size_t(K->pc.n) * sizeof(float4)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&wt, size_t(K->pc.n) * sizeof(double)));
    hipLaunchKernelGGL(sac_normals_gather_kernel, sac_blocks_of(K->pc.n), dim3(SAC_BLOCK), 0, s, K->nrec, nstride, n_rec,
                       K->pc.idx, K->pc.n, K->ndw, K->nn, wt);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  }
  SacDev h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, K->st, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  PCLHIP_REQUIRE(ctx, h.bad_index == 0u, "an entry of indices lies outside the cloud");
  return PCLHIP_OK;
}

uint32_t sac_cylinder_count_grid(const pclhip_ctx* ctx, uint32_t n) {
  static int per_cu = 0;
  if (per_cu == 0) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, sac_cylinder_count_kernel, SAC_BLOCK, 0) != hipSuccess || v < 1) {
      (void)hipGetLastError();
      v = 4;
    }
    per_cu = v;
  }
  const uint64_t tiles = (uint64_t(n) + SACC_TILE - 1) / SACC_TILE;
  const uint64_t most = uint64_t(per_cu) * uint64_t(ctx->num_cus > 0 ? ctx->num_cus : 1);
  return uint32_t(tiles < most ? (tiles > 0 ? tiles : 1) : most);
}

// the gate and the scoring pass of H hypotheses (trace records, or septuples on the device); counts[] is zero before it
void sac_cylinder_score(const pclhip_ctx* ctx, const SacCyl& K, const pclhip_sac_cylinder_trace* rec, const float* coeffs,
                        float4* A, float4* B, uint32_t* valid, uint32_t H, double thr, float e_out, uint32_t* counts,
                        hipEvent_t ea, hipEvent_t eb) {
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(sac_cylinder_prepare_kernel, sac_blocks_of(H), dim3(SAC_BLOCK), 0, s, K.gate, H, rec, coeffs, A, B, valid);
  if (ea) (void)hipEventRecord(ea, s);
  if (K.pc.n > 0)
    hipLaunchKernelGGL(sac_cylinder_count_kernel, dim3(sac_cylinder_count_grid(ctx, K.pc.n)), dim3(SAC_BLOCK), 0, s, K.pc.pts, K.nn,
                       K.pc.n, A, B, H, K.ndw, K.om, thr, e_out, counts);
  if (eb) (void)hipEventRecord(eb, s);
}

// the scratch of a selection
struct SacCylSelect {
  uint32_t *flag = nullptr, *excl = nullptr;
  uint2* part = nullptr;
  pclhip_status alloc(pclhip_ctx* ctx, DeviceScope& scope, uint32_t n) {
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&flag, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&excl, size_t(n) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&part, size_t((uint64_t(n) + SC_BLOCK - 1) / SC_BLOCK + 1) * sizeof(uint2)));
    return PCLHIP_OK;
  }
  // the gate, the flags and their scan with the coefficients the device holds: st->tot[0] = inliers
  void run(const pclhip_ctx* ctx, const SacCyl& K, double thr) {
    hipStream_t s = ctx->stream;
    (void)hipMemsetAsync(K.st->tot, 0, 16, s);
    hipLaunchKernelGGL(sac_cylinder_gate_held_kernel, dim3(1), dim3(WAVE), 0, s, K.gate, K.cy);
    hipLaunchKernelGGL(sac_cylinder_flag_kernel, sac_blocks_of(K.pc.n), dim3(SAC_BLOCK), 0, s, K.pc.pts, K.nn, K.pc.n, K.cy, K.ndw,
                       K.om, thr, flag);
    launch_scan_u32(s, flag, K.pc.n, part, K.st->tot, excl);
  }
};

// optimizeModelCoefficients on the m points at pos_list (null: positions 0 .. m-1) with the coefficients the device holds;
// the caller has run the gate (cy->invalid) and checked m > 2
pclhip_status sac_cylinder_refit(pclhip_ctx* ctx, DeviceScope& scope, const SacCyl& K, const uint32_t* pos_list, uint32_t m) {
  hipStream_t s = ctx->stream;
  uint32_t blocks = (m + SAC_BLOCK - 1) / SAC_BLOCK;
  if (blocks > uint32_t(SAC_MOMENT_BLOCKS)) blocks = uint32_t(SAC_MOMENT_BLOCKS);
  double *partials = nullptr, *sums = nullptr;
  SacCylLM* lm = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&partials, size_t(blocks) * SACC_NS * sizeof(double)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&sums, SACC_NS * sizeof(double)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&lm, sizeof(SacCylLM)));
  hipLaunchKernelGGL(sac_cylinder_centroid_kernel, dim3(blocks), dim3(SAC_BLOCK), 0, s, K.pc.pts, pos_list, m, partials);
  hipLaunchKernelGGL(block_sums_finalize_kernel<3>, dim3(3), dim3(WAVE), 0, s, partials, int(blocks), sums);
  hipLaunchKernelGGL(sac_cylinder_frame_kernel, dim3(1), dim3(WAVE), 0, s, sums, m, K.cy, lm);
  // (the first pass evaluates the start; every later one a step)
  for (int done = 0; done < SACC_LM_CAP + 1; done += SACC_LM_CHUNK) {
    for (int i = 0; i < SACC_LM_CHUNK && done + i < SACC_LM_CAP + 1; ++i) {
      hipLaunchKernelGGL(sac_cylinder_lm_pass_kernel, dim3(blocks), dim3(SAC_BLOCK), 0, s, K.pc.pts, pos_list, m, lm, partials);
      hipLaunchKernelGGL(block_sums_finalize_kernel<SACC_NS>, dim3(SACC_NS), dim3(WAVE), 0, s, partials, int(blocks), sums);
      hipLaunchKernelGGL(sac_cylinder_lm_step_kernel, dim3(1), dim3(WAVE), 0, s, sums, lm);
    }
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    uint32_t stop = 0u;
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&stop, &lm->stop, 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    if (stop != 0u) break;
  }
  hipLaunchKernelGGL(sac_cylinder_lm_finish_kernel, dim3(1), dim3(WAVE), 0, s, lm, K.cy);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  return PCLHIP_OK;
}

}  // namespace
}  // namespace pclhip

extern "C" {

void pclhip_sac_cylinder_params_default(pclhip_sac_cylinder_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->normal_distance_weight = 0.1;  // SACSegmentationFromNormals' default (sac_segmentation.h:397)
  p->radius_min = -DBL_MAX;         // not set (sac_model.h:88-89)
  p->radius_max = DBL_MAX;
}

pclhip_status pclhip_sac_cylinder_segment(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const void* normals,
                                          size_t nstride, const int32_t* indices, uint64_t n_indices,
                                          const pclhip_sac_plane_params* P, const pclhip_sac_cylinder_params* CP,
                                          float out_coeff[7], int32_t* out_inliers, uint64_t inliers_capacity,
                                          uint64_t* out_n_inliers, int32_t* out_outliers, uint64_t outliers_capacity,
                                          uint64_t* out_n_outliers, pclhip_sac_plane_stats* out_stats) {
  using namespace pclhip;
  if (!ctx || !P || !CP || !out_coeff || !out_n_inliers) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *out_n_inliers = 0;
  if (out_n_outliers) *out_n_outliers = 0;
  for (int i = 0; i < 7; ++i) out_coeff[i] = 0.0f;
  pclhip_sac_plane_stats stats;
  std::memset(&stats, 0, sizeof stats);
  stats.best_trial = -1;
  if (out_stats) *out_stats = stats;
  ctx->sac_cylinder_trace.clear();
  PCLHIP_REQUIRE(ctx, P->max_iterations >= 0 && P->max_iterations <= 100000000, "max_iterations must be in 0 .. 1e8");
  PCLHIP_REQUIRE(ctx, P->probability >= 0.0 && P->probability <= 1.0, "the probability must be in [0, 1]");
  PCLHIP_REQUIRE(ctx, P->batch_size >= 0 && P->batch_size <= SAC_MAX_BATCH, "batch_size must be in 0 .. 1024");
  PCLHIP_REQUIRE(ctx, (out_inliers != nullptr || inliers_capacity == 0) && (out_outliers != nullptr || outliers_capacity == 0),
                 "a capacity without a buffer");
  DeviceScope scope(ctx);
  SacCyl K;
  pclhip_status rc = sac_cylinder_setup(ctx, scope, cloud, n_rec, stride, normals, nstride, true, indices, n_indices, CP, &K);
  if (rc != PCLHIP_OK) return rc;
  hipStream_t s = ctx->stream;
  hipEvent_t ev_call[2] = {nullptr, nullptr};
  PCLHIP_CHECK_HIP(ctx, scope.event(&ev_call[0]));
  PCLHIP_CHECK_HIP(ctx, scope.event(&ev_call[1]));
  (void)hipEventRecord(ev_call[0], s);
  const uint32_t n = K.pc.n;
  const double thr = P->distance_threshold;
  const float e_out = sac_cylinder_e_out(K.ndw, K.om, thr);
  const int cap = P->batch_size > 0 ? P->batch_size : SAC_MAX_BATCH;

  // ---- the trials ----
  sac::Replay rp;
  rp.start(P->max_iterations, P->probability, n > 0 ? n : 1, 2);
  pclhip_sac_cylinder_trace best_rec;
  std::memset(&best_rec, 0, sizeof best_rec);
  std::vector<hipEvent_t> ev_count;
  if (n >= 2) {  // (fewer points: getSamples finds no sample, ransac.hpp:120-124)
    pclhip_sac_cylinder_trace* rec = nullptr;
    float4 *A = nullptr, *B = nullptr;
    uint32_t *counts = nullptr, *valid = nullptr;
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&rec, size_t(cap) * sizeof(pclhip_sac_cylinder_trace)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&A, size_t(cap) * sizeof(float4)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&B, size_t(cap) * sizeof(float4)));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&counts, size_t(cap) * 4));
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&valid, size_t(cap) * 4));
    std::vector<pclhip_sac_cylinder_trace> hrec(static_cast<size_t>(cap));
    std::vector<uint32_t> hcnt(static_cast<size_t>(cap)), hval(static_cast<size_t>(cap));
    uint64_t t0 = 0;
    int Bn = P->batch_size > 0 ? P->batch_size : SAC_AUTO_BATCH;
    while (!rp.done) {
      // no batch holds more trials than the loop can still score: one pass covers a call that meets no skip
      const int64_t left = int64_t(P->max_iterations) + 1 - rp.iterations;
      const uint32_t nit = uint32_t(left < Bn ? (left > 0 ? left : 1) : Bn);
      hipEvent_t ea = nullptr, eb = nullptr;
      PCLHIP_CHECK_HIP(ctx, scope.event(&ea));
      PCLHIP_CHECK_HIP(ctx, scope.event(&eb));
      hipLaunchKernelGGL(sac_cylinder_hypothesis_kernel, sac_blocks_of(nit), dim3(SAC_BLOCK), 0, s, P->seed, uint32_t(t0), nit, n,
                         K.pc.pts, K.nrec, K.nstride, K.n_rec, K.pc.idx, K.gate.rmin, K.gate.rmax, rec);
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, size_t(nit) * 4, s));
      sac_cylinder_score(ctx, K, rec, nullptr, A, B, valid, nit, thr, e_out, counts, ea, eb);
      PCLHIP_CHECK_HIP(ctx, hipGetLastError());
      ev_count.push_back(ea);
      ev_count.push_back(eb);
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hrec.data(), rec, size_t(nit) * sizeof(pclhip_sac_cylinder_trace), hipMemcpyDeviceToHost, s));
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hcnt.data(), counts, size_t(nit) * 4, hipMemcpyDeviceToHost, s));
      PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hval.data(), valid, size_t(nit) * 4, hipMemcpyDeviceToHost, s));
      PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
      ++stats.batches;
      for (uint32_t t = 0; t < nit; ++t) {
        hrec[t].valid = hval[t] != 0u ? 1 : 0;
        hrec[t].count = hrec[t].valid ? hcnt[t] : 0u;
        const uint32_t before = rp.best;
        const bool more = rp.feed(hrec[t].skipped != 0, hrec[t].count);  // (an invalid trial: an iteration that counts 0)
        if (rp.best != before) best_rec = hrec[t];
        if (ctx->sac_cylinder_trace.size() < SAC_TRACE_MAX) ctx->sac_cylinder_trace.push_back(hrec[t]);
        if (!more) break;
      }
      t0 += nit;
      if (P->batch_size == 0 && Bn < SAC_MAX_BATCH) Bn *= 2;
      if (t0 + uint64_t(SAC_MAX_BATCH) >= 0xFFFFFFFFull) break;  // (the draw counter holds 32 bits)
    }
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
  SacCylDev hcy;
  std::memset(&hst, 0, sizeof hst);
  std::memset(&hcy, 0, sizeof hcy);
  int32_t *inl = nullptr, *outl = nullptr;
  SacCylSelect sel;
  if (found) {
    if ((rc = sel.alloc(ctx, scope, n)) != PCLHIP_OK) return rc;
    const bool inl_dev = out_inliers && is_device_pointer(out_inliers) && inliers_capacity >= n;
    const bool outl_dev = out_outliers && is_device_pointer(out_outliers) && outliers_capacity >= n;
    if (inl_dev) inl = out_inliers; else PCLHIP_CHECK_HIP(ctx, scope.alloc(&inl, size_t(n) * 4));
    if (out_outliers || out_n_outliers) {
      if (outl_dev) outl = out_outliers; else PCLHIP_CHECK_HIP(ctx, scope.alloc(&outl, size_t(n) * 4));
    }
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(K.cy->coef, best_rec.coefficients, 28, hipMemcpyHostToDevice, s));
    sel.run(ctx, K, thr);
    if (P->optimize_coefficients && rp.best > 2u) {
      // the first selection has rp.best inliers by construction: the same function on the same points (and the winner is valid)
      const uint32_t m = rp.best;
      uint32_t* pos = nullptr;
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&pos, size_t(m) * 4));
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(pos, 0, size_t(m) * 4, s));
      hipLaunchKernelGGL(sac_positions_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, sel.flag, sel.excl, n, pos, m);
      if ((rc = sac_cylinder_refit(ctx, scope, K, pos, m)) != PCLHIP_OK) return rc;
      sel.run(ctx, K, thr);
    }
    hipLaunchKernelGGL(sac_lists_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, sel.flag, sel.excl, n, K.pc.idx, inl, outl);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hst, K.st, sizeof hst, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hcy, K.cy, sizeof hcy, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    n_in = hst.tot[0];
    for (int i = 0; i < 7; ++i) out_coeff[i] = hcy.coef[i];
    stats.refined = int(hcy.refined);
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
      int32_t* all = nullptr;
      if ((rc = sel.alloc(ctx, scope, n)) != PCLHIP_OK) return rc;
      PCLHIP_CHECK_HIP(ctx, scope.alloc(&all, size_t(n) * 4));
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(sel.flag, 0, size_t(n) * 4, s));
      PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(sel.excl, 0, size_t(n) * 4, s));
      hipLaunchKernelGGL(sac_lists_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, sel.flag, sel.excl, n, K.pc.idx,
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
    set_error(ctx, "pclhip_sac_cylinder_segment: capacity too small (the counts hold the required sizes)");
    return PCLHIP_ERR_OVERFLOW;
  }
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_cylinder_model(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const void* normals,
                                        size_t nstride, const int32_t samples[2], const pclhip_sac_cylinder_params* CP,
                                        float out_coeff[7], int* out_found) {
  using namespace pclhip;
  if (!ctx || !CP || !samples || !out_coeff || !out_found) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *out_found = 0;
  for (int i = 0; i < 7; ++i) out_coeff[i] = 0.0f;
  PCLHIP_REQUIRE(ctx, n_rec > 0, "a sample of an empty cloud");
  DeviceScope scope(ctx);
  SacCyl K;
  // (the point set is the sample itself: positions 0 and 1, in the order given)
  pclhip_status rc = sac_cylinder_setup(ctx, scope, cloud, n_rec, stride, normals, nstride, true, samples, 2, CP, &K);
  if (rc != PCLHIP_OK) return rc;
  hipStream_t s = ctx->stream;
  pclhip_sac_cylinder_trace* rec = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&rec, sizeof(pclhip_sac_cylinder_trace)));
  hipLaunchKernelGGL(sac_cylinder_model_kernel, dim3(1), dim3(WAVE), 0, s, K.pc.pts, K.nrec, K.nstride, K.n_rec, K.pc.idx,
                     K.gate.rmin, K.gate.rmax, rec);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  pclhip_sac_cylinder_trace h;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&h, rec, sizeof h, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  *out_found = h.skipped ? 0 : 1;
  for (int i = 0; i < 7; ++i) out_coeff[i] = h.coefficients[i];
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_cylinder_evaluate(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const void* normals,
                                           size_t nstride, const int32_t* indices, uint64_t n_indices, double threshold,
                                           const pclhip_sac_cylinder_params* CP, const float* coeffs, int n_models,
                                           uint32_t* out_counts, uint8_t* out_valid) {
  using namespace pclhip;
  if (!ctx || !CP || n_models < 0 || (n_models > 0 && (!coeffs || !out_counts))) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  DeviceScope scope(ctx);
  SacCyl K;
  pclhip_status rc = sac_cylinder_setup(ctx, scope, cloud, n_rec, stride, normals, nstride, true, indices, n_indices, CP, &K);
  if (rc != PCLHIP_OK) return rc;
  for (int m = 0; m < n_models; ++m) out_counts[m] = 0u;
  if (out_valid) for (int m = 0; m < n_models; ++m) out_valid[m] = 1;
  if (n_models == 0) return PCLHIP_OK;
  hipStream_t s = ctx->stream;
  const float e_out = sac_cylinder_e_out(K.ndw, K.om, threshold);
  float* dco = nullptr;
  float4 *A = nullptr, *B = nullptr;
  uint32_t *counts = nullptr, *valid = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&dco, size_t(SAC_MAX_BATCH) * 7 * sizeof(float)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&A, size_t(SAC_MAX_BATCH) * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&B, size_t(SAC_MAX_BATCH) * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&counts, size_t(SAC_MAX_BATCH) * 4));
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&valid, size_t(SAC_MAX_BATCH) * 4));
  std::vector<uint32_t> hval(static_cast<size_t>(SAC_MAX_BATCH));
  for (int m0 = 0; m0 < n_models; m0 += SAC_MAX_BATCH) {
    const uint32_t H = uint32_t(n_models - m0 < SAC_MAX_BATCH ? n_models - m0 : SAC_MAX_BATCH);
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(dco, coeffs + size_t(m0) * 7, size_t(H) * 7 * sizeof(float), hipMemcpyHostToDevice, s));
    PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, size_t(H) * 4, s));
    sac_cylinder_score(ctx, K, nullptr, dco, A, B, valid, H, threshold, e_out, counts, nullptr, nullptr);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_counts + m0, counts, size_t(H) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(hval.data(), valid, size_t(H) * 4, hipMemcpyDeviceToHost, s));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    if (out_valid) for (uint32_t h = 0; h < H; ++h) out_valid[m0 + h] = hval[h] != 0u ? 1 : 0;
  }
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_cylinder_select(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const void* normals,
                                         size_t nstride, const int32_t* indices, uint64_t n_indices, double threshold,
                                         const pclhip_sac_cylinder_params* CP, const float coeff[7], int32_t* out_inliers,
                                         uint64_t inliers_capacity, uint64_t* out_n_inliers) {
  using namespace pclhip;
  if (!ctx || !CP || !coeff || !out_n_inliers || (!out_inliers && inliers_capacity > 0)) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *out_n_inliers = 0;
  DeviceScope scope(ctx);
  SacCyl K;
  pclhip_status rc = sac_cylinder_setup(ctx, scope, cloud, n_rec, stride, normals, nstride, true, indices, n_indices, CP, &K);
  if (rc != PCLHIP_OK) return rc;
  const uint32_t n = K.pc.n;
  if (n == 0) return PCLHIP_OK;
  hipStream_t s = ctx->stream;
  SacCylSelect sel;
  if ((rc = sel.alloc(ctx, scope, n)) != PCLHIP_OK) return rc;
  int32_t* inl = nullptr;
  PCLHIP_CHECK_HIP(ctx, scope.alloc(&inl, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(K.cy->coef, coeff, 28, hipMemcpyHostToDevice, s));
  sel.run(ctx, K, threshold);
  hipLaunchKernelGGL(sac_lists_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, sel.flag, sel.excl, n, K.pc.idx, inl,
                     static_cast<int32_t*>(nullptr));
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  SacDev hst;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hst, K.st, sizeof hst, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  *out_n_inliers = hst.tot[0];
  if (out_inliers == nullptr) return PCLHIP_OK;
  if (inliers_capacity < hst.tot[0]) {
    set_error(ctx, "pclhip_sac_cylinder_select: capacity too small (the count holds the required size)");
    return PCLHIP_ERR_OVERFLOW;
  }
  if ((rc = sac_copy_out(ctx, out_inliers, inl, hst.tot[0])) != PCLHIP_OK) return rc;
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_cylinder_distances(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride, const void* normals,
                                            size_t nstride, const int32_t* indices, uint64_t n_indices,
                                            const pclhip_sac_cylinder_params* CP, const float coeff[7], double* out_distances,
                                            uint64_t capacity, uint64_t* out_n) {
  using namespace pclhip;
  if (!ctx || !CP || !coeff || !out_n || (!out_distances && capacity > 0)) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *out_n = 0;
  DeviceScope scope(ctx);
  SacCyl K;
  pclhip_status rc = sac_cylinder_setup(ctx, scope, cloud, n_rec, stride, normals, nstride, true, indices, n_indices, CP, &K);
  if (rc != PCLHIP_OK) return rc;
  const uint32_t n = K.pc.n;
  hipStream_t s = ctx->stream;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(K.cy->coef, coeff, 28, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(sac_cylinder_gate_held_kernel, dim3(1), dim3(WAVE), 0, s, K.gate, K.cy);
  double* dist = nullptr;
  if (n > 0) {
    PCLHIP_CHECK_HIP(ctx, scope.alloc(&dist, size_t(n) * sizeof(double)));
    hipLaunchKernelGGL(sac_cylinder_distance_kernel, sac_blocks_of(n), dim3(SAC_BLOCK), 0, s, K.pc.pts, K.nn, n, K.cy, K.ndw, K.om,
                       dist);
  }
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  SacCylDev hcy;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hcy, K.cy, sizeof hcy, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  if (hcy.invalid != 0u || n == 0) return PCLHIP_OK;  // :148-152: an invalid model has no distances
  *out_n = n;
  if (out_distances == nullptr) return PCLHIP_OK;
  if (capacity < n) {
    set_error(ctx, "pclhip_sac_cylinder_distances: capacity too small (the count holds the required size)");
    return PCLHIP_ERR_OVERFLOW;
  }
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(out_distances, dist, size_t(n) * sizeof(double), hipMemcpyDefault, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_cylinder_optimize(pclhip_ctx* ctx, const void* cloud, uint64_t n_rec, size_t stride,
                                           const int32_t* inliers, uint64_t n_inliers, const pclhip_sac_cylinder_params* CP,
                                           const float coeff[7], float out_coeff[7], int* out_refined, int* out_iterations) {
  using namespace pclhip;
  if (!ctx || !CP || !coeff || !out_coeff || (!inliers && n_inliers > 0)) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  for (int i = 0; i < 7; ++i) out_coeff[i] = coeff[i];
  if (out_refined) *out_refined = 0;
  if (out_iterations) *out_iterations = 0;
  DeviceScope scope(ctx);
  SacCyl K;
  const int32_t none = 0;
  // (the point set is the inlier list: positions 0 .. m-1; the refit reads no normal)
  pclhip_status rc = sac_cylinder_setup(ctx, scope, cloud, n_rec, stride, nullptr, 0, false, inliers ? inliers : &none, n_inliers,
                                        CP, &K);
  if (rc != PCLHIP_OK) return rc;
  hipStream_t s = ctx->stream;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(K.cy->coef, coeff, 28, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(sac_cylinder_gate_held_kernel, dim3(1), dim3(WAVE), 0, s, K.gate, K.cy);
  SacCylDev hcy;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hcy, K.cy, sizeof hcy, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  if (hcy.invalid != 0u || K.pc.n <= 2u) return PCLHIP_OK;  // impl/sac_model_cylinder.hpp:275-286
  if ((rc = sac_cylinder_refit(ctx, scope, K, nullptr, K.pc.n)) != PCLHIP_OK) return rc;
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(&hcy, K.cy, sizeof hcy, hipMemcpyDeviceToHost, s));
  PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
  for (int i = 0; i < 7; ++i) out_coeff[i] = hcy.coef[i];
  if (out_refined) *out_refined = int(hcy.refined);
  if (out_iterations) *out_iterations = int(hcy.lm_iterations);
  return PCLHIP_OK;
}

pclhip_status pclhip_sac_last_cylinder_trace(pclhip_ctx* ctx, pclhip_sac_cylinder_trace* buf, uint64_t capacity, uint64_t* count) {
  if (!ctx || !count || (capacity > 0 && !buf)) return PCLHIP_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mutex);
  *count = ctx->sac_cylinder_trace.size();
  const uint64_t m = capacity < *count ? capacity : *count;
  if (m > 0) std::memcpy(buf, ctx->sac_cylinder_trace.data(), size_t(m) * sizeof(pclhip_sac_cylinder_trace));
  return PCLHIP_OK;
}

#ifdef PCLHIP_SACC_STATS
// pairs that reached tier 2 since the last call of this function (scripts/sac_cylinder_timing.py's own build)
PCLHIP_API unsigned long long pclhip_sacc_exact_pairs_take(void) {
  unsigned long long v = 0, zero = 0;
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(pclhip::sacc_exact_pairs), sizeof v);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(pclhip::sacc_exact_pairs), &zero, sizeof zero);
  return v;
}
#endif

}  // extern "C"
