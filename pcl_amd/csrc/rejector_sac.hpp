// rejector_sac.hpp -- CorrespondenceRejectorSampleConsensus (registration/include/pcl/registration/impl/
// correspondence_rejection_sample_consensus.hpp:55-142, sample_consensus/.../impl/sac_model_registration.hpp:48-97,203-249,
// 289-322, sac_model_registration.h:264-289, sac_model.h:162-197, impl/ransac.hpp:56-217; the semantics are stated in
// include/pclhip.h).  Included by rejectors.hip, which holds the host side of the chain kind and of the standalone call.
//
// One run, stream-ordered, without the host in between (it is part of the device-driven ICP loop):
//   the pairs               per slot one float4 source and one float4 target record, gathered once (NaN where a slot holds
//                           no pair); in the chain the slots are the registration's, and a list (position -> slot) in
//                           ascending original query index comes from a scatter of the keep bits, a scan and a compaction;
//                           in the standalone call the slots are the list
//   rejsac_moments_kernel   the nine sums of computeMeanAndCovarianceMatrix over the list's source points and their count,
//                           in double in block_sums.hpp's fixed order on a grid that does not depend on the list
//   rejsac_threshold_kernel one thread: covariance rounded once to float, normals_math.hpp's eigenvalues, the sample distance
//                           threshold; the replay's state
// then batches of trials, queued up front (a small first one, then doubling); every kernel of a batch returns at once when
// the loop has ended:
//   rejsac_hypothesis_kernel  one thread per trial: the attempts (scp_draw.hpp), isSampleGood, umeyama in double
//                             (scp_umeyama.hpp); T, the attempts and the no-sample flag
//   rejsac_count_kernel       the hot path: pairs x hypotheses.  A lane keeps RSAC_P pairs in registers (packed two by two),
//                             the wave walks the batch's hypotheses -- their twelve floats are wave-uniform reads -- and per
//                             (hypothesis, pair slot) one compare gives a ballot whose popcount goes to a wave-uniform
//                             counter.  Lane h % 64 keeps the wave's count of hypothesis h; every 64 hypotheses the lanes add
//                             theirs to the block's LDS counters, and the block adds those to counts[h] once, after its last
//                             tile.  Integer adds: the order never shows.  Every pair is read once per batch.
//   rejsac_replay_kernel      one thread: the batch's counts in trial order through the stopping rule (sac_replay.hpp's
//                             without its skip branch); best trial, iterations, the winner's T and the `done` flag
// and behind them:
//   rejsac_finish_kernel    one thread: "no model" and "fewer than 3 inliers" leave the list as it is and T the identity
//   rejsac_keep_kernel      chain: the winner's flags ANDed into keep
//   rejsac_flag_kernel      standalone: the flags, then scan and compaction (device_scan.hpp) to the list of positions
#pragma once

#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "block_sums.hpp"
#include "device_scan.hpp"
#include "normals_math.hpp"
#include "scp_draw.hpp"
#include "scp_umeyama.hpp"

namespace pclhip {
namespace {

constexpr int RSAC_BLOCK = 256;
constexpr int RSAC_WAVES = RSAC_BLOCK / WAVE;
constexpr int RSAC_P = 8;                            // pairs a lane keeps in registers (six floats each)
constexpr int RSAC_TILE = RSAC_BLOCK * RSAC_P;       // pairs a block scores per step
constexpr int RSAC_MAX_BATCH = 1024;                 // hypotheses of a pass (the block's LDS counters)
constexpr int RSAC_FIRST_BATCH = 16;                 // first batch of a run that names none; doubles up to RSAC_MAX_BATCH
constexpr int RSAC_MOMENT_BLOCKS = 256;              // rows of the moments, whatever the list's length: the order of the
                                                     // sums is a function of that length alone
constexpr int RSAC_MOMENT_ROW = 10;                  // xx xy xz yy yz zz x y z and the number of finite points
constexpr uint32_t RSAC_MAX_SAMPLE_CHECKS = 1000;    // getMaxSampleChecks (sac_model.h)
constexpr uint64_t RSAC_TRACE_MAX = 65536;
constexpr int RSAC_MAX_ITERATIONS = 1000000;

struct RsacPairs {         // kernel argument
  const float4* src;       // per slot: the source point (NaN where the slot holds no pair)
  const float4* tgt;       // ... and its match
  const uint32_t* list;    // list position -> slot (nullptr: the slots are the list)
  const uint32_t* m_dev;   // the list's length in device memory (nullptr: m_host)
  uint32_t m_host;
  uint32_t slots;
};

struct RsacRun {
  double threshold;
  int max_iterations;
  double probability;
  uint64_t seed;
  int batch_size;
};

inline dim3 rsac_blocks_of(uint64_t n) { return dim3(uint32_t((n + RSAC_BLOCK - 1) / RSAC_BLOCK)); }

// the largest float whose double is below threshold^2: double(d2) < threshold * threshold  <=>  d2 <= rsac_float_bound
inline float rsac_float_bound(double threshold) {
  const double t2 = threshold * threshold;
  if (!(t2 == t2)) return __builtin_nanf("");
  float f = t2 > double(FLT_MAX) ? FLT_MAX : float(t2);
  while (double(f) >= t2) f = std::nextafterf(f, -INFINITY);
  return f;
}

// the batches of a run: [first trial, trials), together max_iterations + 1 trials (the loop ends at the latest when
// iterations exceeds max_iterations)
inline std::vector<std::pair<uint32_t, uint32_t>> rsac_schedule(int max_iterations, int batch_size) {
  std::vector<std::pair<uint32_t, uint32_t>> out;
  const uint32_t total = uint32_t(max_iterations) + 1u;
  uint32_t b = batch_size > 0 ? uint32_t(batch_size) : uint32_t(RSAC_FIRST_BATCH);
  if (b > uint32_t(RSAC_MAX_BATCH)) b = uint32_t(RSAC_MAX_BATCH);
  for (uint32_t it0 = 0; it0 < total;) {
    const uint32_t nit = total - it0 < b ? total - it0 : b;
    out.emplace_back(it0, nit);
    it0 += nit;
    if (batch_size <= 0 && b < uint32_t(RSAC_MAX_BATCH)) b *= 2u;
  }
  return out;
}

// ---- the pairs ------------------------------------------------------------------------------------------------------------
// standalone: pair j = (source[index_query[j]], target[index_match[j]]); an index outside its cloud and a query index listed
// twice (one pass over a bitmap of the source) are reported in the state
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_gather_kernel(const char* __restrict__ srec, size_t sstride, uint64_t n_src,
                                                                   const char* __restrict__ trec, size_t tstride, uint64_t n_tgt,
                                                                   const int32_t* __restrict__ iq, const int32_t* __restrict__ im,
                                                                   uint32_t n, uint32_t* __restrict__ bitmap,
                                                                   float4* __restrict__ S, float4* __restrict__ T,
                                                                   RejSacState* __restrict__ st) {
  const uint32_t i = blockIdx.x * RSAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float nan = __builtin_nanf("");
  float4 s = make_float4(nan, nan, nan, 0.0f), t = s;
  const int64_t q = iq[i], m = im[i];
  if (q >= 0 && uint64_t(q) < n_src && m >= 0 && uint64_t(m) < n_tgt) {
    const float* a = reinterpret_cast<const float*>(srec + size_t(q) * sstride);
    const float* b = reinterpret_cast<const float*>(trec + size_t(m) * tstride);
    s.x = a[0]; s.y = a[1]; s.z = a[2];
    t.x = b[0]; t.y = b[1]; t.z = b[2];
    if (bitmap != nullptr) {
      const uint32_t bit = 1u << (uint32_t(q) & 31u);
      if (atomicOr(&bitmap[uint32_t(q) >> 5], bit) & bit) st->duplicate = 1u;  // (every writer stores the same value)
    }
  } else {
    st->bad_index = 1u;
  }
  S[i] = s;
  T[i] = t;
}

// chain: the keep bits by ORIGINAL query index (a scan of them numbers the list) ...
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_scatter_keep_kernel(const float4* __restrict__ cur,
                                                                         const uint8_t* __restrict__ keep, uint32_t n,
                                                                         uint32_t n_orig, uint32_t* __restrict__ by_orig) {
  const uint32_t i = blockIdx.x * RSAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = __float_as_uint(cur[i].w);
  if (o < n_orig) by_orig[o] = keep[i] ? 1u : 0u;
}
// ... list position -> slot, and the pair records slot by slot
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_gather_icp_kernel(const float4* __restrict__ cur,
                                                                       const float4* __restrict__ tgt_pts,
                                                                       const uint32_t* __restrict__ match_pos,
                                                                       const uint8_t* __restrict__ keep, uint32_t n,
                                                                       uint32_t n_orig, const uint32_t* __restrict__ excl,
                                                                       uint32_t* __restrict__ list, float4* __restrict__ S,
                                                                       float4* __restrict__ T) {
  const uint32_t i = blockIdx.x * RSAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float nan = __builtin_nanf("");
  float4 s = make_float4(nan, nan, nan, 0.0f), t = s;
  const float4 c = cur[i];
  const uint32_t o = __float_as_uint(c.w), pos = match_pos[i];
  if (keep[i] && o < n_orig) {  // (the condition of rejsac_scatter_keep_kernel: the list holds exactly these slots)
    list[excl[o]] = i;
    if (pos != NO_INDEX) {      // (a kept slot has a match: rej_init_kernel)
      const float4 q = tgt_pts[pos];
      s.x = c.x; s.y = c.y; s.z = c.z;
      t.x = q.x; t.y = q.y; t.z = q.z;
    }
  }
  S[i] = s;
  T[i] = t;
}

__device__ __forceinline__ uint32_t rsac_slot(const RsacPairs& P, uint32_t j) { return P.list ? P.list[j] : j; }

// ---- moments and threshold ------------------------------------------------------------------------------------------------
// computeMeanAndCovarianceMatrix (common/include/pcl/common/impl/centroid.hpp:581-650, the path that skips non-finite
// points) over the list's source points, shifted by the first one: thread g of the grid adds entries g, g + threads, ...
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_moments_kernel(RsacPairs P, double* __restrict__ partials) {
  double acc[RSAC_MOMENT_ROW];
#pragma unroll
  for (int i = 0; i < RSAC_MOMENT_ROW; ++i) acc[i] = 0.0;
  const uint32_t m = P.m_dev ? *P.m_dev : P.m_host;
  double kx = 0.0, ky = 0.0, kz = 0.0;
  if (m > 0u) {
    const float4 k4 = P.src[rsac_slot(P, 0u)];
    if (isfinite(k4.x) && isfinite(k4.y) && isfinite(k4.z)) {
      kx = double(k4.x); ky = double(k4.y); kz = double(k4.z);
    }
  }
  const uint32_t threads = gridDim.x * RSAC_BLOCK;
  for (uint32_t e = blockIdx.x * RSAC_BLOCK + threadIdx.x; e < m; e += threads) {
    const float4 p = P.src[rsac_slot(P, e)];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
    const double x = double(p.x) - kx, y = double(p.y) - ky, z = double(p.z) - kz;
    acc[0] += x * x; acc[1] += x * y; acc[2] += x * z;
    acc[3] += y * y; acc[4] += y * z; acc[5] += z * z;
    acc[6] += x; acc[7] += y; acc[8] += z;
    acc[9] += 1.0;
  }
  block_rows<RSAC_MOMENT_ROW, RSAC_WAVES, RSAC_MOMENT_ROW>(acc, partials);
}

// computeSampleDistanceThreshold (sac_model_registration.h:264-289) from the sums, and the start of the replay
__global__ void rejsac_threshold_kernel(const double* __restrict__ sums, RsacPairs P, double log_probability,
                                        RejSacState* __restrict__ st) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t m = P.m_dev ? *P.m_dev : P.m_host;
  double thresh = 0.0;  // sample_dist_thresh_ as constructed: what the reference keeps when no point is finite
  const double cnt = sums[9];
  if (cnt > 0.0) {
    double a[9];
    for (int i = 0; i < 9; ++i) a[i] = sums[i] / cnt;
    float cov[9];
    cov[0] = float(a[0] - a[6] * a[6]); cov[1] = float(a[1] - a[6] * a[7]); cov[2] = float(a[2] - a[6] * a[8]);
    cov[4] = float(a[3] - a[7] * a[7]); cov[5] = float(a[4] - a[7] * a[8]); cov[8] = float(a[5] - a[8] * a[8]);
    cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
    // pcl::eigen33(mat, evals) (common/include/pcl/common/impl/eigen.hpp): scaled by the largest entry
    float scale = 0.0f;
    for (int i = 0; i < 9; ++i) scale = fmaxf(scale, fabsf(cov[i]));
    if (scale <= FLT_MIN) scale = 1.0f;
    float sm[9], ev[3];
    for (int i = 0; i < 9; ++i) sm[i] = cov[i] / scale;
    compute_roots(sm, ev);
    const float r0 = sqrtf(ev[0] * scale), r1 = sqrtf(ev[1] * scale), r2 = sqrtf(ev[2] * scale);
    const double d = double(__fadd_rn(__fadd_rn(r0, r1), r2)) / 3.0;
    thresh = d * d;
  }
  st->sample_dist_thresh = thresh;
  st->log_probability = log_probability;
  st->one_over_n = 1.0 / double(m);
  st->k = DBL_MAX;
  st->n = m;
  st->best = 0u;
  st->best_trial = -1;
  st->iterations = 0;
  st->trials = 0u;
  st->done = m < 3u ? 1u : 0u;  // getSamples cannot select three points: no model
}

// ---- one batch ------------------------------------------------------------------------------------------------------------
// getSamples (sac_model.h:162-197) with isSampleGood (impl/sac_model_registration.hpp:48-66) and computeModelCoefficients
// (:69-97) for trial it0 + t.  info[trial] = attempts made, bit 31: none of them was good.
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_hypothesis_kernel(uint64_t seed, uint32_t it0, uint32_t nit, RsacPairs P,
                                                                       const RejSacState* __restrict__ st,
                                                                       float* __restrict__ Ts, uint32_t* __restrict__ info,
                                                                       pclhip_rejector_sac_trace* __restrict__ rec,
                                                                       uint32_t rec_cap) {
  if (st->done != 0u) return;
  const uint32_t t = blockIdx.x * RSAC_BLOCK + threadIdx.x;
  if (t >= nit) return;
  const uint32_t trial = it0 + t;
  const int n = int(st->n);
  const double thresh = st->sample_dist_thresh;
  int s[3] = {0, 0, 0};
  uint32_t slot[3] = {0u, 0u, 0u};
  float ps[3][3], pt[3][3];
  bool good = false;
  uint32_t attempts = 0u;
  while (attempts < RSAC_MAX_SAMPLE_CHECKS && !good) {
    int draws[3];
    for (int j = 0; j < 3; ++j) draws[j] = scp::draw_index_attempt(seed, trial, attempts, uint32_t(j), n - j);
    scp::insert_samples(draws, 3, s);
    for (int i = 0; i < 3; ++i) {
      slot[i] = rsac_slot(P, uint32_t(s[i]));
      const float4 q = P.src[slot[i]];
      ps[i][0] = q.x; ps[i][1] = q.y; ps[i][2] = q.z;
    }
    good = double(scp::edge_sq(ps[0], ps[1])) > thresh && double(scp::edge_sq(ps[0], ps[2])) > thresh &&
           double(scp::edge_sq(ps[1], ps[2])) > thresh;
    ++attempts;
  }
  float T[16];
  cf::zero16(T);
  if (good) {
    for (int i = 0; i < 3; ++i) {
      const float4 q = P.tgt[slot[i]];
      pt[i][0] = q.x; pt[i][1] = q.y; pt[i][2] = q.z;
    }
    scp_umeyama(ps, pt, 3, T);
  }
  for (int e = 0; e < 12; ++e) Ts[size_t(trial) * 12 + e] = T[e];
  info[trial] = attempts | (good ? 0u : 0x80000000u);
  if (rec != nullptr && trial < rec_cap) {
    pclhip_rejector_sac_trace& r = rec[trial];
    r.samples[0] = s[0]; r.samples[1] = s[1]; r.samples[2] = s[2];
    r.attempts = int(attempts);
    r.no_sample = good ? 0 : 1;
    for (int e = 0; e < 16; ++e) r.transformation[e] = T[e];
    r.count = 0u;
  }
}


// d2 of two pairs under the rows m0, m1, m2 of T: p = ((Tr0 s.x + Tr1 s.y) + Tr2 s.z) + Tr3, e = p - t,
// d2 = (e.x e.x + e.z e.z) + e.y e.y (-ffp-contract=off: no fused multiply-add)
__device__ __forceinline__ v2f rsac_d2_pair(const float4 m0, const float4 m1, const float4 m2, v2f sx, v2f sy,
                                                 v2f sz, v2f tx, v2f ty, v2f tz) {
  const v2f ex = (((v2f{m0.x, m0.x} * sx + v2f{m0.y, m0.y} * sy) + v2f{m0.z, m0.z} * sz) +
                       v2f{m0.w, m0.w}) - tx;
  const v2f ey = (((v2f{m1.x, m1.x} * sx + v2f{m1.y, m1.y} * sy) + v2f{m1.z, m1.z} * sz) +
                       v2f{m1.w, m1.w}) - ty;
  const v2f ez = (((v2f{m2.x, m2.x} * sx + v2f{m2.y, m2.y} * sy) + v2f{m2.z, m2.z} * sz) +
                       v2f{m2.w, m2.w}) - tz;
  return (ex * ex + ez * ez) + ey * ey;
}
// the same for one pair, with T in memory: what selects
__device__ __forceinline__ bool rsac_inlier(const float* __restrict__ T, const float4 s, const float4 t, float bound) {
  const float px = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], s.x), __fmul_rn(T[1], s.y)), __fmul_rn(T[2], s.z)), T[3]);
  const float py = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], s.x), __fmul_rn(T[5], s.y)), __fmul_rn(T[6], s.z)), T[7]);
  const float pz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], s.x), __fmul_rn(T[9], s.y)), __fmul_rn(T[10], s.z)), T[11]);
  const float ex = __fsub_rn(px, t.x), ey = __fsub_rn(py, t.y), ez = __fsub_rn(pz, t.z);
  const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ez, ez)), __fmul_rn(ey, ey));
  return d2 <= bound;
}

// countWithinDistance of H transforms at once (Ts: twelve floats each, 16-byte aligned).  counts[] is zero before the
// launch.  st == nullptr: an evaluation outside a run.
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_count_kernel(const float4* __restrict__ src, const float4* __restrict__ tgt,
                                                                  uint32_t n, const float4* __restrict__ Ts, uint32_t H,
                                                                  float bound, const RejSacState* __restrict__ st,
                                                                  uint32_t* __restrict__ counts) {
  if (st != nullptr && st->done != 0u) return;
  __shared__ uint32_t cnt_s[RSAC_MAX_BATCH];
  for (uint32_t h = threadIdx.x; h < H; h += RSAC_BLOCK) cnt_s[h] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint32_t tiles = (n + RSAC_TILE - 1) / RSAC_TILE;
  const float nan = __builtin_nanf("");
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // the wave's RSAC_P * 64 pairs: slot k of lane l is pair base + k * 64 + l (coalesced); past the end: NaN, never inside
    const uint32_t base = tile * uint32_t(RSAC_TILE) + wave * uint32_t(RSAC_P * WAVE) + lane;
    v2f sx[RSAC_P / 2], sy[RSAC_P / 2], sz[RSAC_P / 2], tx[RSAC_P / 2], ty[RSAC_P / 2], tz[RSAC_P / 2];
#pragma unroll
    for (int k = 0; k < RSAC_P / 2; ++k) {
      const uint32_t i0 = base + uint32_t(2 * k) * WAVE, i1 = i0 + WAVE;
      float4 a0 = make_float4(nan, nan, nan, 0.0f), a1 = a0, b0 = a0, b1 = a0;
      if (i0 < n) { a0 = src[i0]; b0 = tgt[i0]; }
      if (i1 < n) { a1 = src[i1]; b1 = tgt[i1]; }
      sx[k] = v2f{a0.x, a1.x}; sy[k] = v2f{a0.y, a1.y}; sz[k] = v2f{a0.z, a1.z};
      tx[k] = v2f{b0.x, b1.x}; ty[k] = v2f{b0.y, b1.y}; tz[k] = v2f{b0.z, b1.z};
    }
    for (uint32_t h0 = 0; h0 < H; h0 += WAVE) {
      const uint32_t hn = H - h0 < uint32_t(WAVE) ? H - h0 : uint32_t(WAVE);
      uint32_t mine = 0u;  // lane j: the wave's count of hypothesis h0 + j
      for (uint32_t j = 0; j < hn; ++j) {
        const float4* M = Ts + size_t(h0 + j) * 3;  // (the same for the wave: scalar loads)
        const float4 m0 = M[0], m1 = M[1], m2 = M[2];
        // a trial without a sample (zeros) is scored like any other: the replay never reads its count
        uint32_t cw = 0u;
#pragma unroll
        for (int k = 0; k < RSAC_P / 2; ++k) {
          const v2f d2 = rsac_d2_pair(m0, m1, m2, sx[k], sy[k], sz[k], tx[k], ty[k], tz[k]);
          cw += uint32_t(__popcll(__builtin_amdgcn_ballot_w64(d2.x <= bound)));
          cw += uint32_t(__popcll(__builtin_amdgcn_ballot_w64(d2.y <= bound)));
        }
        mine += lane == j ? cw : 0u;
      }
      if (mine != 0u) atomicAdd(&cnt_s[h0 + lane], mine);
    }
  }
  __syncthreads();
  for (uint32_t h = threadIdx.x; h < H; h += RSAC_BLOCK) {
    const uint32_t v = cnt_s[h];
    if (v != 0u) atomicAdd(&counts[h], v);
  }
}

// ransac.hpp:120-124,154-201 over the batch's trials in order
__global__ void rejsac_replay_kernel(RejSacState* __restrict__ st, const uint32_t* __restrict__ counts,
                                     const uint32_t* __restrict__ info, const float* __restrict__ Ts, uint32_t it0,
                                     uint32_t nit, int max_iterations) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || st->done != 0u) return;
  uint32_t best = st->best;
  int iterations = st->iterations;
  double k = st->k;
  for (uint32_t t = 0; t < nit; ++t) {
    const uint32_t trial = it0 + t;
    st->trials = trial + 1u;
    if (info[trial] >> 31) {  // "No samples could be selected"
      st->no_sample = 1u;
      st->done = 1u;
      break;
    }
    const uint32_t c = counts[trial];
    if (c > best) {
      best = c;
      st->best_trial = int32_t(trial);
      for (int e = 0; e < 12; ++e) st->T[e] = Ts[size_t(trial) * 12 + e];
      const double w = double(best) * st->one_over_n;
      double p_outliers = 1.0 - pow(w, 3.0);
      p_outliers = p_outliers > DBL_EPSILON ? p_outliers : DBL_EPSILON;
      p_outliers = p_outliers < 1.0 - DBL_EPSILON ? p_outliers : 1.0 - DBL_EPSILON;
      k = st->log_probability / log(p_outliers);
    }
    ++iterations;
    if (double(iterations) > k || iterations > max_iterations) {
      st->done = 1u;
      break;
    }
  }
  st->best = best;
  st->iterations = iterations;
  st->k = k;
}

// correspondence_rejection_sample_consensus.hpp:101-119: no model, or a winner with fewer than 3 inliers, leaves the list
// as it is and the transformation the identity.  The winner's count IS its selection: one expression counts and selects.
__global__ void rejsac_finish_kernel(RejSacState* __restrict__ st) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const bool model = st->best_trial >= 0 && st->best >= 3u;
  st->done = 1u;
  st->has_model = model ? 1u : 0u;
  st->remaining = model ? st->best : st->n;
  if (!model)
    for (int e = 0; e < 12; ++e) st->T[e] = (e % 5 == 0) ? 1.0f : 0.0f;
  st->T[12] = st->T[13] = st->T[14] = 0.0f;
  st->T[15] = 1.0f;
}

// ---- select ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_keep_kernel(const float4* __restrict__ src, const float4* __restrict__ tgt,
                                                                 uint32_t n, const RejSacState* __restrict__ st, float bound,
                                                                 uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * RSAC_BLOCK + threadIdx.x;
  if (i >= n || st->has_model == 0u) return;
  if (keep[i] && !rsac_inlier(st->T, src[i], tgt[i], bound)) keep[i] = 0;
}
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_flag_kernel(const float4* __restrict__ src, const float4* __restrict__ tgt,
                                                                 uint32_t n, const RejSacState* __restrict__ st, float bound,
                                                                 uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * RSAC_BLOCK + threadIdx.x;
  if (i >= n) return;
  flag[i] = st->has_model == 0u || rsac_inlier(st->T, src[i], tgt[i], bound) ? 1u : 0u;
}
__global__ __launch_bounds__(RSAC_BLOCK) void rejsac_positions_kernel(const uint32_t* __restrict__ flag,
                                                                      const uint32_t* __restrict__ excl, uint32_t n,
                                                                      int32_t* __restrict__ out, uint64_t capacity) {
  const uint32_t i = blockIdx.x * RSAC_BLOCK + threadIdx.x;
  if (i < n && flag[i] != 0u && uint64_t(excl[i]) < capacity) out[excl[i]] = int32_t(i);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// grid of the scoring pass: by occupancy, no more blocks than tiles
inline uint32_t rsac_count_grid(const pclhip_ctx* ctx, uint32_t n) {
  static int per_cu = 0;
  if (per_cu == 0) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, rejsac_count_kernel, RSAC_BLOCK, 0) != hipSuccess || v < 1) {
      (void)hipGetLastError();
      v = 4;
    }
    per_cu = v;
  }
  const uint64_t tiles = (uint64_t(n) + RSAC_TILE - 1) / RSAC_TILE;
  const uint64_t most = uint64_t(per_cu) * uint64_t(ctx->num_cus > 0 ? ctx->num_cus : 1);
  return uint32_t(tiles < most ? (tiles > 0 ? tiles : 1) : most);
}

// the buffers of a run besides the pairs
struct RsacWork {
  RejSacState* st = nullptr;   // the state block: the state, then one counter per trial (ONE memset)
  uint32_t* counts = nullptr;
  float* Ts = nullptr;         // [trials][12]
  uint32_t* info = nullptr;    // [trials]
  double* partials = nullptr;  // [RSAC_MOMENT_BLOCKS][RSAC_MOMENT_ROW]
  double* sums = nullptr;      // [RSAC_MOMENT_ROW]
  uint32_t trials = 0;         // max_iterations + 1
};

// A is anything with alloc(T**, bytes): rejectors.hip's Guard in the chain, a DeviceScope in the standalone call
template <class A>
pclhip_status rsac_alloc_work(pclhip_ctx* ctx, A& g, int max_iterations, RsacWork* w) {
  w->trials = uint32_t(max_iterations) + 1u;
  char* block = nullptr;
  const size_t head = (sizeof(RejSacState) + 15) / 16 * 16, bytes = head + size_t(w->trials) * 4;
  PCLHIP_CHECK_HIP(ctx, g.alloc(&block, bytes));
  w->st = reinterpret_cast<RejSacState*>(block);
  w->counts = reinterpret_cast<uint32_t*>(block + head);
  PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(block, 0, bytes, ctx->stream));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&w->Ts, size_t(w->trials) * 12 * sizeof(float)));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&w->info, size_t(w->trials) * 4));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&w->partials, size_t(RSAC_MOMENT_BLOCKS) * RSAC_MOMENT_ROW * sizeof(double)));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&w->sums, RSAC_MOMENT_ROW * sizeof(double)));
  return PCLHIP_OK;
}

// threshold, batches and finish of a run over the pairs P, queued on the context's stream
inline pclhip_status rsac_queue_run(pclhip_ctx* ctx, const RsacPairs& P, const RsacRun& R, const RsacWork& w, float bound,
                                    pclhip_rejector_sac_trace* rec, uint32_t rec_cap) {
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(rejsac_moments_kernel, dim3(RSAC_MOMENT_BLOCKS), dim3(RSAC_BLOCK), 0, s, P, w.partials);
  hipLaunchKernelGGL(block_sums_finalize_kernel<RSAC_MOMENT_ROW>, dim3(RSAC_MOMENT_ROW), dim3(WAVE), 0, s, w.partials,
                     RSAC_MOMENT_BLOCKS, w.sums);
  hipLaunchKernelGGL(rejsac_threshold_kernel, dim3(1), dim3(1), 0, s, w.sums, P, std::log(1.0 - R.probability), w.st);
  const uint32_t grid = rsac_count_grid(ctx, P.slots);
  for (const std::pair<uint32_t, uint32_t>& b : rsac_schedule(R.max_iterations, R.batch_size)) {
    const uint32_t it0 = b.first, nit = b.second;
    hipLaunchKernelGGL(rejsac_hypothesis_kernel, rsac_blocks_of(nit), dim3(RSAC_BLOCK), 0, s, R.seed, it0, nit, P, w.st, w.Ts,
                       w.info, rec, rec_cap);
    hipLaunchKernelGGL(rejsac_count_kernel, dim3(grid), dim3(RSAC_BLOCK), 0, s, P.src, P.tgt, P.slots,
                       reinterpret_cast<const float4*>(w.Ts) + size_t(it0) * 3, nit, bound, w.st, w.counts + it0);
    hipLaunchKernelGGL(rejsac_replay_kernel, dim3(1), dim3(1), 0, s, w.st, w.counts, w.info, w.Ts, it0, nit, R.max_iterations);
  }
  hipLaunchKernelGGL(rejsac_finish_kernel, dim3(1), dim3(1), 0, s, w.st);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  return PCLHIP_OK;
}

inline void rsac_stats_of(const RejSacState& h, pclhip_rejector_sac_stats* o) {
  std::memset(o, 0, sizeof *o);
  o->trials = h.trials;
  o->iterations = h.iterations;
  o->best_trial = h.best_trial;
  o->best_count = h.best;
  o->remaining = h.remaining;
  o->has_model = int(h.has_model);
  o->no_sample = int(h.no_sample);
  o->n = h.n;
  o->sample_dist_thresh = h.sample_dist_thresh;
}

inline pclhip_status rsac_checked_run(pclhip_ctx* ctx, const RsacRun& R) {
  PCLHIP_REQUIRE(ctx, R.max_iterations >= 0 && R.max_iterations <= RSAC_MAX_ITERATIONS,
                 "SampleConsensus rejector: max_iterations must lie in [0, 1000000]");
  PCLHIP_REQUIRE(ctx, R.threshold >= 0.0, "SampleConsensus rejector: the inlier threshold must be >= 0");
  PCLHIP_REQUIRE(ctx, R.probability > 0.0 && R.probability < 1.0, "SampleConsensus rejector: probability must lie in ]0, 1[");
  PCLHIP_REQUIRE(ctx, R.batch_size >= 0 && R.batch_size <= RSAC_MAX_BATCH, "SampleConsensus rejector: batch_size must lie in [0, 1024]");
  return PCLHIP_OK;
}

// the chain kind: the pairs still kept, in ascending original query index, over the moved source
template <class A>
pclhip_status rsac_apply_chain(pclhip_icp* icp, A& g, const pclhip_rejector& r) {
  pclhip_ctx* ctx = icp->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = icp->n, n_orig = uint32_t(icp->n_orig);
  RsacRun R;
  R.threshold = r.param;
  R.max_iterations = r.min_correspondences > uint32_t(RSAC_MAX_ITERATIONS) ? -1 : int(r.min_correspondences);
  R.probability = 0.99;
  R.seed = r.reserved;
  R.batch_size = 0;
  pclhip_status rc = rsac_checked_run(ctx, R);
  if (rc != PCLHIP_OK) return rc;
  // two slots with one original index: the scan below would count one pair and the scoring pass two, and with as many
  // indices as records an original index without a slot would leave by_orig unwritten
  PCLHIP_REQUIRE(ctx, !icp->src_repeats,
                 "SampleConsensus rejector: a source index is listed twice (the reference would silently keep the last pair)");
  if (!icp->rejsac_host) {
    PCLHIP_CHECK_HIP(ctx, pinned_malloc(ctx, &icp->rejsac_host, sizeof(RejSacState)));
    std::memset(icp->rejsac_host, 0, sizeof(RejSacState));
  }
  RsacWork w;
  if ((rc = rsac_alloc_work(ctx, g, R.max_iterations, &w)) != PCLHIP_OK) return rc;
  uint32_t *by_orig = nullptr, *excl = nullptr, *tot = nullptr, *list = nullptr;
  uint2* partial = nullptr;
  float4 *S = nullptr, *T = nullptr;
  PCLHIP_CHECK_HIP(ctx, g.alloc(&by_orig, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&excl, size_t(n_orig) * 4));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&partial, ((size_t(n_orig) + SC_BLOCK - 1) / SC_BLOCK) * sizeof(uint2)));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&tot, 4 * sizeof(uint32_t)));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&list, size_t(n) * 4));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&S, size_t(n) * sizeof(float4)));
  PCLHIP_CHECK_HIP(ctx, g.alloc(&T, size_t(n) * sizeof(float4)));
  // every original index has one slot unless the source is a subset of its cloud: only then are there gaps to clear
  if (uint64_t(n) != icp->n_orig) PCLHIP_CHECK_HIP(ctx, hipMemsetAsync(by_orig, 0, size_t(n_orig) * 4, s));
  hipLaunchKernelGGL(rejsac_scatter_keep_kernel, rsac_blocks_of(n), dim3(RSAC_BLOCK), 0, s, icp->src_cur, icp->keep, n, n_orig,
                     by_orig);
  launch_scan_u32(s, by_orig, n_orig, partial, tot, excl);
  hipLaunchKernelGGL(rejsac_gather_icp_kernel, rsac_blocks_of(n), dim3(RSAC_BLOCK), 0, s, icp->src_cur, icp->target->pts,
                     icp->match_pos, icp->keep, n, n_orig, excl, list, S, T);
  RsacPairs P;
  P.src = S;
  P.tgt = T;
  P.list = list;
  P.m_dev = tot;  // the scan's total: the pairs still kept
  P.m_host = 0;
  P.slots = n;
  const float bound = rsac_float_bound(R.threshold);
  if ((rc = rsac_queue_run(ctx, P, R, w, bound, nullptr, 0u)) != PCLHIP_OK) return rc;
  hipLaunchKernelGGL(rejsac_keep_kernel, rsac_blocks_of(n), dim3(RSAC_BLOCK), 0, s, S, T, n, w.st, bound, icp->keep);
  PCLHIP_CHECK_HIP(ctx, hipGetLastError());
  PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(icp->rejsac_host, w.st, sizeof(RejSacState), hipMemcpyDeviceToHost, s));
  icp->rejsac_ran = true;
  return PCLHIP_OK;
}

}  // namespace
}  // namespace pclhip
