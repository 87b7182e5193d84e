// scp_draw.hpp -- the random draws of SampleConsensusPrerejective, written once for the host, the device and the
// wavefront emulation (tests/scp_restatement.py restates them in numpy).
//
// The reference draws from rand() (sample_consensus_prerejective.h:250-253, n * (rand() / (RAND_MAX + 1.0))): a sequence
// no other libc reproduces and one that ties the result to the order of the iterations.  Here a draw is a pure function
// of (seed, iteration, slot): splitmix64's finalizer over a counter, u = (x >> 11) * 2^-53, index = int(n * u).
//   slots 0 .. nr_samples-1               the sample draws of selectSamples (draw j picks from n_src - j)
//   slots nr_samples .. 2 nr_samples-1    the pick among the k nearest features of sample j
// The result therefore does not depend on how iterations are batched, and a test can replay every draw.
// CorrespondenceRejectorSampleConsensus (rejector_sac.hpp) keys its draws by (seed, trial, attempt, slot): draw_index_attempt
// below; tests/rejector_sac_restatement.py restates it.
#pragma once

#include <stdint.h>

#include "closed_forms.hpp"  // PCLHIP_HD

namespace pclhip {
namespace scp {

constexpr int MAX_SAMPLES = 8;  // nr_samples of an alignment (the trace record holds that many)

PCLHIP_HD uint64_t draw_mix(uint64_t seed, uint64_t counter) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (counter + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

PCLHIP_HD uint64_t draw_bits(uint64_t seed, uint32_t iteration, uint32_t slot) {
  return draw_mix(seed, (uint64_t(iteration) << 8) | uint64_t(slot));
}

// CorrespondenceRejectorSampleConsensus redraws a bad sample INSIDE its trial (SampleConsensusModel::getSamples, sac_model.h:
// 162-197, up to 1,000 attempts): there a draw is a pure function of (seed, trial, attempt, slot), the same finalizer over
// the counter (trial << 24) | (attempt << 8) | slot (attempt < 65536, slot < 256).
PCLHIP_HD int draw_index_attempt(uint64_t seed, uint32_t trial, uint32_t attempt, uint32_t slot, int n) {
  const uint64_t x = draw_mix(seed, (uint64_t(trial) << 24) | (uint64_t(attempt) << 8) | uint64_t(slot));
  const double u = double(x >> 11) * (1.0 / 9007199254740992.0);
  return int(double(n) * u);
}

// getRandomIndex(n): an index in [0, n)
PCLHIP_HD int draw_index(uint64_t seed, uint32_t iteration, uint32_t slot, int n) {
  const double u = double(draw_bits(seed, iteration, slot) >> 11) * (1.0 / 9007199254740992.0);
  return int(double(n) * u);
}

// selectSamples (impl/sample_consensus_prerejective.hpp:96-117): draw j picks from n - j and is moved up past every
// earlier pick it reaches; the list comes out sorted and without duplicates.  draws[j] in [0, n - j).
PCLHIP_HD void insert_samples(const int* draws, int nr_samples, int* s) {
  for (int i = 0; i < nr_samples; ++i) {
    s[i] = draws[i];
    for (int j = 0; j < i; ++j) {
      if (s[i] >= s[j]) {
        s[i]++;
      } else {
        const int tmp = s[i];
        for (int k = i; k > j; --k) s[k] = s[k - 1];
        s[j] = tmp;
        break;
      }
    }
  }
}

PCLHIP_HD void select_samples(uint64_t seed, uint32_t iteration, int nr_samples, int n, int* s) {
  int draws[MAX_SAMPLES];
  for (int i = 0; i < nr_samples; ++i) draws[i] = draw_index(seed, iteration, uint32_t(i), n - i);
  insert_samples(draws, nr_samples, s);
}

// CorrespondenceRejectorPoly::thresholdEdgeLength (correspondence_rejection_poly.h:302-338): float squared lengths
// (dx*dx + dy*dy) + dz*dz, their ratio min / max in float, kept when >= simsq (0 / 0 is NaN: rejected)
PCLHIP_HD float edge_sq(const float* a, const float* b) {
  const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  return (dx * dx + dy * dy) + dz * dz;
}
PCLHIP_HD bool edge_similar(float dist_src, float dist_tgt, float simsq) {
  const float edge_sim = dist_src < dist_tgt ? dist_src / dist_tgt : dist_tgt / dist_src;
  return edge_sim >= simsq;
}

}  // namespace scp
}  // namespace pclhip
