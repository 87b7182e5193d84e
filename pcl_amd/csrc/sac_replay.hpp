// sac_replay.hpp -- the sequential part of RandomSampleConsensus::computeModel (sample_consensus/include/pcl/
// sample_consensus/impl/ransac.hpp:66-202), written once for the host side of the library and of the wavefront emulation
// (tests/sac_restatement.py restates it in Python).  The device scores a batch of trials; their counts and skip flags are
// fed here in trial order, so the stopping rule's log and pow are the host libm's, as in the reference.
#pragma once

#include <cfloat>
#include <cmath>
#include <stdint.h>

namespace pclhip {
namespace sac {

struct Replay {
  int max_iterations = 50;
  double log_probability = 0.0;   // log(1 - probability)
  double one_over_n = 0.0;
  int sample_size = 3;            // the model's: the exponent of the stopping rule (2 for the cylinder)
  int iterations = 0;
  uint32_t skipped = 0;
  uint32_t best = 0;
  double k = DBL_MAX;
  int64_t best_trial = -1;
  uint64_t trials = 0;            // trials fed so far
  bool done = false;

  void start(int max_it, double probability, uint64_t n, int samples = 3) {
    *this = Replay();
    sample_size = samples;
    max_iterations = max_it;
    log_probability = std::log(1.0 - probability);
    one_over_n = 1.0 / double(n);
  }
  // one trial, in order; false once the loop has ended (this trial was the last one consumed)
  bool feed(bool skip, uint32_t count) {
    const int64_t trial = int64_t(trials++);
    if (skip) {  // :127-139
      ++skipped;
      if (uint64_t(skipped) < uint64_t(max_iterations) * 10u) return true;
      done = true;
      return false;
    }
    if (count > best) {  // :154-176
      best = count;
      best_trial = trial;
      const double w = double(best) * one_over_n;
      double p_outliers = 1.0 - std::pow(w, double(sample_size));
      p_outliers = p_outliers > DBL_EPSILON ? p_outliers : DBL_EPSILON;
      p_outliers = p_outliers < 1.0 - DBL_EPSILON ? p_outliers : 1.0 - DBL_EPSILON;
      k = log_probability / std::log(p_outliers);
    }
    ++iterations;  // :185-201
    if (double(iterations) > k || iterations > max_iterations) {
      done = true;
      return false;
    }
    return true;
  }
};

}  // namespace sac
}  // namespace pclhip
