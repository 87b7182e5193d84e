// pclhip_step_clock.hpp -- the clock of the ICP step stamps (search.hip and icp_loop.hip include this by name through the
// include path).  THIS file: TEST INFRASTRUCTURE -- the host form for the emulation (tests/wavesim): the stamps are
// nanoseconds of std::chrono::steady_clock, the rate is fixed, and a stream is done whenever it is asked (launches are
// synchronous here).  The Makefile here puts this directory in front of pcl_amd/csrc on the include path.
#pragma once

#include <chrono>

namespace pclhip {

__device__ __forceinline__ unsigned long long step_clock_now() {
  return static_cast<unsigned long long>(
      std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count());
}

__device__ __forceinline__ void step_record_publish(unsigned int* seq, unsigned int value) {
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  __atomic_store_n(seq, value, __ATOMIC_RELEASE);
}

inline hipError_t step_clock_rate_khz(int, int* khz) {
  *khz = 1000000;  // nanoseconds: 1e6 ticks per millisecond
  return hipSuccess;
}

inline hipError_t step_stream_query(hipStream_t) { return hipSuccess; }

}  // namespace pclhip
