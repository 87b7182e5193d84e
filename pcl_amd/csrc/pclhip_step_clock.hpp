// pclhip_step_clock.hpp -- the clock of the ICP step stamps (search.hip, icp_loop.hip include this by name through the
// include path).  The kernels of a step of the marker-free device-driven loop stamp their own times with the device's
// constant-rate counter; the host turns differences of stamps into milliseconds with the counter's rate, and asks the
// stream how it is doing while it waits for a step record.  The CPU emulation of the test tier provides a file of the same
// name in front of this one on ITS include path (tests/wavesim/pclhip_step_clock.hpp: std::chrono::steady_clock, a fixed
// rate, a stream that is always done) -- an include-path hook like <pclhip_wave_reduce.hpp>.
#pragma once

#if defined(PCLHIP_WAVESIM)
// an emulation build whose include path does not lead to its own file first (a copy of its Makefile built elsewhere)
#include "../../tests/wavesim/pclhip_step_clock.hpp"
#else

#include <hip/hip_runtime.h>

namespace pclhip {

// ticks of the constant-rate counter (100 MHz on gfx950): the same clock in every kernel of the device, whatever the
// shader clock does
__device__ __forceinline__ unsigned long long step_clock_now() { return wall_clock64(); }

// Publishes a step record that lies in host-coherent memory: everything this thread stored before is visible to the
// host before the sequence word is (a vector store with system scope; nothing else flushes for the ring).
__device__ __forceinline__ void step_record_publish(unsigned int* seq, unsigned int value) {
  __threadfence_system();
  __hip_atomic_store(seq, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the counter's rate in kHz = ticks per millisecond (read once per context: icp_loop.hip)
inline hipError_t step_clock_rate_khz(int device, int* khz) {
  return hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, device);
}

// hipSuccess: everything queued on the stream is done; hipErrorNotReady: not yet; anything else: the stream failed
inline hipError_t step_stream_query(hipStream_t s) { return hipStreamQuery(s); }

}  // namespace pclhip

#endif
