// block_sums.hpp -- the fixed-order double sums of GICP, NDT, the outlier statistics and the fitness score (included by
// search.hip and radius.hip).  No atomics: two runs give the same bits, and a pass that adds fewer columns gives, for its
// columns, the bits of the full pass.  The order, which the tests pin:
//   1. every thread adds its terms in a fixed order into its own accumulators
//   2. wave step: wave_sum_d (the xor butterfly, offsets 32, 16, ..., 1) over each accumulator; lane 0 writes the wave's
//      sum to LDS, red_s[wave][column]
//   3. block step: behind a barrier thread s adds column s over the block's waves in wave order, starting from 0.0, and
//      stores it to the block's row, partials[block * ROW + s]
//   4. block_sums_finalize_kernel: one wave per column, lane l adds rows l, l + 64, ..., then the wave's butterfly
// BlockSums is the host side of 3 and 4: the rows, the sums on the device and their pinned copy on the host.
#pragma once

#include <cstring>

#include "traverse.hpp"

namespace pclhip {

// wave step: accumulator i of the wave -> red_s[wave][i]
template <int N, int W>
__device__ __forceinline__ void wave_rows(const double (&acc)[N], double (*red_s)[W]) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double v = wave_sum_d(acc[i]);
    if (lane == 0) red_s[wave][i] = v;
  }
}

// block step, behind the barrier: column s over the block's waves in order
template <int NWAVES, int W>
__device__ __forceinline__ double block_column(const double (*red_s)[W], int s) {
  double a = 0.0;
#pragma unroll
  for (int w = 0; w < NWAVES; ++w) a += red_s[w][s];
  return a;
}

// block step: the barrier, then thread s < NS stores column s to the block's row
template <int NS, int NWAVES, int ROW, int W>
__device__ __forceinline__ void block_store(const double (*red_s)[W], double* __restrict__ partials) {
  __syncthreads();
  if (threadIdx.x < NS) partials[size_t(blockIdx.x) * ROW + threadIdx.x] = block_column<NWAVES>(red_s, threadIdx.x);
}

// both steps: one row of NS block sums per block
template <int NS, int NWAVES, int ROW>
__device__ __forceinline__ void block_rows(const double (&acc)[NS], double* __restrict__ partials) {
  __shared__ double red_s[NWAVES][NS];
  wave_rows(acc, red_s);
  block_store<NS, NWAVES, ROW>(red_s, partials);
}

// the block rows summed in a fixed order: grid = the number of sums, one wave per sum, lane l adds rows l, l + 64, ...
// (coalesced across the sums' waves), then the wave's tree
template <int ROW>
__global__ __launch_bounds__(WAVE) void block_sums_finalize_kernel(const double* __restrict__ partials, int blocks,
                                                                   double* __restrict__ out) {
  const int s = blockIdx.x, lane = threadIdx.x;
  double a = 0.0;
  for (int b = lane; b < blocks; b += WAVE) a += partials[size_t(b) * ROW + s];
  a = wave_sum_d(a);
  if (lane == 0) out[s] = a;
}

template <int ROW>
struct BlockSums {
  double* partials = nullptr;  // [blocks * ROW]
  double* dev = nullptr;       // [ROW]
  double* host = nullptr;      // pinned [ROW]
  int blocks = 0;

  hipError_t create(pclhip_ctx* ctx) {
    const hipError_t e = dev_malloc(ctx, &dev, ROW * sizeof(double));
    return e != hipSuccess ? e : pinned_malloc(ctx, &host, ROW * sizeof(double));
  }
  hipError_t resize(pclhip_ctx* ctx, int nblocks) {
    dev_free_if(ctx, partials);
    partials = nullptr;
    blocks = nblocks;
    return dev_malloc(ctx, &partials, size_t(nblocks) * ROW * sizeof(double));
  }
  void release(pclhip_ctx* ctx) {
    dev_free_if(ctx, partials);
    dev_free_if(ctx, dev);
    if (host) pinned_free(ctx, host, ROW * sizeof(double));
    partials = dev = host = nullptr;
  }
  // the first ns sums of the rows a pass has just written, on the host; `after` is recorded behind the finalize
  pclhip_status read(pclhip_ctx* ctx, int ns, double* out, hipEvent_t after) {
    hipLaunchKernelGGL(block_sums_finalize_kernel<ROW>, dim3(ns), dim3(WAVE), 0, ctx->stream, partials, blocks, dev);
    PCLHIP_CHECK_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(after, ctx->stream);
    PCLHIP_CHECK_HIP(ctx, hipMemcpyAsync(host, dev, size_t(ns) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCLHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out, host, size_t(ns) * sizeof(double));
    return PCLHIP_OK;
  }
};

}  // namespace pclhip
