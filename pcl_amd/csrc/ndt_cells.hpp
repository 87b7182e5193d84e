// ndt_cells.hpp -- the voxel Gaussians of NormalDistributionsTransform's target: VoxelGridCovariance::applyFilter
// (filters/include/pcl/filters/impl/voxel_grid_covariance.hpp:47-367).  Included by voxelgrid.hip: grid, voxel ids, the
// stable sort by voxel id and the runs are VoxelGrid's own (voxelgrid_run); this file is the stage behind them.
//
//   ndt_cell_kernel   one thread per kept run (a voxel with >= min_points_per_voxel points), walking the run in sorted =
//                     ascending input order: the float centroid sum and the double sums of p and p p^T are SEQUENTIAL
//                     sums in input order, bit for bit what the reference's leaf accumulates (:230-239), whatever the
//                     launch shape.  Then mean, covariance, eigen-decomposition, inflation and inverse
//                     (nf::cell_from_sums).  Cost: the longest run serialises its thread (one gather per point, no
//                     coalescing) -- the pass is one-off per target and resolution and is reported as cells_ms.
//                     The 3x3 Jacobi sweeps index their matrices at run time: they live in scratch memory (one thread per
//                     voxel, once).
#pragma once

#include "ndt_forms.hpp"

namespace pclhip {
namespace {

__global__ __launch_bounds__(256) void ndt_cell_kernel(const void* pts, size_t stride, const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ keys_sorted,
                                                       const uint32_t* __restrict__ run_start,
                                                       const uint32_t* __restrict__ keep,
                                                       const uint32_t* __restrict__ keep_scan, uint32_t nruns, double mult,
                                                       float4* __restrict__ centroid, double* __restrict__ rec_out,
                                                       double* __restrict__ cov_out, int32_t* __restrict__ npoints,
                                                       int32_t* __restrict__ voxel, uint8_t* __restrict__ valid) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nruns || !keep[r]) return;
  const uint32_t b = run_start[r], e = run_start[r + 1];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  double ps[3] = {0.0, 0.0, 0.0};
  double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
  for (uint32_t j = b; j < e; ++j) {
    const float* p = rec(pts, stride, vals[j]);
    const float x = p[0], y = p[1], z = p[2];
    sx = __fadd_rn(sx, x);
    sy = __fadd_rn(sy, y);
    sz = __fadd_rn(sz, z);
    const double dx = double(x), dy = double(y), dz = double(z);
    ps[0] += dx;
    ps[1] += dy;
    ps[2] += dz;
    c00 += dx * dx;
    c01 += dx * dy;
    c02 += dx * dz;
    c11 += dy * dy;
    c12 += dy * dz;
    c22 += dz * dz;
  }
  const uint32_t n = e - b;
  const uint32_t c = keep_scan[r];
  const float cnt = float(n);
  centroid[c] = make_float4(__fdiv_rn(sx, cnt), __fdiv_rn(sy, cnt), __fdiv_rn(sz, cnt), __uint_as_float(c));
  const double cs[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
  double mean[3], cov[9], icov[6];
  const bool ok = nf::cell_from_sums(n, ps, cs, mult, mean, cov, icov);
  double* o = rec_out + size_t(c) * nf::kNdtCellDoubles;
  for (int k = 0; k < 3; ++k) o[k] = mean[k];
  for (int k = 0; k < 6; ++k) o[3 + k] = icov[k];
  for (int k = 0; k < 9; ++k) cov_out[size_t(c) * 9 + k] = cov[k];
  npoints[c] = int32_t(n);
  voxel[c] = int32_t(keys_sorted[b]);
  valid[c] = ok ? 1 : 0;
}

// the stage behind VoxelGrid's runs: `total` kept runs -> cells
pclhip_status ndt_cells_from_runs(pclhip_ctx* ctx, const void* dp, size_t stride, const uint32_t* vals_sorted,
                                  const uint32_t* keys_sorted, const uint32_t* run_start, const uint32_t* keep,
                                  const uint32_t* keep_scan, uint32_t nruns, uint32_t total, double mult, NdtCells* cells) {
  ndt_free_cells(ctx, cells);
  if (total == 0) return PCLHIP_OK;
  const size_t m = total;
  if (dev_malloc(ctx, &cells->centroid, m * sizeof(float4)) != hipSuccess ||
      dev_malloc(ctx, &cells->rec, m * nf::kNdtCellDoubles * sizeof(double)) != hipSuccess ||
      dev_malloc(ctx, &cells->cov, m * 9 * sizeof(double)) != hipSuccess ||
      dev_malloc(ctx, &cells->npoints, m * sizeof(int32_t)) != hipSuccess ||
      dev_malloc(ctx, &cells->voxel, m * sizeof(int32_t)) != hipSuccess ||
      dev_malloc(ctx, &cells->valid, m) != hipSuccess) {
    ndt_free_cells(ctx, cells);
    set_error(ctx, "allocation failed for the voxel Gaussians");
    return PCLHIP_ERR_HIP;
  }
  hipLaunchKernelGGL(ndt_cell_kernel, dim3((nruns + 255) / 256), dim3(256), 0, ctx->stream, dp, stride, vals_sorted, keys_sorted,
                     run_start, keep, keep_scan, nruns, mult, cells->centroid, cells->rec, cells->cov, cells->npoints,
                     cells->voxel, cells->valid);
  const hipError_t e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess || es != hipSuccess) {
    ndt_free_cells(ctx, cells);
    PCLHIP_CHECK_HIP(ctx, e);
    PCLHIP_CHECK_HIP(ctx, es);
  }
  cells->count = total;
  return PCLHIP_OK;
}

}  // namespace

void ndt_free_cells(pclhip_ctx* ctx, NdtCells* cells) {
  void* p[6] = {cells->centroid, cells->rec, cells->cov, cells->npoints, cells->voxel, cells->valid};
  for (void* q : p)
    if (q) dev_free(ctx, q);
  *cells = NdtCells();
}

}  // namespace pclhip
