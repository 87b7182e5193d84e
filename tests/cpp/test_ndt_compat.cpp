// C++ host-side test of NormalDistributionsTransform in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp):
// test/registration/test_ndt.cpp:53-97 restated (bun0 -> bun4, RADIUS neighbourhood, step size 0.05, resolution 0.025,
// 50 iterations, epsilon 1e-8, fitness < 0.001, again under the four caching schemes of the search trees).  Inputs:
// bun0.txt bun4.txt written by the pytest wrapper (tests/test_gpu_ndt_cpp.py) from tests/golden/.
#include <cstdio>
#include <fstream>

#include "pclhip/pcl_compat.hpp"

using namespace pclhip;

static PointCloud<PointXYZ>::Ptr load_xyz(const char* path) {
  auto c = std::make_shared<PointCloud<PointXYZ>>();
  std::ifstream f(path);
  float x, y, z;
  while (f >> x >> y >> z) c->push_back(PointXYZ(x, y, z));
  return c;
}

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  int failures = 0;
  auto ctx = std::make_shared<Context>(0);
  if (!ctx->ok()) {
    std::fprintf(stderr, "no device: %s\n", ctx->getLastError().c_str());
    return 3;
  }
  auto src = load_xyz(argv[1]);
  auto tgt = load_xyz(argv[2]);
  EXPECT(src->size() == 397 && tgt->size() == 361);
  PointCloud<PointXYZ> output;
  NormalDistributionsTransform<PointXYZ, PointXYZ> reg(ctx);
  EXPECT(reg.getResolution() == 1.0f && reg.getStepSize() == 0.1 && reg.getOutlierRatio() == 0.55);
  EXPECT(reg.getMaximumIterations() == 35 && reg.getTransformationEpsilon() == 0.1);
  reg.setNeighborhoodSearchMethod(NeighborSearchMethod::RADIUS);
  reg.setNumberOfThreads(1);
  reg.setStepSize(0.05);
  reg.setResolution(0.025f);
  reg.setInputSource(src);
  reg.setInputTarget(tgt);
  reg.setMaximumIterations(50);
  reg.setTransformationEpsilon(1e-8);
  reg.align(output);
  EXPECT(output.size() == src->size());
  EXPECT(reg.hasConverged());
  const double fit0 = reg.getFitnessScore();
  EXPECT(fit0 < 0.001);
  std::printf("fitness %.3g after %d iterations, %llu cells, likelihood %.3g\n", fit0, reg.getFinalNumIteration(),
              (unsigned long long)reg.lastResult().num_cells, reg.getTransformationLikelihood());
  EXPECT(reg.lastResult().num_cells == 32 && reg.lastResult().cells_ms > 0.0);
  for (int iter = 0; iter < 4; ++iter) {
    const bool force_cache = iter / 2 != 0, force_cache_reciprocal = iter % 2 != 0;
    auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
    if (force_cache) tree->setInputCloud(tgt);
    reg.setSearchMethodTarget(tree, force_cache);
    auto tree_recip = std::make_shared<search::KdTree<PointXYZ>>(ctx);
    if (force_cache_reciprocal) tree_recip->setInputCloud(src);
    reg.setSearchMethodSource(tree_recip, force_cache_reciprocal);
    reg.align(output);
    EXPECT(output.size() == src->size());
    EXPECT(reg.getFitnessScore() < 0.001);
    EXPECT(reg.lastResult().cells_ms == 0.0);  // the voxel Gaussians are kept
  }
  bool refused = false;
  try {
    reg.setNeighborhoodSearchMethod(NeighborSearchMethod::DIRECT7);
  } catch (const std::logic_error&) {
    refused = true;
  }
  EXPECT(refused);
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
