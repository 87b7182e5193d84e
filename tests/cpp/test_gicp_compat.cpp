// C++ host-side test of GeneralizedIterativeClosestPoint in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp):
// test/registration/test_registration.cpp:602-660 restated (bun0 -> bun4, 50 iterations, epsilon 1e-8, fitness < 1e-4;
// the four caching schemes of the search trees < 1e-3; the guess case asserted on reg_guess).  Inputs: bun0.txt bun4.txt
// written by the pytest wrapper (tests/test_gpu_gicp_cpp.py) from tests/golden/.
#include <cmath>
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
  GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ> reg(ctx);
  EXPECT(reg.getMaximumIterations() == 200 && reg.getCorrespondenceRandomness() == 20);
  reg.setInputSource(src);
  reg.setInputTarget(tgt);
  reg.setMaximumIterations(50);
  reg.setTransformationEpsilon(1e-8);
  reg.align(output);
  EXPECT(output.size() == src->size());
  const double fit0 = reg.getFitnessScore();
  EXPECT(fit0 < 1e-4);
  std::printf("fitness %.3g after %d iterations, %d Newton iterations\n", fit0, reg.getNumberOfIterations(),
              reg.lastResult().newton_iterations);
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
    EXPECT(reg.getFitnessScore() < 1e-3);
  }
  // the guess case: the target moved by AngleAxis(0.25 pi, X) * AngleAxis(0.5 pi, Y) * AngleAxis(0.33 pi, Z) + (0.1, 0.2, 0.3)
  const double a[3] = {0.25 * M_PI, 0.50 * M_PI, 0.33 * M_PI};
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int ax = 0; ax < 3; ++ax) {
    const double c = std::cos(a[ax]), s = std::sin(a[ax]);
    double B[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    const int i = ax == 0 ? 1 : 0, j = ax == 2 ? 1 : 2;
    B[i][i] = B[j][j] = c;
    B[i][j] = ax == 1 ? s : -s;
    B[j][i] = ax == 1 ? -s : s;
    double P[3][3];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) P[r][k] = R[r][0] * B[0][k] + R[r][1] * B[1][k] + R[r][2] * B[2][k];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) R[r][k] = P[r][k];
  }
  Matrix4f T = Matrix4f::Identity();
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) T(r, k) = float(R[r][k]);
  T(0, 3) = 0.1f;
  T(1, 3) = 0.2f;
  T(2, 3) = 0.3f;
  auto moved = std::make_shared<PointCloud<PointXYZ>>(*tgt);
  pclhip_transform_cloud(ctx->get(), T.m, 1, moved->points.data(), moved->points.data(), sizeof(PointXYZ), moved->size(), 0);
  GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ> reg_guess(ctx);
  reg_guess.setInputSource(src);
  reg_guess.setInputTarget(moved);
  reg_guess.setMaximumIterations(50);
  reg_guess.setTransformationEpsilon(1e-8);
  reg_guess.align(output, T);
  EXPECT(output.size() == src->size());
  EXPECT(reg_guess.getFitnessScore() < 1e-4);
  bool refused = false;
  try {
    reg.useBFGS();
  } catch (const std::logic_error&) {
    refused = true;
  }
  EXPECT(refused);
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
