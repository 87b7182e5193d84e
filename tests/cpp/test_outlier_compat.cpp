// C++ host-side test of StatisticalOutlierRemoval / RadiusOutlierRemoval in the PCL-compatible mirror
// (include/pclhip/pcl_compat.hpp): test/filters/test_filters.cpp:1494-1700 restated on bun0 (PointXYZ), plus the same
// filters on 48-byte PointNormal records.  Input: bun0.txt written by the pytest wrapper (tests/test_gpu_outlier_cpp.py).
#include <cmath>
#include <cstdio>
#include <fstream>

#include "pclhip/pcl_compat.hpp"

using namespace pclhip;

template <typename PointT>
static typename PointCloud<PointT>::Ptr load(const char* path) {
  auto c = std::make_shared<PointCloud<PointT>>();
  std::ifstream f(path);
  float x, y, z;
  while (f >> x >> y >> z) {
    PointT p;
    p.x = x;
    p.y = y;
    p.z = z;
    c->push_back(p);
  }
  return c;
}

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)
#define NEAR(a, b) EXPECT(std::fabs(double(a) - double(b)) < 1e-4)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  int failures = 0;
  auto ctx = std::make_shared<Context>(0);
  if (!ctx->ok()) {
    std::fprintf(stderr, "no device: %s\n", ctx->getLastError().c_str());
    return 3;
  }
  auto cloud = load<PointXYZ>(argv[1]);
  EXPECT(cloud->size() == 397);
  {
    PointCloud<PointXYZ> output;
    StatisticalOutlierRemoval<PointXYZ> outrem(ctx, true);
    outrem.setInputCloud(cloud);
    outrem.setMeanK(50);
    outrem.setStddevMulThresh(1.0);
    outrem.filter(output);
    EXPECT(output.size() == 352 && output.width == 352 && output.height == 1 && output.is_dense);
    EXPECT(output.size() == cloud->size() - outrem.getRemovedIndices()->size());
    NEAR(output[output.size() - 1].x, -0.034667);
    NEAR(output[output.size() - 1].y, 0.15131);
    NEAR(output[output.size() - 1].z, -0.00071029);
    outrem.setNegative(true);
    outrem.filter(output);
    EXPECT(output.size() == cloud->size() - 352 && output.width == cloud->width - 352 && output.is_dense);
    NEAR(output[output.size() - 1].x, -0.07793);
    NEAR(output[output.size() - 1].y, 0.17516);
    NEAR(output[output.size() - 1].z, -0.0444);
    Indices idx;
    outrem.setNegative(false);
    outrem.filter(idx);
    EXPECT(idx.size() == 352 && outrem.getRemovedIndices()->size() == 45);
    // keep organized: the input's size, removed points at the user value, not dense with NaN
    outrem.setKeepOrganized(true);
    outrem.filter(output);
    EXPECT(output.size() == cloud->size() && !output.is_dense);
    EXPECT(std::isnan(output[std::size_t((*outrem.getRemovedIndices())[0])].x));
  }
  {
    PointCloud<PointXYZ> output;
    RadiusOutlierRemoval<PointXYZ> outrem(ctx, true);
    outrem.setInputCloud(cloud);
    outrem.setRadiusSearch(0.02);
    outrem.setMinNeighborsInRadius(14);
    outrem.setNumberOfThreads(4);
    outrem.filter(output);
    EXPECT(output.size() == 307 && output.width == 307 && output.is_dense);
    EXPECT(output.size() == cloud->size() - outrem.getRemovedIndices()->size());
    NEAR(output[output.size() - 1].x, -0.077893);
    NEAR(output[output.size() - 1].y, 0.16039);
    NEAR(output[output.size() - 1].z, -0.021299);
    outrem.setNegative(true);
    outrem.filter(output);
    EXPECT(output.size() == 90 && output.is_dense);
  }
  {
    auto pn = load<PointNormal>(argv[1]);
    PointCloud<PointNormal> output;
    StatisticalOutlierRemoval<PointNormal> sor(ctx, false);
    sor.setInputCloud(pn);
    sor.setMeanK(50);
    sor.setStddevMulThresh(1.0);
    sor.filter(output);
    EXPECT(output.size() == 352);
    EXPECT(sor.getRemovedIndices()->empty());  // not extracted
    RadiusOutlierRemoval<PointNormal> ror(ctx, false);
    ror.setInputCloud(pn);
    ror.setRadiusSearch(0.02);
    ror.setMinNeighborsInRadius(14);
    ror.filter(output);
    EXPECT(output.size() == 307);
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
