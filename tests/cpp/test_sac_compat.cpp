// C++ host-side test of SACSegmentation in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp) on the cloud of the
// reference's RANSAC plane test (test/sample_consensus/test_sample_consensus_plane_models.cpp:66-103,229-241): threshold
// 0.03, more than 2,000 inliers, coefficients / d within 0.1 of the expected plane; seed 1 gives 2,527 inliers in 8
// iterations (tests/test_sac_restatement.py pins them).  Input: the cloud as text, written by tests/test_gpu_sac_cpp.py.
#include <cmath>
#include <cstdio>
#include <fstream>

#include "pclhip/pcl_compat.hpp"

using namespace pclhip;

static PointCloud<PointXYZ>::Ptr load(const char* path) {
  auto c = std::make_shared<PointCloud<PointXYZ>>();
  std::ifstream f(path);
  float x, y, z;
  while (f >> x >> y >> z) {
    PointXYZ p;
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  int failures = 0;
  auto ctx = std::make_shared<Context>(0);
  if (!ctx->ok()) {
    std::fprintf(stderr, "no device: %s\n", ctx->getLastError().c_str());
    return 3;
  }
  auto cloud = load(argv[1]);
  EXPECT(cloud->size() == 3283);
  const double want[3] = {-0.8964, -0.5868, -1.208};
  {
    SACSegmentation<PointXYZ> seg(ctx);
    EXPECT(seg.getDistanceThreshold() == 0.0 && seg.getMaxIterations() == 50 && seg.getProbability() == 0.99 &&
           seg.getOptimizeCoefficients());
    PointIndices inliers;
    ModelCoefficients coeff;
    seg.setInputCloud(cloud);
    seg.segment(inliers, coeff);  // no model type yet
    EXPECT(inliers.indices.empty() && coeff.values.empty() && !seg.getLastError().empty());
    seg.setModelType(SACMODEL_PLANE);
    seg.setMethodType(SAC_RANSAC);
    seg.setDistanceThreshold(0.03);
    seg.setSeed(1);
    seg.setOptimizeCoefficients(false);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty());
    EXPECT(inliers.indices.size() == 2527 && seg.getLastStats().iterations == 8 && seg.getLastStats().skipped == 0);
    EXPECT(coeff.values.size() == 4);
    if (coeff.values.size() == 4)
      for (int i = 0; i < 3; ++i) EXPECT(std::fabs(double(coeff.values[i]) / double(coeff.values[3]) - want[i]) < 0.1);
    EXPECT(inliers.indices.size() + seg.getOutliers().size() == cloud->size());
    std::vector<int> seen(cloud->size(), 0);
    for (std::size_t j = 0; j < inliers.indices.size(); ++j) {
      if (j > 0) EXPECT(inliers.indices[j - 1] < inliers.indices[j]);  // ascending
      ++seen[std::size_t(inliers.indices[j])];
    }
    for (index_t i : seg.getOutliers()) ++seen[std::size_t(i)];
    for (int s : seen) EXPECT(s == 1);
    // the refit, and the selection with it
    const std::vector<float> first = coeff.values;
    seg.setOptimizeCoefficients(true);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastStats().refined == 1 && inliers.indices.size() > 2000 && coeff.values.size() == 4);
    if (coeff.values.size() == 4) {
      for (int i = 0; i < 2; ++i) EXPECT(std::fabs(double(coeff.values[i]) / double(coeff.values[3]) - want[i]) < 0.1);
      EXPECT(coeff.values != first);
    }
    seg.setMethodType(1);  // SAC_LMEDS
    seg.segment(inliers, coeff);
    EXPECT(inliers.indices.empty() && coeff.values.empty() && !seg.getLastError().empty());
  }
  {  // an index subset: the lists hold cloud indices, in the subset's order
    SACSegmentation<PointXYZ> seg(ctx);
    auto ind = std::make_shared<Indices>();
    for (index_t i = index_t(cloud->size()) - 1; i >= 0; i -= 3) ind->push_back(i);
    seg.setInputCloud(cloud);
    seg.setIndices(IndicesPtr(ind));
    seg.setModelType(SACMODEL_PLANE);
    seg.setMethodType(SAC_RANSAC);
    seg.setDistanceThreshold(0.03);
    PointIndices inliers;
    ModelCoefficients coeff;
    seg.segment(inliers, coeff);
    EXPECT(inliers.indices.size() > 600 && inliers.indices.size() + seg.getOutliers().size() == ind->size());
    for (std::size_t j = 0; j < inliers.indices.size(); ++j) {
      EXPECT((index_t(cloud->size()) - 1 - inliers.indices[j]) % 3 == 0);
      if (j > 0) EXPECT(inliers.indices[j - 1] > inliers.indices[j]);  // the subset descends
    }
  }
  {  // nothing but one point: no model, everything is left over
    auto flat = std::make_shared<PointCloud<PointXYZ>>();
    for (int i = 0; i < 100; ++i) flat->push_back((*cloud)[0]);
    SACSegmentation<PointXYZ> seg(ctx);
    seg.setInputCloud(flat);
    seg.setModelType(SACMODEL_PLANE);
    seg.setMethodType(SAC_RANSAC);
    seg.setDistanceThreshold(0.03);
    seg.setMaxIterations(5);
    PointIndices inliers;
    ModelCoefficients coeff;
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty() && inliers.indices.empty() && coeff.values.empty());
    EXPECT(seg.getOutliers().size() == 100 && seg.getLastStats().skipped == 50 && seg.getLastStats().best_trial == -1);
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
