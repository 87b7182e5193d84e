// C++ host-side test of SampleConsensusPrerejective in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp): the object
// path of test/registration/test_sac_ia.cpp:140-209 -- bun0 moved by (100, 0, 0) and 90 degrees about z against bun4,
// correspondence distance 0.1, 5,000 iterations, similarity 0.6, randomness 2, more than 95 % inliers -- with the project's
// normals (k = 10) and FPFH (r = 0.05), and the error returns of :161-212.  Input: source.txt and target.txt (x y z per
// line), written by the pytest wrapper (tests/test_gpu_scp_cpp.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "pclhip/pcl_compat.hpp"

using namespace pclhip;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

static std::shared_ptr<PointCloud<PointXYZ>> load(const char* path) {
  auto cloud = std::make_shared<PointCloud<PointXYZ>>();
  std::ifstream f(path);
  float x, y, z;
  while (f >> x >> y >> z) cloud->push_back(PointXYZ(x, y, z));
  return cloud;
}

static std::shared_ptr<PointCloud<FPFHSignature33>> features(const Context::Ptr& ctx, const std::shared_ptr<PointCloud<PointXYZ>>& cloud) {
  auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
  auto normals = std::make_shared<PointCloud<Normal>>();
  NormalEstimation<PointXYZ> ne(ctx);
  ne.setInputCloud(cloud);
  ne.setSearchMethod(tree);
  ne.setKSearch(10);
  ne.compute(*normals);
  auto out = std::make_shared<PointCloud<FPFHSignature33>>();
  FPFHEstimation<PointXYZ, Normal, FPFHSignature33> fpfh(ctx);
  fpfh.setInputCloud(cloud);
  fpfh.setInputNormals(normals);
  fpfh.setSearchMethod(tree);
  fpfh.setRadiusSearch(0.05);
  fpfh.compute(*out);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  int failures = 0;
  auto ctx = std::make_shared<Context>(0);
  if (!ctx->ok()) {
    std::fprintf(stderr, "no device: %s\n", ctx->getLastError().c_str());
    return 3;
  }
  auto source = load(argv[1]), target = load(argv[2]);
  EXPECT(source->size() == 397 && target->size() == 361);
  auto fs = features(ctx, source), ft = features(ctx, target);
  EXPECT(fs->size() == source->size() && ft->size() == target->size());
  using Scp = SampleConsensusPrerejective<PointXYZ, PointXYZ, FPFHSignature33>;
  for (std::uint64_t seed = 1; seed <= 3; ++seed) {
    Scp reg(ctx);
    EXPECT(reg.getNumberOfSamples() == 3 && reg.getCorrespondenceRandomness() == 2 && reg.getMaximumIterations() == 5000);
    EXPECT(reg.getSimilarityThreshold() == 0.6f && reg.getInlierFraction() == 0.0f);
    reg.setMaxCorrespondenceDistance(0.1);
    reg.setMaximumIterations(5000);
    reg.setSimilarityThreshold(0.6f);
    reg.setCorrespondenceRandomness(2);
    reg.setSeed(seed);
    reg.setInputSource(source);
    reg.setInputTarget(target);
    reg.setSourceFeatures(fs);
    reg.setTargetFeatures(ft);
    EXPECT(reg.getSourceFeatures() == fs && reg.getTargetFeatures() == ft);
    PointCloud<PointXYZ> out;
    reg.align(out);
    EXPECT(reg.hasConverged());
    EXPECT(out.size() == source->size());
    const float fraction = float(reg.getInliers().size()) / float(source->size());
    EXPECT(fraction > 0.95f);
    EXPECT(reg.lastResult().best_count == reg.getInliers().size());
    for (std::size_t i = 1; i < reg.getInliers().size(); ++i) EXPECT(reg.getInliers()[i - 1] < reg.getInliers()[i]);
    // every point is an inlier here: getFitnessScore (the mean over all points) is the accepted error
    if (reg.getInliers().size() == source->size())
      EXPECT(std::fabs(reg.getFitnessScore() - double(reg.lastResult().best_error)) <= 1e-5 * double(reg.lastResult().best_error));
    std::printf("seed %llu: %zu inliers, error %g, %d of %d rejected\n", (unsigned long long)seed, reg.getInliers().size(),
                double(reg.lastResult().best_error), reg.lastResult().rejected, reg.lastResult().iterations);
  }
  {  // the error returns: converged_ stays false, the final transformation is the guess
    Scp reg(ctx);
    reg.setMaxCorrespondenceDistance(0.1);
    reg.setMaximumIterations(10);
    reg.setInputSource(source);
    reg.setInputTarget(target);
    PointCloud<PointXYZ> out;
    reg.align(out);  // no features
    EXPECT(!reg.hasConverged() && reg.lastStatus() == PCLHIP_ERR_STATE);
    reg.setSourceFeatures(fs);
    reg.setTargetFeatures(fs);  // 397 rows for 361 target points
    reg.align(out);
    EXPECT(!reg.hasConverged() && reg.lastStatus() == PCLHIP_ERR_STATE);
    reg.setTargetFeatures(ft);
    reg.setInlierFraction(1.5f);
    reg.align(out);
    EXPECT(!reg.hasConverged() && reg.lastStatus() == PCLHIP_ERR_INVALID);
    reg.setInlierFraction(0.0f);
    reg.setSimilarityThreshold(1.0f);
    reg.align(out);
    EXPECT(!reg.hasConverged() && reg.lastStatus() == PCLHIP_ERR_INVALID);
    reg.setSimilarityThreshold(0.6f);
    reg.setCorrespondenceRandomness(0);
    reg.align(out);
    EXPECT(!reg.hasConverged() && reg.lastStatus() == PCLHIP_ERR_INVALID && reg.getInliers().empty());
    reg.setCorrespondenceRandomness(2);
    reg.setNumberOfSamples(8);
    reg.setInlierFraction(1.0f);  // nothing reaches it: not converged, no error
    reg.align(out);
    EXPECT(!reg.hasConverged() && reg.lastStatus() == PCLHIP_OK && reg.getInliers().empty());
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
