// C++ host-side test of SampleConsensusModelCylinder and RandomSampleConsensus in the PCL-compatible mirror
// (include/pclhip/pcl_compat.hpp) on the 20 points and normals of the reference's cylinder test
// (test/sample_consensus/test_sample_consensus_quadric_models.cpp:400-497), with that test's own expectations.  Input: a text
// file of records x y z nx ny nz and what tests/sac_cylinder_restatement.py gives for the seeded call below, both from
// tests/test_gpu_sac_cylinder_cpp.py:  <file> <iterations> <sample 0> <sample 1>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pclhip/pcl_compat.hpp"

using namespace pclhip;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  int failures = 0;
  auto ctx = std::make_shared<Context>(0);
  if (!ctx->ok()) {
    std::fprintf(stderr, "no device: %s\n", ctx->getLastError().c_str());
    return 3;
  }
  auto cloud = std::make_shared<PointCloud<PointXYZ>>();
  auto normals = std::make_shared<PointCloud<Normal>>();
  if (std::FILE* f = std::fopen(argv[1], "r")) {
    float v[6];
    while (std::fscanf(f, "%f %f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
      cloud->push_back(PointXYZ(v[0], v[1], v[2]));
      Normal q;
      q.normal_x = v[3]; q.normal_y = v[4]; q.normal_z = v[5]; q.curvature = 0.0f;
      normals->push_back(q);
    }
    std::fclose(f);
  }
  EXPECT(cloud->size() == 20 && normals->size() == 20);
  auto model = std::make_shared<SampleConsensusModelCylinder<PointXYZ, Normal>>(cloud, ctx);
  EXPECT(model->getSampleSize() == 2 && model->getModelSize() == 7 && model->getNormalDistanceWeight() == 0.1);
  RandomSampleConsensus<PointXYZ> sac(model, 0.03);
  sac.setSeed(1);
  EXPECT(!sac.computeModel() && !model->getLastError().empty());  // no normals yet
  model->setInputNormals(normals);
  model->setNormalDistanceWeight(0.1);
  EXPECT(sac.computeModel() && model->getLastError().empty());
  EXPECT(sac.getLastStats().iterations == std::atoi(argv[2]));
  Indices sample, inliers;
  sac.getModel(sample);
  EXPECT(sample.size() == 2);
  if (sample.size() == 2) EXPECT(sample[0] == std::atoi(argv[3]) && sample[1] == std::atoi(argv[4]));
  sac.getInliers(inliers);
  EXPECT(inliers.size() == 20);
  VectorXf coeff, fine, again;
  sac.getModelCoefficients(coeff);
  EXPECT(coeff.size() == 7);
  if (coeff.size() == 7) {
    EXPECT(std::fabs(coeff[0] + 0.5f) < 1e-3f && std::fabs(coeff[1] - 1.7f) < 1e-3f && std::fabs(coeff[6] - 0.5f) < 1e-3f);
    if (sample.size() == 2) {
      EXPECT(model->computeModelCoefficients(sample, again) && again.size() == 7);
      for (std::size_t i = 0; i < again.size(); ++i) EXPECT(again[i] == coeff[i]);
    }
    model->optimizeModelCoefficients(inliers, coeff, fine);
    EXPECT(fine.size() == 7 && model->lastRefined() && model->lastIterations() > 0);
    EXPECT(std::fabs(fine[6] - 0.5f) < 1e-3f);
    std::vector<double> distances;
    model->getDistancesToModel(fine, distances);
    EXPECT(distances.size() == 20);
    if (distances.size() == 20) {
      EXPECT(std::fabs(distances[0] - 0.020) < 1e-3);
      for (std::size_t i = 1; i < 20; ++i) EXPECT(std::fabs(distances[i]) < 1e-3);
    }
    EXPECT(model->countWithinDistance(fine, 0.021) == 20 && model->countWithinDistance(fine, 0.019) == 19);
    model->selectWithinDistance(fine, 0.021, inliers);
    EXPECT(inliers.size() == 20);
    model->selectWithinDistance(fine, 0.019, inliers);
    EXPECT(inliers.size() == 19 && inliers[0] == 1);
    // the one call: the same coefficients and list as the three steps
    EXPECT(sac.segment(true) && sac.getLastStats().refined == 1);
    sac.getModelCoefficients(again);
    EXPECT(again.size() == 7);
    for (std::size_t i = 0; i < again.size() && i < fine.size(); ++i) EXPECT(again[i] == fine[i]);
    Indices rest;
    sac.getInliers(inliers);
    sac.getOutliers(rest);
    EXPECT(inliers.size() == 20 && rest.empty());
    // the gate: an axis across the cylinder leaves no valid hypothesis; radius limits away from 0.5 skip every sample
    model->setAxis(Vector3f(1.0f, 0.0f, 0.0f));
    model->setEpsAngle(0.1);
    sac.setMaxIterations(30);
    EXPECT(!sac.computeModel() && model->getLastError().empty() && sac.getLastStats().iterations == 31);
    EXPECT(model->countWithinDistance(fine, 0.021) == 0);
    model->getDistancesToModel(fine, distances);
    EXPECT(distances.empty());
    model->setAxis(Vector3f::Zero());
    EXPECT(!sac.computeModel() && !model->getLastError().empty());  // an angle without an axis
    model->setEpsAngle(0.0);
    model->setRadiusLimits(0.1, 0.2);
    sac.setMaxIterations(5);
    EXPECT(!sac.computeModel() && model->getLastError().empty() && sac.getLastStats().skipped == 50);
    model->setRadiusLimits(0.2, 0.1);
    EXPECT(!sac.computeModel() && !model->getLastError().empty());
    double lo = 0, hi = 0;
    model->getRadiusLimits(lo, hi);
    EXPECT(lo == 0.2 && hi == 0.1);
  }
  {  // a subset: the even points
    Indices even;
    for (index_t i = 0; i < 20; i += 2) even.push_back(i);
    auto part = std::make_shared<SampleConsensusModelCylinder<PointXYZ, Normal>>(cloud, even, ctx);
    part->setInputNormals(normals);
    RandomSampleConsensus<PointXYZ> sac2(part, 0.03);
    EXPECT(sac2.computeModel());
    sac2.getInliers(inliers);
    EXPECT(inliers.size() == 10);
    for (index_t i : inliers) EXPECT(i % 2 == 0);
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
