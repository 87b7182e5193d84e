// C++ host-side test of the constrained planes of SACSegmentation and of SACSegmentationFromNormals in the PCL-compatible
// mirror (include/pclhip/pcl_compat.hpp) on the cloud and the normals of the reference's plane tests
// (test/sample_consensus/test_sample_consensus_plane_models.cpp:66-103,319-397).  Input: a text file of records
// x y z nx ny nz curvature and the counts tests/sac_models_restatement.py gives for the two seeded calls below, both from
// tests/test_gpu_sac_models_cpp.py:  <file> <normal-plane inliers> <its iterations> <perpendicular inliers> <its iterations>
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
  if (argc < 6) return 2;
  int failures = 0;
  auto ctx = std::make_shared<Context>(0);
  if (!ctx->ok()) {
    std::fprintf(stderr, "no device: %s\n", ctx->getLastError().c_str());
    return 3;
  }
  auto cloud = std::make_shared<PointCloud<PointXYZ>>();
  auto normals = std::make_shared<PointCloud<Normal>>();
  if (std::FILE* f = std::fopen(argv[1], "r")) {
    float v[7];
    while (std::fscanf(f, "%f %f %f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7) {  // (reads "nan")
      cloud->push_back(PointXYZ(v[0], v[1], v[2]));
      Normal q;
      q.normal_x = v[3]; q.normal_y = v[4]; q.normal_z = v[5]; q.curvature = v[6];
      normals->push_back(q);
    }
    std::fclose(f);
  }
  EXPECT(cloud->size() == 3283 && normals->size() == 3283);
  const std::size_t want_normal = std::size_t(std::atol(argv[2])), want_perp = std::size_t(std::atol(argv[4]));
  const int it_normal = std::atoi(argv[3]), it_perp = std::atoi(argv[5]);
  const double want[3] = {-0.8964, -0.5868, -1.208};
  const Vector3f floor_axis(-0.8964f, -0.5868f, -1.208f), along(0.5477f, -0.8367f, 0.0f);  // (unit length: the gates take the axis as given)
  PointIndices inliers;
  ModelCoefficients coeff;
  {  // SACMODEL_NORMAL_PLANE as the reference tests it: weight 0.01, threshold 0.03
    SACSegmentationFromNormals<PointXYZ, Normal> seg(ctx);
    EXPECT(seg.getNormalDistanceWeight() == 0.1 && seg.getDistanceFromOrigin() == 0.0 && seg.getEpsAngle() == 0.0);
    seg.setInputCloud(cloud);
    seg.setModelType(SACMODEL_NORMAL_PLANE);
    seg.setMethodType(SAC_RANSAC);
    seg.setDistanceThreshold(0.03);
    seg.setNormalDistanceWeight(0.01);
    seg.setSeed(1);
    seg.setOptimizeCoefficients(false);
    seg.segment(inliers, coeff);  // no normals yet
    EXPECT(inliers.indices.empty() && coeff.values.empty() && !seg.getLastError().empty());
    seg.setInputNormals(normals);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty());
    EXPECT(inliers.indices.size() == want_normal && want_normal > 2000 && seg.getLastStats().iterations == it_normal);
    EXPECT(coeff.values.size() == 4);
    if (coeff.values.size() == 4)
      for (int i = 0; i < 3; ++i) EXPECT(std::fabs(double(coeff.values[i]) / double(coeff.values[3]) - want[i]) < 0.1);
    EXPECT(inliers.indices.size() + seg.getOutliers().size() == cloud->size());
    for (index_t i : inliers.indices) EXPECT(!std::isnan((*normals)[std::size_t(i)].curvature));  // a NaN record: never inside
    seg.setOptimizeCoefficients(true);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastStats().refined == 1 && inliers.indices.size() > 2000 && coeff.values.size() == 4);
    if (coeff.values.size() == 4)
      for (int i = 0; i < 3; ++i) EXPECT(std::fabs(double(coeff.values[i]) / double(coeff.values[3]) - want[i]) < 0.1);
    // SACMODEL_NORMAL_PARALLEL_PLANE: the floor's normal as the axis keeps it, a direction inside the floor leaves nothing
    seg.setModelType(SACMODEL_NORMAL_PARALLEL_PLANE);
    seg.setAxis(floor_axis);
    seg.setEpsAngle(0.1);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty() && inliers.indices.size() > 2000);
    seg.setAxis(along);
    seg.setEpsAngle(0.02);
    seg.setMaxIterations(40);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty() && inliers.indices.empty() && coeff.values.empty());
    EXPECT(seg.getLastStats().iterations == 41 && seg.getLastStats().skipped == 0 && seg.getOutliers().size() == cloud->size());
    seg.setAxis(Vector3f::Zero());  // an angle without an axis
    seg.segment(inliers, coeff);
    EXPECT(!seg.getLastError().empty());
    seg.setModelType(5);  // SACMODEL_CYLINDER
    seg.segment(inliers, coeff);
    EXPECT(inliers.indices.empty() && coeff.values.empty() && !seg.getLastError().empty());
  }
  {  // the constrained planes of the plain class
    SACSegmentation<PointXYZ> seg(ctx);
    seg.setInputCloud(cloud);
    seg.setMethodType(SAC_RANSAC);
    seg.setDistanceThreshold(0.03);
    seg.setSeed(1);
    seg.setOptimizeCoefficients(false);
    seg.setModelType(SACMODEL_PERPENDICULAR_PLANE);
    seg.setAxis(floor_axis);
    seg.setEpsAngle(0.1);
    EXPECT(seg.getAxis()[2] == -1.208f && seg.getEpsAngle() == 0.1);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty() && inliers.indices.size() == want_perp && seg.getLastStats().iterations == it_perp);
    seg.setModelType(SACMODEL_PARALLEL_PLANE);  // the floor runs along `along`, not along its own normal
    seg.setAxis(along);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty() && inliers.indices.size() > 2000);
    seg.setAxis(floor_axis);
    seg.segment(inliers, coeff);
    EXPECT(seg.getLastError().empty() && inliers.indices.size() < 2000);
    seg.setModelType(SACMODEL_NORMAL_PLANE);  // the plain class builds no model with normals
    seg.segment(inliers, coeff);
    EXPECT(inliers.indices.empty() && coeff.values.empty() && !seg.getLastError().empty());
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
