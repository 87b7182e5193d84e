// C++ host-side test of ISSKeypoint3D in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp): the object path of
// test/keypoints/test_iss_3d.cpp:56-101 on bun0.  Input: bun0.txt (x y z per line) and the six golden keypoints (x y z per
// line), both written by the pytest wrapper (tests/test_gpu_iss_cpp.py).
#include <cmath>
#include <cstdio>
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

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  int failures = 0;
  auto ctx = std::make_shared<Context>(0);
  if (!ctx->ok()) {
    std::fprintf(stderr, "no device: %s\n", ctx->getLastError().c_str());
    return 3;
  }
  auto cloud = std::make_shared<PointCloud<PointXYZ>>();
  {
    std::ifstream f(argv[1]);
    float x, y, z;
    while (f >> x >> y >> z) cloud->push_back(PointXYZ(x, y, z));
  }
  EXPECT(cloud->size() == 397);
  float gold[6][3];
  {
    std::ifstream f(argv[2]);
    for (auto& g : gold)
      for (float& v : g) EXPECT(bool(f >> v));
  }
  const double cloud_resolution = 0.0058329;
  const index_t records[6] = {31, 98, 143, 178, 332, 371};
  auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
  PointCloud<PointXYZ> keypoints;
  ISSKeypoint3D<PointXYZ, PointXYZ> iss_detector(ctx);
  {  // ISSKeypoint3D_WBE
    iss_detector.setSearchMethod(tree);
    iss_detector.setSalientRadius(6 * cloud_resolution);
    iss_detector.setNonMaxRadius(4 * cloud_resolution);
    iss_detector.setThreshold21(0.975);
    iss_detector.setThreshold32(0.975);
    iss_detector.setMinNeighbors(5);
    iss_detector.setNumberOfThreads(1);
    iss_detector.setInputCloud(cloud);
    iss_detector.compute(keypoints);
    EXPECT(iss_detector.getLastError().empty());
    EXPECT(keypoints.size() == 6 && keypoints.width == 6 && keypoints.height == 1 && keypoints.is_dense);
    for (std::size_t i = 0; i < 6 && keypoints.size() == 6; ++i) {
      EXPECT(std::fabs(keypoints[i].x - gold[i][0]) <= 1e-6);
      EXPECT(std::fabs(keypoints[i].y - gold[i][1]) <= 1e-6);
      EXPECT(std::fabs(keypoints[i].z - gold[i][2]) <= 1e-6);
    }
    const auto ids = iss_detector.getKeypointsIndices();
    EXPECT(ids && ids->indices.size() == 6);
    for (std::size_t i = 0; i < 6 && ids->indices.size() == 6; ++i) EXPECT(ids->indices[i] == records[i]);
    EXPECT(iss_detector.getSearchMethod() == tree && tree->getInputCloud() == cloud);
    // the saliency of a keypoint is its third eigenvalue, and no neighbour's is larger; most records are not salient
    const auto& s = iss_detector.getSaliency();
    const auto& e = iss_detector.getEigenvalues();
    EXPECT(s.size() == 397 && e.size() == 3 * 397);
    std::size_t salient = 0;
    for (std::size_t i = 0; i < s.size(); ++i) salient += s[i] > 0.0 ? 1 : 0;
    EXPECT(salient >= 6 && salient < 397);
    for (std::size_t i = 0; i < 6 && ids->indices.size() == 6 && s.size() == 397; ++i) {
      const std::size_t r = std::size_t(ids->indices[i]);
      EXPECT(s[r] > 0.0 && s[r] == e[3 * r + 2] && e[3 * r] >= e[3 * r + 1] && e[3 * r + 1] >= e[3 * r + 2]);
    }
  }
  {  // the default search method, and the same answer again
    ISSKeypoint3D<PointXYZ> again(ctx, 6 * cloud_resolution);
    again.setNonMaxRadius(4 * cloud_resolution);
    again.setInputCloud(cloud);
    PointCloud<PointXYZ> out;
    again.compute(out);
    EXPECT(out.size() == 6);
    for (std::size_t i = 0; i < out.size() && keypoints.size() == 6; ++i)
      EXPECT(out[i].x == keypoints[i].x && out[i].y == keypoints[i].y && out[i].z == keypoints[i].z);
    // min_neighbors above every neighbourhood: no keypoints, no error
    again.setMinNeighbors(397);
    again.compute(out);
    EXPECT(out.empty() && again.getKeypointsIndices()->indices.empty() && again.getLastError().empty());
  }
  {  // what this path does not build, and what initCompute refuses, leaves the output empty and says why
    PointCloud<PointXYZ> out;
    iss_detector.setBorderRadius(3 * cloud_resolution);
    iss_detector.compute(out);
    EXPECT(out.empty() && iss_detector.getKeypointsIndices()->indices.empty() && !iss_detector.getLastError().empty());
    iss_detector.setBorderRadius(0.0);
    iss_detector.setNormalRadius(4 * cloud_resolution);
    iss_detector.compute(out);
    EXPECT(out.empty() && !iss_detector.getLastError().empty());
    iss_detector.setNormalRadius(0.0);
    iss_detector.setNonMaxRadius(0.0);
    iss_detector.compute(out);
    EXPECT(out.empty() && !iss_detector.getLastError().empty());
    iss_detector.setNonMaxRadius(4 * cloud_resolution);
    auto sel = std::make_shared<Indices>();
    for (std::size_t i = 0; i < cloud->size(); i += 3) sel->push_back(index_t(i));
    iss_detector.setIndices(sel);
    iss_detector.compute(out);
    EXPECT(out.empty() && !iss_detector.getLastError().empty());
  }
  {  // a non-finite record is no keypoint and nobody's neighbour
    auto holed = std::make_shared<PointCloud<PointXYZ>>(*cloud);
    (*holed)[31].x = std::nanf("");
    holed->is_dense = false;
    ISSKeypoint3D<PointXYZ> det(ctx);
    det.setSalientRadius(6 * cloud_resolution);
    det.setNonMaxRadius(4 * cloud_resolution);
    det.setInputCloud(holed);
    PointCloud<PointXYZ> out;
    det.compute(out);
    EXPECT(det.getLastError().empty() && !out.empty());
    for (const index_t i : det.getKeypointsIndices()->indices) EXPECT(i != 31);
    EXPECT(det.getSaliency().size() == 397 && det.getSaliency()[31] == 0.0 && std::isnan(det.getEigenvalues()[3 * 31]));
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
