// C++ host-side test of RegionGrowing in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp).  Input, written by the
// pytest wrapper (tests/test_gpu_region_growing_cpp.py): roof.txt with one "x y z nx ny nz curvature" record per line (the
// roof of tests/region_growing_restatement.py) and labels.txt with the literal restatement's label per record at the
// default parameters and with min/max sizes 30/160.
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
  auto normals = std::make_shared<PointCloud<Normal>>();
  {
    std::ifstream f(argv[1]);
    float v[7];
    while (f >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> v[6]) {
      PointXYZ p;
      p.x = v[0]; p.y = v[1]; p.z = v[2];
      cloud->push_back(p);
      Normal q;
      q.normal_x = v[3]; q.normal_y = v[4]; q.normal_z = v[5]; q.curvature = v[6];
      normals->push_back(q);
    }
  }
  std::vector<int> want, want_sized;
  {
    std::ifstream f(argv[2]);
    int a, b;
    while (f >> a >> b) {
      want.push_back(a);
      want_sized.push_back(b);
    }
  }
  const std::size_t n = cloud->size();
  EXPECT(n == 325 && normals->size() == n && want.size() == n);
  {
    RegionGrowing<PointXYZ, Normal> rg(ctx);
    EXPECT(rg.getNumberOfNeighbours() == 30 && rg.getMinClusterSize() == 1 && rg.getMaxClusterSize() == 0xFFFFFFFFu);
    EXPECT(rg.getSmoothModeFlag() && rg.getCurvatureTestFlag() && !rg.getResidualTestFlag());
    EXPECT(rg.getSmoothnessThreshold() == 30.0f / 180.0f * static_cast<float>(M_PI));
    EXPECT(rg.getCurvatureThreshold() == 0.05f && rg.getResidualThreshold() == 0.05f);
    auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
    rg.setSearchMethod(tree);
    rg.setInputCloud(cloud);
    rg.setInputNormals(normals);
    std::vector<PointIndices> clusters;
    rg.extract(clusters);
    EXPECT(rg.getLastError().empty());
    EXPECT(clusters.size() == 2);
    EXPECT(rg.getLabels().size() == n);
    for (std::size_t i = 0; i < n && i < rg.getLabels().size(); ++i) EXPECT(rg.getLabels()[i] == want[i]);
    std::size_t total = 0;
    for (std::size_t c = 0; c < clusters.size(); ++c) {
      const Indices& ind = clusters[c].indices;
      for (std::size_t j = 0; j < ind.size(); ++j) {
        if (j > 0) EXPECT(ind[j - 1] < ind[j]);  // ascending
        EXPECT(want[std::size_t(ind[j])] == int(c));
      }
      total += ind.size();
    }
    EXPECT(total == n);
    EXPECT(tree->handle() != nullptr);  // the tree given was the one used
    PointIndices seg;
    rg.getSegmentFromPoint(7, seg);
    EXPECT(!clusters.empty() && seg.indices == clusters[std::size_t(want[7])].indices);
    // the size range
    rg.setMinClusterSize(30);
    rg.setMaxClusterSize(160);
    rg.extract(clusters);
    for (std::size_t i = 0; i < n && i < rg.getLabels().size(); ++i) EXPECT(rg.getLabels()[i] == want_sized[i]);
    rg.getSegmentFromPoint(7, seg);
    EXPECT(seg.indices.empty() == (want_sized[7] < 0));
  }
  {  // RegionGrowingTest.SegmentWithoutCloud / WithoutNormals / WithDifferentNormalAndCloudSize / no neighbours
    std::vector<PointIndices> clusters(3);
    RegionGrowing<PointXYZ, Normal> a(ctx);
    a.setInputNormals(normals);
    a.extract(clusters);
    EXPECT(clusters.empty());
    RegionGrowing<PointXYZ, Normal> b(ctx);
    b.setInputCloud(cloud);
    b.extract(clusters);
    EXPECT(clusters.empty());
    auto fewer = std::make_shared<PointCloud<Normal>>(*normals);
    fewer->points.pop_back();
    b.setInputNormals(fewer);
    b.extract(clusters);
    EXPECT(clusters.empty());
    b.setInputNormals(normals);
    b.setNumberOfNeighbours(0);
    b.extract(clusters);
    EXPECT(clusters.empty() && b.getLastError().empty());
  }
  {  // what is not built: an empty output and a reason
    std::vector<PointIndices> clusters;
    RegionGrowing<PointXYZ, Normal> rg(ctx);
    rg.setInputCloud(cloud);
    rg.setInputNormals(normals);
    rg.setCurvatureTestFlag(false);  // switches the residual test on
    EXPECT(rg.getResidualTestFlag());
    rg.extract(clusters);
    EXPECT(clusters.empty() && rg.getLastError().find("residual") != std::string::npos);
    rg.setCurvatureTestFlag(true);
    rg.setResidualTestFlag(false);
    rg.setSmoothModeFlag(false);
    rg.extract(clusters);
    EXPECT(clusters.empty() && rg.getLastError().find("smooth") != std::string::npos);
    rg.setSmoothModeFlag(true);
    rg.setNumberOfNeighbours(65);
    rg.extract(clusters);
    EXPECT(clusters.empty() && rg.getLastError().find("64") != std::string::npos);
    rg.setNumberOfNeighbours(30);
    rg.extract(clusters);
    EXPECT(clusters.size() == 2 && rg.getLastError().empty());
  }
  {  // on an index subset: ids stay original
    RegionGrowing<PointXYZ, Normal> rg(ctx);
    auto ind = std::make_shared<Indices>();
    for (index_t i = 0; i < index_t(n); i += 3) ind->push_back(i);
    rg.setInputCloud(cloud);
    rg.setInputNormals(normals);
    rg.setIndices(IndicesPtr(ind));
    std::vector<PointIndices> clusters;
    rg.extract(clusters);
    std::size_t total = 0;
    for (const PointIndices& c : clusters) {
      total += c.indices.size();
      for (index_t i : c.indices) EXPECT(i % 3 == 0);
    }
    EXPECT(total == ind->size());
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
