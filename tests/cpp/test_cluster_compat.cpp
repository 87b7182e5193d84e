// C++ host-side test of EuclideanClusterExtraction in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp): bun0 at
// tolerance 0.01 gives clusters of 357, 23, 12, 3, 1 and 1 points (tests/test_cluster_restatement.py pins them on brute
// force).  Input: bun0.txt written by the pytest wrapper (tests/test_gpu_cluster_cpp.py).
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
  EXPECT(cloud->size() == 397);
  const std::size_t want[6] = {357, 23, 12, 3, 1, 1};
  {
    EuclideanClusterExtraction<PointXYZ> ec(ctx);
    EXPECT(ec.getClusterTolerance() == 0.0 && ec.getMinClusterSize() == 1 && ec.getMaxClusterSize() == 0xFFFFFFFFu);
    auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
    ec.setSearchMethod(tree);
    ec.setInputCloud(cloud);
    ec.setClusterTolerance(0.01);
    std::vector<PointIndices> clusters;
    ec.extract(clusters);
    EXPECT(ec.getLastError().empty());
    EXPECT(clusters.size() == 6);
    std::size_t total = 0;
    std::vector<int> seen(cloud->size(), 0);
    for (std::size_t c = 0; c < clusters.size() && c < 6; ++c) {
      const Indices& ind = clusters[c].indices;
      EXPECT(ind.size() == want[c]);
      for (std::size_t j = 0; j < ind.size(); ++j) {
        EXPECT(ind[j] >= 0 && std::size_t(ind[j]) < cloud->size());
        if (j > 0) EXPECT(ind[j - 1] < ind[j]);  // ascending
        ++seen[std::size_t(ind[j])];
        EXPECT(ec.getLabels()[std::size_t(ind[j])] == std::int32_t(c));
      }
      total += ind.size();
    }
    EXPECT(total == cloud->size());
    for (int s : seen) EXPECT(s == 1);
    if (clusters.size() == 6) EXPECT(clusters[4].indices[0] < clusters[5].indices[0]);  // the tie of the singletons
    EXPECT(tree->handle() != nullptr);  // the tree given was the one used
    // the size range, both edges kept
    ec.setMinClusterSize(3);
    ec.setMaxClusterSize(23);
    ec.extract(clusters);
    EXPECT(clusters.size() == 3 && clusters[0].indices.size() == 23 && clusters[2].indices.size() == 3);
  }
  {  // without a tree, on an index subset: ids stay original
    EuclideanClusterExtraction<PointXYZ> ec(ctx);
    auto ind = std::make_shared<Indices>();
    for (index_t i = 0; i < index_t(cloud->size()); i += 3) ind->push_back(i);
    ec.setInputCloud(cloud);
    ec.setIndices(IndicesPtr(ind));
    ec.setClusterTolerance(0.01);
    std::vector<PointIndices> clusters;
    ec.extract(clusters);
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
