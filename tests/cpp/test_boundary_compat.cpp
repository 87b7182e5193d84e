// C++ host-side test of BoundaryEstimation in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp): what
// test/features/test_boundary_estimation.cpp checks on bun0 -- normals with k = n, the basis of every normal, isBoundaryPoint
// by index and by point, and compute() with k = n (its OMP test maps to the same class).  Input: bun0.txt (x y z per line),
// written by the pytest wrapper (tests/test_gpu_boundary_cpp.py).
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
  if (argc < 2) return 2;
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
  const std::size_t n = cloud->size();
  auto indices = std::make_shared<Indices>(n);
  for (std::size_t i = 0; i < n; ++i) (*indices)[i] = index_t(i);
  auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
  tree->setInputCloud(cloud);
  auto normals = std::make_shared<PointCloud<Normal>>();
  {  // every point's normal from all n points: one plane normal for the cloud
    NormalEstimation<PointXYZ> ne(ctx);
    ne.setInputCloud(cloud);
    ne.setSearchMethod(tree);
    ne.setKSearch(int(n));
    ne.compute(*normals);
    EXPECT(normals->size() == n);
  }
  const float half_pi = static_cast<float>(M_PI) / 2.0f;
  const std::size_t probes[4] = {0, n / 3, n / 2, n - 1};
  const bool want[4] = {false, false, false, true};
  for (int omp = 0; omp < 2; ++omp) {  // BoundaryEstimationOMP, BoundaryEstimation
    BoundaryEstimation<PointXYZ, Normal, Boundary> b(ctx);
    if (omp) b.setNumberOfThreads(0);
    b.setInputNormals(normals);
    EXPECT(b.getInputNormals() == normals);
    Vector4f u = Vector4f::Zero(), v = Vector4f::Zero();
    if (!omp && normals->size() == n) {
      for (const auto& point : normals->points) {  // getCoordinateSystemOnPlane
        b.getCoordinateSystemOnPlane(point, u, v);
        const Vector4f n4uv = getNormalVector4f(point);
        EXPECT(std::fabs(n4uv.dot(u)) <= 1e-4f);
        EXPECT(std::fabs(n4uv.dot(v)) <= 1e-4f);
        EXPECT(std::fabs(u.dot(v)) <= 1e-4f);
      }
      for (int p = 0; p < 4; ++p) {  // isBoundaryPoint (indices), (points): the basis of the last normal, as the reference
        EXPECT(b.isBoundaryPoint(*cloud, int(probes[p]), *indices, u, v, half_pi) == want[p]);
        EXPECT(b.isBoundaryPoint(*cloud, (*cloud)[probes[p]], *indices, u, v, half_pi) == want[p]);
      }
      EXPECT(!b.isBoundaryPoint(*cloud, 0, Indices{0, 1}, u, v, half_pi));  // fewer than 3 neighbours
    }
    PointCloud<Boundary> bps;
    b.setInputCloud(cloud);
    b.setIndices(indices);
    b.setSearchMethod(tree);
    b.setKSearch(int(indices->size()));
    b.compute(bps);
    EXPECT(b.getLastError().empty());
    EXPECT(bps.size() == indices->size() && bps.is_dense && b.getInvalidCount() == 0);
    for (int p = 0; p < 4 && bps.size() == n; ++p) EXPECT(bool(bps[probes[p]].boundary_point) == want[p]);
    // the device's flags are the host function's, record by record (the cloud's gaps are far from the threshold)
    for (std::size_t i = 0; i < n && bps.size() == n && normals->size() == n; ++i) {
      b.getCoordinateSystemOnPlane((*normals)[i], u, v);
      EXPECT(bool(bps[i].boundary_point) == b.isBoundaryPoint(*cloud, int(i), *indices, u, v, half_pi));
    }
    // by radius, every point a neighbour: the same flags; a subset keeps its order
    PointCloud<Boundary> by_radius;
    b.setKSearch(0);
    b.setRadiusSearch(10.0);
    b.compute(by_radius);
    EXPECT(b.getLastError().empty() && by_radius.size() == n);
    for (std::size_t i = 0; i < n && by_radius.size() == n && bps.size() == n; ++i)
      EXPECT(by_radius[i].boundary_point == bps[i].boundary_point);
    auto sel = std::make_shared<Indices>(Indices{index_t(n - 1), 0, index_t(n - 1)});
    b.setIndices(sel);
    PointCloud<Boundary> few;
    b.compute(few);
    EXPECT(few.size() == 3 && few[0].boundary_point == 1 && few[1].boundary_point == 0 && few[2].boundary_point == 1);
  }
  {  // what initCompute refuses and what this path does not build leaves the output empty and says why
    BoundaryEstimation<PointXYZ, Normal> b(ctx);
    EXPECT(b.getAngleThreshold() == half_pi);
    PointCloud<Boundary> out;
    b.setInputCloud(cloud);
    b.setRadiusSearch(0.02);
    b.compute(out);  // no normals
    EXPECT(out.empty() && !b.getLastError().empty());
    b.setInputNormals(normals);
    b.setKSearch(10);  // both
    b.compute(out);
    EXPECT(out.empty() && !b.getLastError().empty());
    b.setKSearch(0);
    b.setAngleThreshold(0.2f);  // below pi / 8
    b.compute(out);
    EXPECT(out.empty() && !b.getLastError().empty());
    b.setAngleThreshold(half_pi);
    b.compute(out);
    EXPECT(out.size() == n && b.getLastError().empty());
    // a non-finite record: flag 0, counted, is_dense cleared
    auto holed = std::make_shared<PointCloud<PointXYZ>>(*cloud);
    (*holed)[5].y = std::nanf("");
    b.setInputCloud(holed);
    b.compute(out);
    EXPECT(out.size() == n && !out.is_dense && b.getInvalidCount() == 1 && out[5].boundary_point == 0);
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
