// C++ host-side test of MovingLeastSquares in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp): the object path of
// test/surface/test_moving_least_squares.cpp:95-118 on bun0.  Input: bun0.txt (x y z per line) and the expected records of
// the restatement (index x y z nx ny nz curvature per line), both written by the pytest wrapper
// (tests/test_gpu_mls_cpp.py).
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

struct Want {
  index_t index;
  double v[7];
};

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
  std::vector<Want> want;
  {
    std::ifstream f(argv[2]);
    Want w;
    double id;
    while (f >> id) {
      w.index = index_t(id);
      for (double& v : w.v) EXPECT(bool(f >> v));
      want.push_back(w);
    }
  }
  EXPECT(want.size() == 380);
  auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
  PointCloud<PointNormal> mls_normals;
  MovingLeastSquares<PointXYZ, PointNormal> mls(ctx);
  {  // the reference's test: r = 0.03, order 2, normals
    mls.setInputCloud(cloud);
    mls.setComputeNormals(true);
    mls.setPolynomialOrder(2);
    mls.setSearchMethod(tree);
    mls.setSearchRadius(0.03);
    mls.setNumberOfThreads(1);
    mls.process(mls_normals);
    EXPECT(mls.getLastError().empty());
    EXPECT(mls_normals.size() == 397 && mls_normals.width == 397 && mls_normals.height == 1);
    if (mls_normals.size() == 397) {
      EXPECT(std::fabs(mls_normals[0].x - 0.005417) <= 1e-3);
      EXPECT(std::fabs(mls_normals[0].y - 0.113463) <= 1e-3);
      EXPECT(std::fabs(mls_normals[0].z - 0.040715) <= 1e-3);
      EXPECT(std::fabs(std::fabs(mls_normals[0].normal_x) - 0.111894) <= 1e-3);
      EXPECT(std::fabs(std::fabs(mls_normals[0].normal_y) - 0.594906) <= 1e-3);
      EXPECT(std::fabs(std::fabs(mls_normals[0].normal_z) - 0.795969) <= 1e-3);
      EXPECT(std::fabs(mls_normals[0].curvature - 0.012019) <= 1e-3);
    }
    const auto ids = mls.getCorrespondingIndices();
    EXPECT(ids && ids->indices.size() == 397);
    for (std::size_t i = 0; i < ids->indices.size(); ++i) EXPECT(ids->indices[i] == index_t(i));
    EXPECT(mls.getSearchMethod() == tree && tree->getInputCloud() == cloud && mls.getSqrGaussParam() == 0.03 * 0.03);
  }
  {  // r = 0.01: records are dropped; against the restatement's records (within 1e-5: the exact bound is the Python tier's)
    mls.setSearchRadius(0.01);
    PointCloud<PointNormal> out;
    mls.process(out);
    const auto& ids = mls.getCorrespondingIndices()->indices;
    EXPECT(mls.getLastError().empty() && out.size() == 380 && ids.size() == 380 && mls.getUnrounded().size() == 8 * 380);
    for (std::size_t i = 0; i < out.size() && out.size() == want.size(); ++i) {
      const Want& w = want[i];
      EXPECT(ids[i] == w.index);
      EXPECT(std::fabs(out[i].x - w.v[0]) <= 1e-5 && std::fabs(out[i].y - w.v[1]) <= 1e-5 && std::fabs(out[i].z - w.v[2]) <= 1e-5);
      const double dot = out[i].normal_x * w.v[3] + out[i].normal_y * w.v[4] + out[i].normal_z * w.v[5];
      EXPECT(std::fabs(std::fabs(dot) - 1.0) <= 1e-5 && std::fabs(out[i].curvature - w.v[6]) <= 1e-5);
      EXPECT(float(mls.getUnrounded()[8 * i]) == out[i].x && mls.getUnrounded()[8 * i + 7] >= 3.0);
    }
    // PointXYZ out, no normals: the same points
    MovingLeastSquares<PointXYZ, PointXYZ> plain(ctx);
    plain.setInputCloud(cloud);
    plain.setSearchRadius(0.01);
    PointCloud<PointXYZ> xyz;
    plain.process(xyz);
    EXPECT(plain.getLastError().empty() && xyz.size() == out.size());
    for (std::size_t i = 0; i < xyz.size() && xyz.size() == out.size(); ++i)
      EXPECT(xyz[i].x == out[i].x && xyz[i].y == out[i].y && xyz[i].z == out[i].z);
    // order 1 and the method NONE: the plane, the same record
    PointCloud<PointNormal> a, b;
    mls.setPolynomialOrder(1);
    mls.process(a);
    mls.setPolynomialOrder(2);
    mls.setProjectionMethod(MLSResult::NONE);
    mls.process(b);
    EXPECT(a.size() == 380 && b.size() == 380);
    bool moved = false;
    for (std::size_t i = 0; i < a.size() && a.size() == b.size() && out.size() == a.size(); ++i) {
      EXPECT(a[i].x == b[i].x && a[i].y == b[i].y && a[i].z == b[i].z && a[i].normal_x == b[i].normal_x);
      moved = moved || a[i].x != out[i].x;
    }
    EXPECT(moved);
    mls.setProjectionMethod(MLSResult::SIMPLE);
  }
  {  // what this path does not build, and what process() refuses, leaves the output empty and says why
    PointCloud<PointNormal> out;
    mls.setProjectionMethod(MLSResult::ORTHOGONAL);
    mls.process(out);
    EXPECT(out.empty() && mls.getCorrespondingIndices()->indices.empty() && !mls.getLastError().empty());
    mls.setProjectionMethod(MLSResult::SIMPLE);
    mls.setPolynomialOrder(3);
    mls.process(out);
    EXPECT(out.empty() && !mls.getLastError().empty());
    mls.setPolynomialOrder(2);
    mls.setUpsamplingMethod(MovingLeastSquares<PointXYZ, PointNormal>::SAMPLE_LOCAL_PLANE);
    mls.process(out);
    EXPECT(out.empty() && !mls.getLastError().empty());
    mls.setUpsamplingMethod(MovingLeastSquares<PointXYZ, PointNormal>::NONE);
    mls.setCacheMLSResults(true);
    mls.process(out);
    EXPECT(out.empty() && !mls.getLastError().empty());
    mls.setCacheMLSResults(false);
    mls.setSearchRadius(0.0);
    mls.process(out);
    EXPECT(out.empty() && !mls.getLastError().empty());
    mls.setSearchRadius(0.01);
    mls.setSqrGaussParam(-1.0);
    mls.process(out);
    EXPECT(out.empty() && !mls.getLastError().empty());
    mls.setSearchRadius(0.01);
    mls.process(out);
    EXPECT(out.size() == 380 && mls.getLastError().empty());
    auto sel = std::make_shared<Indices>();
    for (std::size_t i = 0; i < cloud->size(); i += 3) sel->push_back(index_t(i));
    mls.setIndices(sel);
    mls.process(out);
    EXPECT(out.empty() && !mls.getLastError().empty());
  }
  {  // a non-finite record gives no output and is nobody's neighbour
    auto holed = std::make_shared<PointCloud<PointXYZ>>(*cloud);
    (*holed)[31].x = std::nanf("");
    holed->is_dense = false;
    MovingLeastSquares<PointXYZ, PointNormal> m2(ctx);
    m2.setInputCloud(holed);
    m2.setSearchRadius(0.03);
    m2.setComputeNormals(true);
    PointCloud<PointNormal> out;
    m2.process(out);
    EXPECT(m2.getLastError().empty() && out.size() == 396);
    for (const index_t i : m2.getCorrespondingIndices()->indices) EXPECT(i != 31);
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
