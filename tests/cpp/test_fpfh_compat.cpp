// C++ host-side test of FPFHEstimation / FPFHEstimationOMP in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp):
// the object path of test/features/test_pfh_estimation.cpp:388-444 restated on bun0 with a radius that makes every point a
// neighbour (the reference's test asks for k = 397).  Input: bun0.txt (x y z nx ny nz per line) and the 33 golden values of
// fpfhs[0] (tests/golden/fpfh_bun0.json), both written by the pytest wrapper (tests/test_gpu_fpfh_cpp.py).
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
  auto both = std::make_shared<PointCloud<PointNormal>>();
  {
    std::ifstream f(argv[1]);
    float x, y, z, nx, ny, nz;
    while (f >> x >> y >> z >> nx >> ny >> nz) {
      cloud->push_back(PointXYZ(x, y, z));
      Normal n;
      n.normal_x = nx; n.normal_y = ny; n.normal_z = nz;
      normals->push_back(n);
      PointNormal p;
      p.x = x; p.y = y; p.z = z;
      p.normal_x = nx; p.normal_y = ny; p.normal_z = nz;
      both->push_back(p);
    }
  }
  EXPECT(cloud->size() == 397);
  float gold[33];
  {
    std::ifstream f(argv[2]);
    for (float& g : gold) EXPECT(bool(f >> g));
  }
  PointCloud<FPFHSignature33> fpfhs;
  {
    FPFHEstimation<PointXYZ, Normal, FPFHSignature33> fpfh(ctx);
    fpfh.setInputNormals(normals);
    EXPECT(fpfh.getInputNormals() == normals);
    fpfh.setInputCloud(cloud);
    fpfh.setNrSubdivisions(11, 11, 11);
    auto tree = std::make_shared<search::KdTree<PointXYZ>>(ctx);
    fpfh.setSearchMethod(tree);
    fpfh.setRadiusSearch(1.0);
    EXPECT(fpfh.getRadiusSearch() == 1.0);
    fpfh.compute(fpfhs);
    EXPECT(fpfhs.size() == 397 && fpfhs.is_dense);
    if (fpfhs.size() == 397)
      for (int b = 0; b < 33; ++b) EXPECT(std::fabs(double(fpfhs[0].histogram[b]) - double(gold[b])) < 1e-2);
    // every third point: the same rows (testIndicesAndSearchSurface, test_pfh_estimation.cpp:437-444)
    auto sel = std::make_shared<Indices>();
    for (std::size_t i = 0; i < cloud->size(); i += 3) sel->push_back(index_t(i));
    fpfh.setIndices(sel);
    PointCloud<FPFHSignature33> sub;
    fpfh.compute(sub);
    EXPECT(sub.size() == sel->size());
    for (std::size_t j = 0; j < sub.size() && fpfhs.size() == 397; ++j)
      EXPECT(std::memcmp(sub[j].histogram, fpfhs[std::size_t((*sel)[j])].histogram, sizeof(float) * 33) == 0);
    // what this path does not build leaves the output empty
    fpfh.setKSearch(10);
    fpfh.compute(sub);
    EXPECT(sub.empty());
    fpfh.setKSearch(0);
    fpfh.setNrSubdivisions(5, 11, 11);
    fpfh.compute(sub);
    EXPECT(sub.empty());
  }
  {  // the OMP name and PointNormal records as the normals: the same bits; default search method
    FPFHEstimationOMP<PointXYZ, PointNormal, FPFHSignature33> fpfh(ctx, 4);
    EXPECT(fpfh.getNumberOfThreads() == 4);
    fpfh.setInputCloud(cloud);
    fpfh.setInputNormals(both);
    fpfh.setRadiusSearch(1.0);
    PointCloud<FPFHSignature33> again;
    fpfh.compute(again);
    EXPECT(again.size() == 397 && again.is_dense);
    for (std::size_t i = 0; i < again.size() && fpfhs.size() == 397; ++i)
      EXPECT(std::memcmp(again[i].histogram, fpfhs[i].histogram, sizeof(float) * 33) == 0);
  }
  {  // a non-finite record: a NaN row, is_dense false
    auto holed = std::make_shared<PointCloud<PointXYZ>>(*cloud);
    (*holed)[5].x = std::nanf("");
    holed->is_dense = false;
    FPFHEstimation<PointXYZ, Normal> fpfh(ctx);
    fpfh.setInputCloud(holed);
    fpfh.setInputNormals(normals);
    fpfh.setRadiusSearch(0.02);
    PointCloud<FPFHSignature33> out;
    fpfh.compute(out);
    EXPECT(out.size() == 397 && !out.is_dense && fpfh.getNaNCount() == 1);
    if (out.size() == 397) {
      EXPECT(std::isnan(out[5].histogram[0]) && std::isnan(out[5].histogram[32]));
      EXPECT(!std::isnan(out[6].histogram[0]));
    }
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
