// C++ host-side test of CorrespondenceRejectorSampleConsensus in the PCL-compatible mirror (include/pclhip/pcl_compat.hpp) on
// the bunny pairs of the reference's test (test/registration/test_registration_api.cpp:225-263).  Input, from
// tests/test_gpu_rejector_sac_cpp.py: a text file "<n_src> <n_tgt> <n_pairs>", the source points, the target points, the
// pairs, the 16 entries of the golden transform; then the count tests/rejector_sac_restatement.py gives for the seeded call:
//   <file> <seed> <inliers of the seeded run> <its iterations>
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
  auto source = std::make_shared<PointCloud<PointXYZ>>();
  auto target = std::make_shared<PointCloud<PointXYZ>>();
  auto pairs = std::make_shared<Correspondences>();
  Matrix4f golden;
  if (std::FILE* f = std::fopen(argv[1], "r")) {
    int ns = 0, nt = 0, np = 0;
    if (std::fscanf(f, "%d %d %d", &ns, &nt, &np) == 3) {
      float v[3];
      for (int i = 0; i < ns && std::fscanf(f, "%f %f %f", &v[0], &v[1], &v[2]) == 3; ++i) source->push_back(PointXYZ(v[0], v[1], v[2]));
      for (int i = 0; i < nt && std::fscanf(f, "%f %f %f", &v[0], &v[1], &v[2]) == 3; ++i) target->push_back(PointXYZ(v[0], v[1], v[2]));
      int q = 0, m = 0;
      for (int i = 0; i < np && std::fscanf(f, "%d %d", &q, &m) == 2; ++i) pairs->push_back(Correspondence(q, m, 0.0f));
      for (int i = 0; i < 16; ++i)
        if (std::fscanf(f, "%f", &golden.m[i]) != 1) ++failures;
    }
    std::fclose(f);
  }
  EXPECT(source->size() == 397 && target->size() == 361 && pairs->size() == 397);
  const unsigned seed = unsigned(std::atol(argv[2]));
  const std::size_t want = std::size_t(std::atol(argv[3]));
  const int want_iterations = std::atoi(argv[4]);

  registration::CorrespondenceRejectorSampleConsensus<PointXYZ> rej(ctx);
  EXPECT(rej.getInlierThreshold() == 0.05 && rej.getMaximumIterations() == 1000 && !rej.getRefineModel());
  EXPECT(rej.getClassName() == "CorrespondenceRejectorSampleConsensus");
  rej.setMaximumIterations(-5);  // negative values clamp to 0
  EXPECT(rej.getMaximumIterations() == 0);
  Correspondences remaining;
  rej.getRemainingCorrespondences(*pairs, remaining);  // no clouds yet
  EXPECT(remaining.empty() && !rej.getLastError().empty());
  rej.setInputSource(source);
  rej.setInputTarget(target);
  rej.setInlierThreshold(0.01);
  rej.setMaximumIterations(1000);
  rej.setSeed(seed);
  rej.setSaveInliers(true);
  {  // the reference's transform keeps the reference's 97 pairs
    const std::vector<std::uint32_t> c = rej.evaluate(*pairs, {golden, Matrix4f()});
    EXPECT(c.size() == 2 && c[0] == 97u);
  }
  rej.setInputCorrespondences(pairs);
  rej.getCorrespondences(remaining);
  EXPECT(rej.getLastError().empty());
  EXPECT(remaining.size() == want && rej.getLastStats().iterations == want_iterations);
  EXPECT(rej.getLastStats().has_model == 1 && rej.getLastStats().best_count == want);
  Indices pos;
  rej.getInliersIndices(pos);
  EXPECT(pos.size() == remaining.size());
  for (std::size_t i = 0; i < pos.size() && i < remaining.size(); ++i) {
    EXPECT(remaining[i].index_query == (*pairs)[std::size_t(pos[i])].index_query);
    EXPECT(remaining[i].index_match == (*pairs)[std::size_t(pos[i])].index_match);
    if (i > 0) EXPECT(pos[i] > pos[i - 1]);
  }
  const Matrix4f best = rej.getBestTransformation();
  {  // the remaining list is the score of the returned transformation
    const std::vector<std::uint32_t> c = rej.evaluate(*pairs, {best});
    EXPECT(c.size() == 1 && c[0] == want);
  }
  EXPECT(best(3, 0) == 0.0f && best(3, 1) == 0.0f && best(3, 2) == 0.0f && best(3, 3) == 1.0f);
  {  // refused: the output stays empty, the error says why, and the object keeps working
    rej.setRefineModel(true);
    rej.getCorrespondences(remaining);
    EXPECT(remaining.empty() && rej.getLastError().find("setRefineModel") != std::string::npos);
    rej.setRefineModel(false);
    Correspondences twice = *pairs;
    twice[7].index_query = twice[2].index_query;
    rej.getRemainingCorrespondences(twice, remaining);
    EXPECT(remaining.empty() && rej.getLastError().find("twice") != std::string::npos);
    rej.getCorrespondences(remaining);
    EXPECT(remaining.size() == want && rej.getLastError().empty());
  }
  {  // inside IterativeClosestPoint: the reference's IterativeClosestPointWithRejectors on a shifted copy
    auto moved = std::make_shared<PointCloud<PointXYZ>>();
    for (const PointXYZ& p : source->points) moved->push_back(PointXYZ(p.x - 0.03f, p.y - 0.02f, p.z - 0.03f));
    IterativeClosestPoint<PointXYZ, PointXYZ> reg(ctx);
    reg.setMaximumIterations(50);
    reg.setTransformationEpsilon(1e-8);
    reg.setMaxCorrespondenceDistance(0.15);
    auto med = std::make_shared<registration::CorrespondenceRejectorMedianDistance>();
    med->setMedianFactor(4.0);
    reg.addCorrespondenceRejector(med);
    auto sac = std::make_shared<registration::CorrespondenceRejectorSampleConsensus<PointXYZ>>(ctx);
    reg.addCorrespondenceRejector(sac);
    reg.setInputSource(moved);
    reg.setInputTarget(source);
    PointCloud<PointXYZ> out;
    reg.align(out);
    const Matrix4f T = reg.getFinalTransformation();
    EXPECT(reg.hasConverged());
    EXPECT(std::fabs(T(0, 3) - 0.03f) < 1e-2f && std::fabs(T(1, 3) - 0.02f) < 1e-2f && std::fabs(T(2, 3) - 0.03f) < 1e-2f);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) EXPECT(std::fabs(T(r, c) - (r == c ? 1.0f : 0.0f)) < 1e-1f);
    EXPECT(sac->getLastStats().has_model == 1 && sac->getLastStats().n > 3u);
    const Matrix4f B = sac->getBestTransformation();
    EXPECT(std::fabs(B(0, 0) - 1.0f) < 1e-1f && std::fabs(B(0, 3)) < 1e-1f);
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
