// pcl_compat.hpp -- header-only C++ mirror of the PCL plugin surface for the ICP hot path, written against the
// C ABI of pclhip.h (no Eigen, no Boost, no FLANN) for applications that do not have PCL at all.  Same names,
// the same VIRTUAL structure, argument meaning and error behaviour as the reference classes, so user code
// (and PCL's own tests) port by changing the namespace -- including code that plugs its own search method,
// correspondence estimation or transformation estimation into a Registration:
//
//   pclhip::PointXYZ / PointNormal / Normal         common/include/pcl/impl/point_types.hpp:315-321,843-853,787-794
//   pclhip::PointCloud<PointT>                      common/include/pcl/point_cloud.h:173,393-409
//   pclhip::PCLBase<PointT>                         common/include/pcl/pcl_base.h:65-175 (setIndices)
//   pclhip::PointRepresentation<PointT> (+Default, Custom)   common/include/pcl/point_representation.h
//   pclhip::Correspondence(s)                       common/include/pcl/correspondence.h:60-91
//   pclhip::search::Search<PointT> (abstract)       search/include/pcl/search/search.h:60-420
//   pclhip::search::KdTree<PointT>                  search/include/pcl/search/kdtree.h:61-168
//   pclhip::registration::CorrespondenceEstimationBase (abstract) / CorrespondenceEstimation
//                                                   registration/include/pcl/registration/correspondence_estimation.h
//   pclhip::registration::TransformationEstimation (abstract, four overloads) / ...SVD / ...PointToPlaneLLS /
//   ...SymmetricPointToPlaneLLS                     registration/include/pcl/registration/transformation_estimation*.h
//   pclhip::registration::CorrespondenceRejector{Distance,MedianDistance,OneToOne,Trimmed,SampleConsensus}
//   pclhip::Registration<S,T> (abstract) / IterativeClosestPoint / IterativeClosestPointWithNormals
//                                                   registration/include/pcl/registration/registration.h, icp.h
//   pclhip::NormalEstimation, pclhip::VoxelGrid, pclhip::io::loadPCDFile / savePCDFile*
//
// With the stock device-backed parts plugged in (the default), align() runs the whole loop on the GPU
// (pclhip_icp_align); a foreign CorrespondenceEstimation or TransformationEstimation makes it run the generic
// loop of impl/icp.hpp:113-268 through the virtual calls.  With real PCL available the same C ABI sits inside
// subclasses of the real pcl:: bases: include/pclhip/pcl_plugin.hpp.
// Errors follow PCL's convention: no exceptions on the hot path, `false`/0 results + a message (getLastError()).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <array>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <type_traits>
#include <vector>

#include "../pclhip.h"

namespace pclhip {

using index_t = std::int32_t;           // common/include/pcl/types.h:110-133
using uindex_t = std::uint32_t;
using Indices = std::vector<index_t>;
using IndicesPtr = std::shared_ptr<Indices>;
using IndicesConstPtr = std::shared_ptr<const Indices>;

struct alignas(16) PointXYZ {
  float x = 0, y = 0, z = 0, w = 1.0f;  // data[4], data[3] = 1 (point_types.hpp:205-213)
  PointXYZ() = default;
  PointXYZ(float x_, float y_, float z_) : x(x_), y(y_), z(z_), w(1.0f) {}
};
struct alignas(16) Normal {
  float normal_x = 0, normal_y = 0, normal_z = 0, pad0 = 0;
  float curvature = 0, pad1[3] = {0, 0, 0};
};
struct alignas(16) PointNormal {
  float x = 0, y = 0, z = 0, w = 1.0f;
  float normal_x = 0, normal_y = 0, normal_z = 0, pad0 = 0;
  float curvature = 0, pad1[3] = {0, 0, 0};
};
static_assert(sizeof(PointXYZ) == 16 && sizeof(Normal) == 32 && sizeof(PointNormal) == 48, "PCL record sizes");
// This header has exactly two point types, PointXYZ (16 bytes) and PointNormal (48 bytes: normal at +16, curvature at
// +32); their size tells them apart.  (The binding to real PCL classifies a type by its field list instead:
// pcl_plugin.hpp, record_layout.)
template <typename PointT> constexpr bool has_normal_fields() {
  static_assert(std::is_same<PointT, PointXYZ>::value || std::is_same<PointT, PointNormal>::value ||
                    std::is_same<PointT, Normal>::value,
                "pcl_compat.hpp: PointXYZ / PointNormal / Normal records only");
  return sizeof(PointT) >= 48;
}

template <typename PointT>
struct PointCloud {
  using Ptr = std::shared_ptr<PointCloud<PointT>>;
  using ConstPtr = std::shared_ptr<const PointCloud<PointT>>;
  std::vector<PointT> points;
  std::uint32_t width = 0, height = 1;
  bool is_dense = true;
  // acquisition pose (common/include/pcl/point_cloud.h:406-408): origin x y z 0, orientation w x y z;
  // filled from a PCD file's VIEWPOINT line and used as NormalEstimation's default viewpoint
  float sensor_origin_[4] = {0, 0, 0, 0};
  float sensor_orientation_[4] = {1, 0, 0, 0};
  std::size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
  void resize(std::size_t n) { points.resize(n); width = std::uint32_t(n); height = 1; }
  void push_back(const PointT& p) { points.push_back(p); width = std::uint32_t(points.size()); }
  PointT& operator[](std::size_t i) { return points[i]; }
  const PointT& operator[](std::size_t i) const { return points[i]; }
  Ptr makeShared() const { return std::make_shared<PointCloud<PointT>>(*this); }
};

struct Correspondence {
  index_t index_query = 0, index_match = -1;
  float distance = FLT_MAX;  // squared (correspondence.h:66-71)
  Correspondence() = default;
  Correspondence(index_t q, index_t m, float d) : index_query(q), index_match(m), distance(d) {}
};
using Correspondences = std::vector<Correspondence>;
using CorrespondencesPtr = std::shared_ptr<Correspondences>;

struct Matrix4f {  // row-major 4x4 with Eigen's coefficient access (row, col); PCL hands out Eigen::Matrix4f
  float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float& operator()(int r, int c) { return m[4 * r + c]; }
  float operator()(int r, int c) const { return m[4 * r + c]; }
  static Matrix4f Identity() { return Matrix4f(); }
  void setIdentity() { *this = Matrix4f(); }
  Matrix4f operator*(const Matrix4f& o) const {  // Eigen's coefficient order ((a0 b0 + a1 b1) + a2 b2) + a3 b3
    Matrix4f r;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        float s = m[4 * i] * o.m[j] + m[4 * i + 1] * o.m[4 + j];
        s = s + m[4 * i + 2] * o.m[8 + j];
        s = s + m[4 * i + 3] * o.m[12 + j];
        r.m[4 * i + j] = s;
      }
    return r;
  }
};

// One context per device, shared by the objects below (like PCL objects share nothing but the clouds).
class Context {
 public:
  using Ptr = std::shared_ptr<Context>;
  explicit Context(int device = 0, void* hip_stream = nullptr) {
    if (pclhip_ctx_create(device, hip_stream, &ctx_) != PCLHIP_OK) {
      error_ = pclhip_last_error(nullptr);
      ctx_ = nullptr;
    }
  }
  ~Context() { if (ctx_) pclhip_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  bool ok() const { return ctx_ != nullptr; }
  pclhip_ctx* get() const { return ctx_; }
  std::string getLastError() const { return ctx_ ? pclhip_last_error(ctx_) : error_; }
  // the context objects use when none is given: PCL classes are default-constructible, so are these
  static Ptr defaultContext() {
    static Ptr c = std::make_shared<Context>(0);
    return c;
  }
 private:
  pclhip_ctx* ctx_ = nullptr;
  std::string error_;
};

// common/include/pcl/pcl_base.h:65-175
template <typename PointT>
class PCLBase {
 public:
  using PointCloudConstPtr = typename PointCloud<PointT>::ConstPtr;
  virtual ~PCLBase() = default;
  virtual void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  virtual void setIndices(const IndicesPtr& indices) { indices_ = indices; fake_indices_ = false; }
  virtual void setIndices(const IndicesConstPtr& indices) { indices_ = std::make_shared<Indices>(*indices); fake_indices_ = false; }
  IndicesPtr getIndices() { return indices_; }
 protected:
  PointCloudConstPtr input_;
  IndicesPtr indices_;
  bool fake_indices_ = false;
  bool initCompute() {  // impl/pcl_base.hpp:138-174: no indices given -> all points
    if (!input_) return false;
    if (!indices_) { fake_indices_ = true; indices_ = std::make_shared<Indices>(); }
    if (fake_indices_ && indices_->size() != input_->size()) {
      indices_->resize(input_->size());
      for (std::size_t i = 0; i < indices_->size(); ++i) (*indices_)[i] = index_t(i);
    }
    return true;
  }
  bool usesAllPoints() const { return !indices_ || fake_indices_ || indices_->size() == input_->size(); }
};

// common/include/pcl/point_representation.h:59-190, 256-279, 546-579
template <typename PointT>
class PointRepresentation {
 public:
  using Ptr = std::shared_ptr<PointRepresentation<PointT>>;
  using ConstPtr = std::shared_ptr<const PointRepresentation<PointT>>;
  virtual ~PointRepresentation() = default;
  virtual void copyToFloatArray(const PointT& p, float* out) const = 0;
  template <typename OutputType> void vectorize(const PointT& p, OutputType& out) const {
    float t[16] = {0};
    copyToFloatArray(p, t);
    for (int i = 0; i < nr_dimensions_; ++i) out[i] = alpha_.empty() ? t[i] : t[i] * alpha_[std::size_t(i)];
  }
  void setRescaleValues(const float* rescale_array) { alpha_.assign(rescale_array, rescale_array + nr_dimensions_); }
  int getNumberOfDimensions() const { return nr_dimensions_; }
 protected:
  int nr_dimensions_ = 0;
  std::vector<float> alpha_;
};
template <typename PointT>
class DefaultPointRepresentation : public PointRepresentation<PointT> {
 public:
  DefaultPointRepresentation() { this->nr_dimensions_ = 3; }
  void copyToFloatArray(const PointT& p, float* out) const override { out[0] = p.x; out[1] = p.y; out[2] = p.z; }
};
template <typename PointT>
class CustomPointRepresentation : public PointRepresentation<PointT> {
 public:
  explicit CustomPointRepresentation(int max_dim = 3, int start_dim = 0) : start_dim_(start_dim) {
    this->nr_dimensions_ = max_dim < 16 ? max_dim : 16;
  }
  void copyToFloatArray(const PointT& p, float* out) const override {
    const float* f = reinterpret_cast<const float*>(&p) + start_dim_;
    for (int i = 0; i < this->nr_dimensions_; ++i) out[i] = f[i];
  }
 private:
  int start_dim_;
};

namespace search {

// pcl::search::Search<PointT>: what Feature::setSearchMethod and the registration classes talk to.  The batch
// overloads have the reference's default (a loop over the per-point virtual, search.hpp:113-136,164-190).
template <typename PointT>
class Search {
 public:
  using Ptr = std::shared_ptr<Search<PointT>>;
  using ConstPtr = std::shared_ptr<const Search<PointT>>;
  using PointCloudConstPtr = typename PointCloud<PointT>::ConstPtr;
  explicit Search(const std::string& name = "", bool sorted = false) : sorted_results_(sorted), name_(name) {}
  virtual ~Search() = default;
  virtual const std::string& getName() const { return name_; }
  virtual void setSortedResults(bool sorted) { sorted_results_ = sorted; }
  virtual bool getSortedResults() { return sorted_results_; }
  virtual bool setInputCloud(const PointCloudConstPtr& cloud, const IndicesConstPtr& indices = IndicesConstPtr()) = 0;
  virtual PointCloudConstPtr getInputCloud() const { return input_; }
  virtual IndicesConstPtr getIndices() const { return indices_; }
  virtual int nearestKSearch(const PointT& point, int k, Indices& k_indices, std::vector<float>& k_sqr_distances) const = 0;
  virtual int nearestKSearch(const PointCloud<PointT>& cloud, index_t index, int k, Indices& k_indices,
                             std::vector<float>& k_sqr_distances) const {
    return nearestKSearch(cloud[std::size_t(index)], k, k_indices, k_sqr_distances);
  }
  virtual void nearestKSearch(const PointCloud<PointT>& cloud, const Indices& indices, int k, std::vector<Indices>& k_indices,
                              std::vector<std::vector<float>>& k_sqr_distances) const {
    const std::size_t n = indices.empty() ? cloud.size() : indices.size();
    k_indices.assign(n, Indices());
    k_sqr_distances.assign(n, std::vector<float>());
    for (std::size_t i = 0; i < n; ++i)
      nearestKSearch(cloud, indices.empty() ? index_t(i) : indices[i], k, k_indices[i], k_sqr_distances[i]);
  }
  virtual int radiusSearch(const PointT& point, double radius, Indices& k_indices, std::vector<float>& k_sqr_distances,
                           unsigned int max_nn = 0) const = 0;
  // queries of another point type (search.h:166-176,287-297): copied by x, y, z
  template <typename PointTDiff>
  int nearestKSearchT(const PointTDiff& point, int k, Indices& k_indices, std::vector<float>& k_sqr_distances) const {
    PointT p{};
    p.x = point.x; p.y = point.y; p.z = point.z;
    return nearestKSearch(p, k, k_indices, k_sqr_distances);
  }
  template <typename PointTDiff>
  int radiusSearchT(const PointTDiff& point, double radius, Indices& k_indices, std::vector<float>& k_sqr_distances,
                    unsigned int max_nn = 0) const {
    PointT p{};
    p.x = point.x; p.y = point.y; p.z = point.z;
    return radiusSearch(p, radius, k_indices, k_sqr_distances, max_nn);
  }
  // the device searches a whole batch per launch; host threads play no part (kept for source compatibility)
  virtual void setNumberOfThreads(unsigned int) {}
  virtual void radiusSearch(const PointCloud<PointT>& cloud, const Indices& indices, double radius,
                            std::vector<Indices>& k_indices, std::vector<std::vector<float>>& k_sqr_distances,
                            unsigned int max_nn = 0) const {
    const std::size_t n = indices.empty() ? cloud.size() : indices.size();
    k_indices.assign(n, Indices());
    k_sqr_distances.assign(n, std::vector<float>());
    for (std::size_t i = 0; i < n; ++i)
      radiusSearch(cloud[std::size_t(indices.empty() ? index_t(i) : indices[i])], radius, k_indices[i], k_sqr_distances[i], max_nn);
  }
 protected:
  PointCloudConstPtr input_;
  IndicesConstPtr indices_;
  bool sorted_results_;
  std::string name_;
};

// pcl::search::KdTree<PointT> on the device index: setInputCloud / nearestKSearch / radiusSearch (single +
// batch overloads; the batch ones are ONE launch).
template <typename PointT>
class KdTree : public Search<PointT> {
 public:
  using Ptr = std::shared_ptr<KdTree<PointT>>;
  using PointCloudConstPtr = typename PointCloud<PointT>::ConstPtr;
  using PointRepresentationConstPtr = typename PointRepresentation<PointT>::ConstPtr;
  using Search<PointT>::nearestKSearch;
  using Search<PointT>::radiusSearch;
  explicit KdTree(bool sorted = true) : KdTree(Context::defaultContext(), sorted) {}
  explicit KdTree(Context::Ptr ctx, bool sorted = true) : Search<PointT>("KdTree", sorted), ctx_(std::move(ctx)) {}
  ~KdTree() override { if (index_) pclhip_index_destroy(index_); }
  KdTree(const KdTree&) = delete;
  KdTree& operator=(const KdTree&) = delete;
  // search/kdtree.h:130-143, kdtree/kdtree.h:306-323: FLANN's eps allows a (1 + eps) approximate search; this index
  // always answers exactly, which satisfies every eps >= 0.  min_pts_ is stored for the getter (kdtree.h:325-338).
  void setEpsilon(float eps) { epsilon_ = eps; }
  float getEpsilon() const { return epsilon_; }
  void setMinPts(int min_pts) { min_pts_ = min_pts; }
  int getMinPts() const { return min_pts_; }

  // search/include/pcl/search/impl/kdtree.hpp:87-97 -> kdtree_flann.hpp:99-136: always (re)builds, like the
  // reference -- the cloud behind an unchanged pointer may have been modified in place.  Who knows it has not
  // keeps the tree and passes it with setSearchMethodTarget(tree, /*force_no_recompute=*/true).
  bool setInputCloud(const PointCloudConstPtr& cloud, const IndicesConstPtr& indices = IndicesConstPtr()) override {
    if (index_) { pclhip_index_destroy(index_); index_ = nullptr; }
    this->input_ = cloud;
    this->indices_ = indices;
    if (!ctx_ || !ctx_->ok() || !cloud || unsupported_) return false;
    const bool sub = indices && !indices->empty();
    return pclhip_index_build_scaled(ctx_->get(), cloud->points.data(), sizeof(PointT), cloud->size(),
                                     sub ? indices->data() : nullptr, sub ? indices->size() : 0,
                                     scaled_ ? scale_ : nullptr, &index_) == PCLHIP_OK;
  }
  // kdtree.h:110: honoured for (x, y, z) prefixes with rescale values (the index is three-dimensional);
  // any other representation makes setInputCloud fail instead of searching something else
  void setPointRepresentation(const PointRepresentationConstPtr& rep) {
    rep_ = rep;
    scaled_ = unsupported_ = false;
    if (!rep) return;
    const int d = rep->getNumberOfDimensions();
    float probe[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    bool ok = d >= 1 && d <= 3;
    for (int a = 0; a < 3 && ok; ++a) {
      PointT p;
      p.x = a == 0 ? 1.0f : 0.0f; p.y = a == 1 ? 1.0f : 0.0f; p.z = a == 2 ? 1.0f : 0.0f;
      float out[16] = {0};
      rep->vectorize(p, out);
      for (int j = 0; j < d; ++j) probe[a][j] = out[j];
    }
    for (int a = 0; a < 3 && ok; ++a)
      for (int j = 0; j < 3; ++j)
        if (j != a && probe[a][j] != 0.0f) ok = false;
    if (!ok) { unsupported_ = true; return; }
    for (int a = 0; a < 3; ++a) scale_[a] = a < d ? probe[a][a] : 0.0f;
    scaled_ = !(scale_[0] == 1.0f && scale_[1] == 1.0f && scale_[2] == 1.0f);
    if (this->input_) setInputCloud(this->input_, this->indices_);
  }
  PointRepresentationConstPtr getPointRepresentation() const { return rep_; }
  bool hasDefaultRepresentation() const { return !scaled_ && !unsupported_; }

  // kdtree_flann.hpp:234-274: returns the number of neighbours found, resizes the outputs
  int nearestKSearch(const PointT& point, int k, Indices& k_indices, std::vector<float>& k_sqr_distances) const override {
    k_indices.clear();
    k_sqr_distances.clear();
    if (!index_ || k < 1) return 0;
    const std::uint64_t n = pclhip_index_size(index_);
    if (std::uint64_t(k) > n) k = int(n);  // :241-242
    if (k == 0) return 0;
    k_indices.resize(std::size_t(k));
    k_sqr_distances.resize(std::size_t(k));
    if (pclhip_knn(index_, &point, sizeof(PointT), 1, k, k_indices.data(), k_sqr_distances.data()) != PCLHIP_OK) return 0;
    int found = 0;
    while (found < k && k_indices[std::size_t(found)] >= 0) ++found;
    k_indices.resize(std::size_t(found));
    k_sqr_distances.resize(std::size_t(found));
    return found;
  }
  // batch overload, search/include/pcl/search/search.h:216-219 -- the efficient entry: one launch
  void nearestKSearch(const PointCloud<PointT>& cloud, const Indices& indices, int k, std::vector<Indices>& k_indices,
                      std::vector<std::vector<float>>& k_sqr_distances) const override {
    k_indices.clear();
    k_sqr_distances.clear();
    if (!index_ || k < 1) return;
    std::vector<PointT> q;
    const PointT* qp = cloud.points.data();
    std::size_t nq = cloud.size();
    if (!indices.empty()) {
      q.reserve(indices.size());
      for (index_t i : indices) q.push_back(cloud[std::size_t(i)]);
      qp = q.data();
      nq = q.size();
    }
    const std::uint64_t n = pclhip_index_size(index_);
    const int kk = std::uint64_t(k) > n ? int(n) : k;
    k_indices.assign(nq, Indices());
    k_sqr_distances.assign(nq, std::vector<float>());
    if (kk == 0 || nq == 0) return;
    Indices flat_i(nq * std::size_t(kk));
    std::vector<float> flat_d(nq * std::size_t(kk));
    if (pclhip_knn(index_, qp, sizeof(PointT), nq, kk, flat_i.data(), flat_d.data()) != PCLHIP_OK) return;
    for (std::size_t i = 0; i < nq; ++i) {
      int found = 0;
      while (found < kk && flat_i[i * std::size_t(kk) + std::size_t(found)] >= 0) ++found;
      k_indices[i].assign(flat_i.begin() + long(i * std::size_t(kk)), flat_i.begin() + long(i * std::size_t(kk)) + found);
      k_sqr_distances[i].assign(flat_d.begin() + long(i * std::size_t(kk)), flat_d.begin() + long(i * std::size_t(kk)) + found);
    }
  }
  // kdtree_flann.hpp:372-414: neighbours with squared distance < radius^2, ascending; max_nn = 0: all
  int radiusSearch(const PointT& point, double radius, Indices& k_indices, std::vector<float>& k_sqr_distances,
                   unsigned int max_nn = 0) const override {
    k_indices.clear();
    k_sqr_distances.clear();
    if (!index_) return 0;
    std::uint64_t off[2] = {0, 0}, total = 0;
    pclhip_status st = pclhip_radius_search(index_, &point, sizeof(PointT), 1, radius, max_nn, off, nullptr, nullptr, 0, &total);
    if ((st != PCLHIP_OK && st != PCLHIP_ERR_OVERFLOW) || total == 0) return 0;
    k_indices.resize(std::size_t(total));
    k_sqr_distances.resize(std::size_t(total));
    if (pclhip_radius_search(index_, &point, sizeof(PointT), 1, radius, max_nn, off, k_indices.data(),
                             k_sqr_distances.data(), total, &total) != PCLHIP_OK) {
      k_indices.clear();
      k_sqr_distances.clear();
      return 0;
    }
    return int(total);
  }
  // batch overload (search/include/pcl/search/impl/search.hpp:164-190): one call for the whole cloud
  void radiusSearch(const PointCloud<PointT>& cloud, const Indices& indices, double radius,
                    std::vector<Indices>& k_indices, std::vector<std::vector<float>>& k_sqr_distances,
                    unsigned int max_nn = 0) const override {
    k_indices.clear();
    k_sqr_distances.clear();
    if (!index_) return;
    std::vector<PointT> q;
    const PointT* qp = cloud.points.data();
    std::size_t nq = cloud.size();
    if (!indices.empty()) {
      for (index_t i : indices) q.push_back(cloud[std::size_t(i)]);
      qp = q.data();
      nq = q.size();
    }
    k_indices.assign(nq, Indices());
    k_sqr_distances.assign(nq, std::vector<float>());
    if (nq == 0) return;
    std::vector<std::uint64_t> off(nq + 1, 0);
    std::uint64_t total = 0;
    pclhip_status st = pclhip_radius_search(index_, qp, sizeof(PointT), nq, radius, max_nn, off.data(), nullptr, nullptr, 0, &total);
    if ((st != PCLHIP_OK && st != PCLHIP_ERR_OVERFLOW) || total == 0) return;
    Indices flat_i(static_cast<std::size_t>(total), 0);
    std::vector<float> flat_d(static_cast<std::size_t>(total), 0.0f);
    if (pclhip_radius_search(index_, qp, sizeof(PointT), nq, radius, max_nn, off.data(), flat_i.data(), flat_d.data(),
                             total, &total) != PCLHIP_OK) return;
    for (std::size_t i = 0; i < nq; ++i) {
      k_indices[i].assign(flat_i.begin() + long(off[i]), flat_i.begin() + long(off[i + 1]));
      k_sqr_distances[i].assign(flat_d.begin() + long(off[i]), flat_d.begin() + long(off[i + 1]));
    }
  }
  pclhip_index* handle() const { return index_; }
  Context::Ptr context() const { return ctx_; }

 private:
  Context::Ptr ctx_;
  pclhip_index* index_ = nullptr;
  PointRepresentationConstPtr rep_;
  float scale_[3] = {1, 1, 1};
  bool scaled_ = false, unsupported_ = false;
  float epsilon_ = 0.0f;
  int min_pts_ = 1;
};

}  // namespace search

// pcl::NormalEstimation<PointInT, pcl::Normal> (setKSearch or setRadiusSearch).
template <typename PointInT>
class NormalEstimation : public PCLBase<PointInT> {
 public:
  using SearchPtr = typename search::Search<PointInT>::Ptr;  // Feature::KdTreePtr is a search::Search (feature.h:119-120)
  NormalEstimation() : NormalEstimation(Context::defaultContext()) {}
  explicit NormalEstimation(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
  void setSearchMethod(const SearchPtr& tree) { tree_ = tree; }
  SearchPtr getSearchMethod() const { return tree_; }
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setRadiusSearch(double radius) { radius_ = radius; }
  double getRadiusSearch() const { return radius_; }
  double getSearchParameter() const { return k_ >= 1 ? double(k_) : radius_; }  // feature.h:190-197
  // Feature::setSearchSurface (features/include/pcl/features/feature.h:139-153): neighbours come from this cloud, one normal
  // per point of the input cloud (or per index, PCLBase::setIndices); unset = the input cloud itself
  void setSearchSurface(const typename PointCloud<PointInT>::ConstPtr& cloud) { surface_ = cloud; }
  typename PointCloud<PointInT>::ConstPtr getSearchSurface() const { return surface_; }
  void getViewPoint(float& x, float& y, float& z) const { x = vp_[0]; y = vp_[1]; z = vp_[2]; }
  // normal_3d.h:255-262 / :328-351: the cloud's sensor origin is the viewpoint until setViewPoint is called
  void setViewPoint(float x, float y, float z) { vp_[0] = x; vp_[1] = y; vp_[2] = z; use_sensor_origin_ = false; }
  void useSensorOriginAsViewPoint() { use_sensor_origin_ = true; }
  // Feature::compute (features/include/pcl/features/impl/feature.hpp:195-229); initCompute refuses
  // "both radius and K defined" and "neither defined" (:131-174).  The fused device kernel needs the device
  // search method (a foreign Search object has no neighbours-for-all-points entry this class could batch).
  void compute(PointCloud<Normal>& output) {
    output.points.clear();
    const auto& input = this->input_;
    if (!input || (k_ < 1) == !(radius_ > 0.0)) return;
    if (!tree_) tree_ = std::make_shared<search::KdTree<PointInT>>(ctx_);
    auto* dev = dynamic_cast<search::KdTree<PointInT>*>(tree_.get());
    if (dev == nullptr) return;
    const auto& surface = surface_ ? surface_ : input;  // feature.hpp:104-118
    if (dev->getInputCloud() != surface || dev->handle() == nullptr) {  // feature.hpp:125-130
      if (!dev->setInputCloud(surface)) return;
    }
    if (use_sensor_origin_) {
      vp_[0] = input->sensor_origin_[0]; vp_[1] = input->sensor_origin_[1]; vp_[2] = input->sensor_origin_[2];
    }
    const bool subset = this->indices_ && !this->fake_indices_;
    if (surface != input || subset) {  // every (selected) input point is a query against the surface
      const std::size_t m = subset ? this->indices_->size() : input->size();
      output.resize(m);
      std::uint64_t nan = 0;
      std::vector<float> tmp(m * 4);
      const pclhip_status st = pclhip_normals_at(dev->handle(), input->points.data(), sizeof(PointInT), input->size(),
                                                 subset ? this->indices_->data() : nullptr, subset ? m : 0, k_ >= 1 ? k_ : 0,
                                                 k_ >= 1 ? 0.0 : radius_, vp_, tmp.data(), 16, &nan);
      if (st != PCLHIP_OK) { output.points.clear(); return; }
      for (std::size_t i = 0; i < m; ++i) {
        output[i].normal_x = tmp[4 * i]; output[i].normal_y = tmp[4 * i + 1]; output[i].normal_z = tmp[4 * i + 2];
        output[i].curvature = tmp[4 * i + 3];
      }
      output.is_dense = (nan == 0);
      return;
    }
    output.resize(input->size());
    std::uint64_t nan = 0;
    static_assert(sizeof(Normal) == 32, "pcl::Normal: normal at +0, curvature at +16");
    // the output type of this class is pcl::Normal: whole records in one copy (pclhip_normals_records)
    if (pclhip_normals_records(dev->handle(), k_ >= 1 ? k_ : 0, k_ >= 1 ? 0.0 : radius_, vp_, output.points.data(), sizeof(Normal),
                               0, 16, &nan) != PCLHIP_OK) {
      output.points.clear();
      return;
    }
    output.is_dense = (nan == 0);  // normal_3d.hpp:56,63
  }
 private:
  Context::Ptr ctx_;
  SearchPtr tree_;
  typename PointCloud<PointInT>::ConstPtr surface_;
  int k_ = 0;
  double radius_ = 0.0;
  float vp_[3] = {0, 0, 0};
  bool use_sensor_origin_ = true;
};

// pcl::NormalEstimationOMP<PointInT, PointOutT> (features/include/pcl/features/normal_3d_omp.h:53-113): the same
// computation; the thread count of the host loop has no meaning for the one-launch device path and is only stored
template <typename PointInT>
class NormalEstimationOMP : public NormalEstimation<PointInT> {
 public:
  explicit NormalEstimationOMP(unsigned int nr_threads = 0) : NormalEstimation<PointInT>() { setNumberOfThreads(nr_threads); }
  explicit NormalEstimationOMP(Context::Ptr ctx, unsigned int nr_threads = 0) : NormalEstimation<PointInT>(std::move(ctx)) {
    setNumberOfThreads(nr_threads);
  }
  void setNumberOfThreads(unsigned int nr_threads = 0) { threads_ = nr_threads; }
  unsigned int getNumberOfThreads() const { return threads_; }
 private:
  unsigned int threads_ = 0;
};

// pcl::FPFHSignature33 (common/include/pcl/impl/point_types.hpp): 33 floats, f1 | f2 | f3 histograms
struct FPFHSignature33 {
  float histogram[33] = {0};
  static constexpr int descriptorSize() { return 33; }
};
static_assert(sizeof(FPFHSignature33) == 132, "pcl::FPFHSignature33 record size");

// pcl::FPFHEstimation<PointInT, PointNT, PointOutT> (features/include/pcl/features/fpfh.h:79-222, impl/fpfh.hpp:51-303)
// with setRadiusSearch over pclhip_fpfh: the search surface is the input cloud, 11 / 11 / 11 subdivisions.  compute()
// leaves the output empty for what this path does not build (setKSearch, another search surface, other subdivisions, a
// foreign Search object).  PointNT is pcl::Normal or pcl::PointNormal.
template <typename PointInT, typename PointNT, typename PointOutT = FPFHSignature33>
class FPFHEstimation : public PCLBase<PointInT> {
  static_assert(sizeof(PointOutT) == 132, "the output type is pcl::FPFHSignature33");
 public:
  using SearchPtr = typename search::Search<PointInT>::Ptr;
  using PointCloudOut = PointCloud<PointOutT>;
  using PointCloudNConstPtr = typename PointCloud<PointNT>::ConstPtr;
  FPFHEstimation() : FPFHEstimation(Context::defaultContext()) {}
  explicit FPFHEstimation(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
  void setInputNormals(const PointCloudNConstPtr& normals) { normals_ = normals; }  // feature.h:339-349
  PointCloudNConstPtr getInputNormals() const { return normals_; }
  void setSearchMethod(const SearchPtr& tree) { tree_ = tree; }
  SearchPtr getSearchMethod() const { return tree_; }
  void setSearchSurface(const typename PointCloud<PointInT>::ConstPtr& cloud) { surface_ = cloud; }
  typename PointCloud<PointInT>::ConstPtr getSearchSurface() const { return surface_; }
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setRadiusSearch(double radius) { radius_ = radius; }
  double getRadiusSearch() const { return radius_; }
  double getSearchParameter() const { return k_ >= 1 ? double(k_) : radius_; }
  void setNrSubdivisions(int nr_bins_f1, int nr_bins_f2, int nr_bins_f3) { bins_[0] = nr_bins_f1; bins_[1] = nr_bins_f2; bins_[2] = nr_bins_f3; }
  void getNrSubdivisions(int& nr_bins_f1, int& nr_bins_f2, int& nr_bins_f3) const { nr_bins_f1 = bins_[0]; nr_bins_f2 = bins_[1]; nr_bins_f3 = bins_[2]; }
  std::uint64_t getNaNCount() const { return nan_; }
  void compute(PointCloudOut& output) {
    output.points.clear();
    output.is_dense = true;
    const auto& input = this->input_;
    if (!input || !normals_ || normals_->size() != input->size()) return;  // feature.hpp:241-250
    if (k_ != 0 || !(radius_ > 0.0) || (surface_ && surface_ != input)) return;
    if (bins_[0] != 11 || bins_[1] != 11 || bins_[2] != 11) return;
    if (!tree_) tree_ = std::make_shared<search::KdTree<PointInT>>(ctx_);
    auto* dev = dynamic_cast<search::KdTree<PointInT>*>(tree_.get());
    if (dev == nullptr) return;
    if (dev->getInputCloud() != input || dev->handle() == nullptr) {
      if (!dev->setInputCloud(input)) return;
    }
    if (input->size() > 0 &&
        pclhip_index_set_normals(dev->handle(), &normals_->points[0].normal_x, sizeof(PointNT)) != PCLHIP_OK)
      return;
    const bool subset = this->indices_ && !this->fake_indices_;
    const std::size_t m = subset ? this->indices_->size() : input->size();
    output.resize(m);
    nan_ = 0;
    if (pclhip_fpfh(dev->handle(), subset ? this->indices_->data() : nullptr, subset ? m : 0, radius_, output.points.data(),
                    sizeof(PointOutT), nullptr, &nan_) != PCLHIP_OK) {
      output.points.clear();
      return;
    }
    output.is_dense = (nan_ == 0);  // fpfh.hpp:248-261
  }
 private:
  Context::Ptr ctx_;
  SearchPtr tree_;
  typename PointCloud<PointInT>::ConstPtr surface_;
  PointCloudNConstPtr normals_;
  int k_ = 0;
  double radius_ = 0.0;
  int bins_[3] = {11, 11, 11};
  std::uint64_t nan_ = 0;
};

// pcl::FPFHEstimationOMP (features/include/pcl/features/fpfh_omp.h): the same computation; the thread count is only stored
template <typename PointInT, typename PointNT, typename PointOutT = FPFHSignature33>
class FPFHEstimationOMP : public FPFHEstimation<PointInT, PointNT, PointOutT> {
 public:
  explicit FPFHEstimationOMP(unsigned int nr_threads = 0) : FPFHEstimation<PointInT, PointNT, PointOutT>() { setNumberOfThreads(nr_threads); }
  explicit FPFHEstimationOMP(Context::Ptr ctx, unsigned int nr_threads = 0) : FPFHEstimation<PointInT, PointNT, PointOutT>(std::move(ctx)) {
    setNumberOfThreads(nr_threads);
  }
  void setNumberOfThreads(unsigned int nr_threads = 0) { threads_ = nr_threads; }
  unsigned int getNumberOfThreads() const { return threads_; }
 private:
  unsigned int threads_ = 0;
};

// pcl::Boundary (common/include/pcl/impl/point_types.hpp): one byte, 1 for a boundary point
struct Boundary {
  std::uint8_t boundary_point = 0;
};
static_assert(sizeof(Boundary) == 1, "pcl::Boundary: the flag is the record");

// What the reference's boundary code uses of Eigen::Vector4f: four floats, Zero(), coefficient access and dot().
struct Vector4f {
  float v[4] = {0, 0, 0, 0};
  Vector4f() = default;
  Vector4f(float a, float b, float c, float d) : v{a, b, c, d} {}
  static Vector4f Zero() { return Vector4f(); }
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
  float dot(const Vector4f& o) const { return ((v[0] * o.v[0] + v[1] * o.v[1]) + v[2] * o.v[2]) + v[3] * o.v[3]; }
};
template <typename PointNT>
inline Vector4f getNormalVector4f(const PointNT& p) { return Vector4f(p.normal_x, p.normal_y, p.normal_z, 0.0f); }

// pcl::BoundaryEstimation<PointInT, PointNT, PointOutT> (features/include/pcl/features/boundary.h:79-178, impl/boundary.hpp
// :87-209) over pclhip_boundary, by radius or by k.  getCoordinateSystemOnPlane and isBoundaryPoint are the reference's host
// functions restated (Eigen's unitOrthogonal rule for 4-vectors written out; the angles sorted on the host).  compute()
// leaves the output empty and says why in getLastError() for what this path does not build: another search surface, a
// foreign Search, an angle threshold below pi / 8.  PointNT is pcl::Normal or pcl::PointNormal.
template <typename PointInT, typename PointNT, typename PointOutT = Boundary>
class BoundaryEstimation : public PCLBase<PointInT> {
  static_assert(sizeof(PointOutT) == 1, "the output type is pcl::Boundary");
 public:
  using SearchPtr = typename search::Search<PointInT>::Ptr;
  using PointCloudOut = PointCloud<PointOutT>;
  using PointCloudNConstPtr = typename PointCloud<PointNT>::ConstPtr;
  BoundaryEstimation() : BoundaryEstimation(Context::defaultContext()) {}
  explicit BoundaryEstimation(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
  virtual ~BoundaryEstimation() = default;
  void setInputNormals(const PointCloudNConstPtr& normals) { normals_ = normals; }
  PointCloudNConstPtr getInputNormals() const { return normals_; }
  void setSearchMethod(const SearchPtr& tree) { tree_ = tree; }
  SearchPtr getSearchMethod() const { return tree_; }
  void setSearchSurface(const typename PointCloud<PointInT>::ConstPtr& cloud) { surface_ = cloud; }
  typename PointCloud<PointInT>::ConstPtr getSearchSurface() const { return surface_; }
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setRadiusSearch(double radius) { radius_ = radius; }
  double getRadiusSearch() const { return radius_; }
  double getSearchParameter() const { return k_ >= 1 ? double(k_) : radius_; }
  void setAngleThreshold(float angle) { angle_threshold_ = angle; }  // boundary.h:131-141
  float getAngleThreshold() const { return angle_threshold_; }
  void setNumberOfThreads(unsigned int nr_threads = 0) { threads_ = nr_threads; }  // only stored
  unsigned int getNumberOfThreads() const { return threads_; }
  std::uint64_t getInvalidCount() const { return invalid_; }
  const std::string& getLastError() const { return error_; }

  // boundary.h:161-168
  void getCoordinateSystemOnPlane(const PointNT& p_coeff, Vector4f& u, Vector4f& v) const {
    const Vector4f n = getNormalVector4f(p_coeff);
    int maxi = 0;  // the first index of the largest |coefficient|
    for (int i = 1; i < 4; ++i)
      if (std::fabs(n[i]) > std::fabs(n[maxi])) maxi = i;
    const int sndi = maxi == 0 ? 1 : 0;
    const float inv = 1.0f / std::sqrt(n[sndi] * n[sndi] + n[maxi] * n[maxi]);
    v = Vector4f::Zero();
    v[maxi] = -n[sndi] * inv;
    v[sndi] = n[maxi] * inv;
    u = Vector4f(n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0], 0.0f);
  }
  // impl/boundary.hpp:72-84, 87-137
  bool isBoundaryPoint(const PointCloud<PointInT>& cloud, int q_idx, const Indices& indices, const Vector4f& u,
                       const Vector4f& v, float angle_threshold) const {
    return isBoundaryPoint(cloud, cloud[std::size_t(q_idx)], indices, u, v, angle_threshold);
  }
  bool isBoundaryPoint(const PointCloud<PointInT>& cloud, const PointInT& q_point, const Indices& indices, const Vector4f& u,
                       const Vector4f& v, float angle_threshold) const {
    if (indices.size() < 3) return false;
    if (!std::isfinite(q_point.x) || !std::isfinite(q_point.y) || !std::isfinite(q_point.z)) return false;
    std::vector<float> angles;
    angles.reserve(indices.size());
    for (const index_t i : indices) {
      const PointInT& p = cloud[std::size_t(i)];
      if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
      const Vector4f delta(p.x - q_point.x, p.y - q_point.y, p.z - q_point.z, 0.0f);
      if (delta[0] == 0.0f && delta[1] == 0.0f && delta[2] == 0.0f) continue;
      angles.push_back(std::atan2(v.dot(delta), u.dot(delta)));
    }
    if (angles.empty()) return false;
    std::sort(angles.begin(), angles.end());
    float max_dif = 0.0f;
    for (std::size_t i = 0; i + 1 < angles.size(); ++i) max_dif = std::max(max_dif, angles[i + 1] - angles[i]);
    max_dif = std::max(max_dif, 2 * static_cast<float>(M_PI) - angles.back() + angles.front());
    return max_dif > angle_threshold;
  }

  // Feature::compute (impl/feature.hpp:195-229)
  void compute(PointCloudOut& output) {
    output.points.clear();
    output.is_dense = true;
    error_.clear();
    invalid_ = 0;
    const char* why = nullptr;
    const auto& input = this->input_;
    if (!input) why = "no input cloud";
    else if (!normals_ || normals_->size() != input->size()) why = "the normals do not match the input cloud";  // feature.hpp:241-250
    else if ((k_ >= 1) == (radius_ > 0.0)) why = "exactly one of setKSearch and setRadiusSearch must be given";  // :131-174
    else if (surface_ && surface_ != input) why = "a search surface other than the input is not built";
    else if (!ctx_ || !ctx_->ok()) why = "no device";
    if (why != nullptr) {
      error_ = why;
      return;
    }
    computeFeature(output);
  }

 protected:
  virtual void computeFeature(PointCloudOut& output) {
    const auto& input = this->input_;
    if (!tree_) tree_ = std::make_shared<search::KdTree<PointInT>>(ctx_);
    auto* dev = dynamic_cast<search::KdTree<PointInT>*>(tree_.get());
    if (dev == nullptr) {
      error_ = "the search method is not a pclhip::search::KdTree";
      return;
    }
    if (dev->getInputCloud() != input || dev->handle() == nullptr) {
      if (!dev->setInputCloud(input)) {
        error_ = pclhip_last_error(ctx_->get());
        return;
      }
    }
    if (input->size() > 0 &&
        pclhip_index_set_normals(dev->handle(), &normals_->points[0].normal_x, sizeof(PointNT)) != PCLHIP_OK) {
      error_ = pclhip_last_error(dev->context()->get());
      return;
    }
    const bool subset = this->indices_ && !this->fake_indices_;
    const std::size_t m = subset ? this->indices_->size() : input->size();
    output.resize(m);
    output.height = 1;
    if (m == 0) return;
    if (pclhip_boundary(dev->handle(), subset ? this->indices_->data() : nullptr, subset ? m : 0, k_ >= 1 ? 0.0 : radius_,
                        k_ >= 1 ? k_ : 0, double(angle_threshold_), 3,
                        m > 0 ? reinterpret_cast<std::uint8_t*>(output.points.data()) : nullptr, &invalid_) != PCLHIP_OK) {
      error_ = pclhip_last_error(dev->context()->get());
      output.points.clear();
      return;
    }
    output.height = 1;
    output.is_dense = (invalid_ == 0);  // impl/boundary.hpp:164-177, 190-203
  }

 private:
  Context::Ptr ctx_;
  SearchPtr tree_;
  typename PointCloud<PointInT>::ConstPtr surface_;
  PointCloudNConstPtr normals_;
  int k_ = 0;
  double radius_ = 0.0;
  float angle_threshold_ = static_cast<float>(M_PI) / 2.0f;  // boundary.h:91
  unsigned int threads_ = 0;
  std::uint64_t invalid_ = 0;
  std::string error_;
};

namespace registration {

// pcl::registration::CorrespondenceRejector{Distance,MedianDistance,OneToOne,Trimmed}: parameter holders;
// the rejection itself runs on the device inside the ICP iteration (pclhip_icp_set_rejectors).
class CorrespondenceRejector {
 public:
  using Ptr = std::shared_ptr<CorrespondenceRejector>;
  pclhip_rejector desc{PCLHIP_REJ_DISTANCE, 0.0, 0, 0};
  virtual ~CorrespondenceRejector() = default;
  const std::string& getClassName() const { return rejection_name_; }
  // after an alignment: what the chain's last application left for this object's getters (SampleConsensus)
  virtual void readBack(const pclhip_icp*) {}
 protected:
  std::string rejection_name_;
};
struct CorrespondenceRejectorDistance : CorrespondenceRejector {
  CorrespondenceRejectorDistance() { desc.kind = PCLHIP_REJ_DISTANCE; rejection_name_ = "CorrespondenceRejectorDistance"; }
  void setMaximumDistance(float d) { desc.param = d; }  // correspondence_rejection_distance.h:93-97
  float getMaximumDistance() const { return float(desc.param); }
};
struct CorrespondenceRejectorMedianDistance : CorrespondenceRejector {
  CorrespondenceRejectorMedianDistance() {
    desc.kind = PCLHIP_REJ_MEDIAN_DISTANCE; desc.param = 1.0; rejection_name_ = "CorrespondenceRejectorMedianDistance";
  }
  void setMedianFactor(double f) { desc.param = f; }
  double getMedianFactor() const { return desc.param; }
};
struct CorrespondenceRejectorOneToOne : CorrespondenceRejector {
  CorrespondenceRejectorOneToOne() { desc.kind = PCLHIP_REJ_ONE_TO_ONE; rejection_name_ = "CorrespondenceRejectorOneToOne"; }
};
struct CorrespondenceRejectorTrimmed : CorrespondenceRejector {
  CorrespondenceRejectorTrimmed() { desc.kind = PCLHIP_REJ_TRIMMED; desc.param = 0.5; rejection_name_ = "CorrespondenceRejectorTrimmed"; }
  void setOverlapRatio(float r) { desc.param = r; }
  float getOverlapRatio() const { return float(desc.param); }
  void setMinCorrespondences(unsigned n) { desc.min_correspondences = n; }
  unsigned getMinCorrespondences() const { return desc.min_correspondences; }
};

// pcl::registration::CorrespondenceRejectorSampleConsensus<PointT> (correspondence_rejection_sample_consensus.h,
// impl/correspondence_rejection_sample_consensus.hpp:55-142; the semantics are stated in include/pclhip.h): standalone through
// getRemainingCorrespondences / setInputCorrespondences + getCorrespondences, or a member of an ICP's chain
// (addCorrespondenceRejector), where the inlier threshold, max_iterations and the seed travel in `desc` and
// getBestTransformation() is filled after the alignment.  setRefineModel(true) is not built: the output stays empty and
// getLastError() says why.
template <typename PointT>
class CorrespondenceRejectorSampleConsensus : public CorrespondenceRejector {
 public:
  using Ptr = std::shared_ptr<CorrespondenceRejectorSampleConsensus<PointT>>;
  using ConstPtr = std::shared_ptr<const CorrespondenceRejectorSampleConsensus<PointT>>;
  using PointCloudConstPtr = typename PointCloud<PointT>::ConstPtr;
  CorrespondenceRejectorSampleConsensus() : CorrespondenceRejectorSampleConsensus(Context::defaultContext()) {}
  explicit CorrespondenceRejectorSampleConsensus(Context::Ptr ctx) : ctx_(std::move(ctx)) {
    desc.kind = PCLHIP_REJ_SAMPLE_CONSENSUS;
    desc.param = 0.05;                // inlier_threshold_
    desc.min_correspondences = 1000;  // max_iterations_
    desc.reserved = 0;                // the seed of the draws
    rejection_name_ = "CorrespondenceRejectorSampleConsensus";
  }
  void setInputSource(const PointCloudConstPtr& cloud) { input_ = cloud; }
  PointCloudConstPtr getInputSource() const { return input_; }
  void setInputTarget(const PointCloudConstPtr& cloud) { target_ = cloud; }
  PointCloudConstPtr getInputTarget() const { return target_; }
  bool requiresSourcePoints() const { return true; }
  bool requiresTargetPoints() const { return true; }
  void setInlierThreshold(double threshold) { desc.param = threshold; }
  double getInlierThreshold() const { return desc.param; }
  void setMaximumIterations(int max_iterations) { desc.min_correspondences = unsigned(std::max(max_iterations, 0)); }  // :177
  int getMaximumIterations() const { return int(desc.min_correspondences); }
  void setRefineModel(bool refine) { refine_ = refine; }
  bool getRefineModel() const { return refine_; }
  void setSaveInliers(bool s) { save_inliers_ = s; }
  bool getSaveInliers() const { return save_inliers_; }
  void setSeed(std::uint32_t seed) { desc.reserved = seed; }
  std::uint32_t getSeed() const { return desc.reserved; }
  Matrix4f getBestTransformation() const { return best_transformation_; }
  void getInliersIndices(Indices& indices) const { indices = inlier_indices_; }
  const pclhip_rejector_sac_stats& getLastStats() const { return stats_; }
  const std::string& getLastError() const { return error_; }

  void setInputCorrespondences(const CorrespondencesPtr& correspondences) { input_correspondences_ = correspondences; }
  void getCorrespondences(Correspondences& correspondences) {
    correspondences.clear();
    if (input_correspondences_) getRemainingCorrespondences(*input_correspondences_, correspondences);
  }

  void getRemainingCorrespondences(const Correspondences& original, Correspondences& remaining) {
    remaining.clear();
    error_.clear();
    if (save_inliers_) inlier_indices_.clear();
    if (!input_ || !target_ || !ctx_ || !ctx_->ok()) {
      error_ = rejection_name_ + ": setInputSource and setInputTarget first";
      return;
    }
    Indices q, m;
    lists(original, q, m);
    pclhip_rejector_sac_params p = params();
    Indices pos(original.size());
    std::uint64_t n_out = 0;
    const pclhip_status rc = pclhip_correspondence_rejector_sample_consensus(
        ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), target_->points.data(), target_->size(),
        sizeof(PointT), q.data(), m.data(), original.size(), &p, pos.data(), pos.size(), &n_out, best_transformation_.m,
        &stats_);
    if (rc != PCLHIP_OK) {  // refused (refine, duplicate query indices, an index outside a cloud): an empty solution
      error_ = pclhip_last_error(ctx_->get());
      best_transformation_.setIdentity();
      return;
    }
    remaining.reserve(std::size_t(n_out));
    for (std::uint64_t i = 0; i < n_out; ++i) remaining.push_back(original[std::size_t(pos[std::size_t(i)])]);
    if (save_inliers_ && stats_.has_model) inlier_indices_.assign(pos.begin(), pos.begin() + std::ptrdiff_t(n_out));
  }

  // countWithinDistance of row-major 4x4 transforms over a list (exposed for tests)
  std::vector<std::uint32_t> evaluate(const Correspondences& list, const std::vector<Matrix4f>& transforms) {
    std::vector<std::uint32_t> counts(transforms.size(), 0u);
    error_.clear();
    if (!input_ || !target_ || !ctx_ || !ctx_->ok() || transforms.empty()) return counts;
    Indices q, m;
    lists(list, q, m);
    std::vector<float> T(16 * transforms.size());
    for (std::size_t i = 0; i < transforms.size(); ++i) std::memcpy(&T[16 * i], transforms[i].m, 16 * sizeof(float));
    if (pclhip_rejector_sac_evaluate(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT),
                                     target_->points.data(), target_->size(), sizeof(PointT), q.data(), m.data(), list.size(),
                                     desc.param, T.data(), int(transforms.size()), counts.data()) != PCLHIP_OK)
      error_ = pclhip_last_error(ctx_->get());
    return counts;
  }

  void readBack(const pclhip_icp* icp) override {
    if (pclhip_icp_last_sac_transformation(icp, best_transformation_.m) != PCLHIP_OK) best_transformation_.setIdentity();
    if (pclhip_icp_last_sac_stats(icp, &stats_) != PCLHIP_OK) stats_ = pclhip_rejector_sac_stats();
  }

 private:
  static void lists(const Correspondences& c, Indices& q, Indices& m) {
    q.resize(c.size());
    m.resize(c.size());
    for (std::size_t i = 0; i < c.size(); ++i) {
      q[i] = c[i].index_query;
      m[i] = c[i].index_match;
    }
  }
  pclhip_rejector_sac_params params() const {
    pclhip_rejector_sac_params p;
    pclhip_rejector_sac_params_default(&p);
    p.inlier_threshold = desc.param;
    p.max_iterations = int(desc.min_correspondences);
    p.seed = desc.reserved;
    p.refine = refine_ ? 1 : 0;
    return p;
  }
  Context::Ptr ctx_;
  PointCloudConstPtr input_, target_;
  CorrespondencesPtr input_correspondences_;
  bool refine_ = false, save_inliers_ = false;
  Matrix4f best_transformation_;
  Indices inlier_indices_;
  pclhip_rejector_sac_stats stats_ = pclhip_rejector_sac_stats();
  std::string error_;
};

// pcl::registration::TransformationEstimation (transformation_estimation.h:50-125): the four overloads
template <typename PointSource, typename PointTarget>
class TransformationEstimation {
 public:
  using Ptr = std::shared_ptr<TransformationEstimation<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const TransformationEstimation<PointSource, PointTarget>>;
  using Matrix4 = Matrix4f;
  virtual ~TransformationEstimation() = default;
  virtual void estimateRigidTransformation(const PointCloud<PointSource>& cloud_src, const PointCloud<PointTarget>& cloud_tgt,
                                           Matrix4& transformation_matrix) const = 0;
  virtual void estimateRigidTransformation(const PointCloud<PointSource>& cloud_src, const Indices& indices_src,
                                           const PointCloud<PointTarget>& cloud_tgt, Matrix4& transformation_matrix) const = 0;
  virtual void estimateRigidTransformation(const PointCloud<PointSource>& cloud_src, const Indices& indices_src,
                                           const PointCloud<PointTarget>& cloud_tgt, const Indices& indices_tgt,
                                           Matrix4& transformation_matrix) const = 0;
  virtual void estimateRigidTransformation(const PointCloud<PointSource>& cloud_src, const PointCloud<PointTarget>& cloud_tgt,
                                           const Correspondences& correspondences, Matrix4& transformation_matrix) const = 0;
};

// The three estimators of the path on the device (pclhip_estimate_rigid_transformation): pair i = (src[i],
// tgt[i]) after the index lists / correspondences have been resolved (transformation_estimation_svd.hpp:49-125,
// ..._point_to_plane_lls.hpp:50-130).  Normals are read from the PointNormal layout (+16 bytes).  On failure
// (size mismatch, missing normals, no device) the matrix is left untouched, as the reference does.
template <typename PointSource, typename PointTarget, int MODE>
class DeviceTransformationEstimation : public TransformationEstimation<PointSource, PointTarget> {
 public:
  using Matrix4 = Matrix4f;
  DeviceTransformationEstimation() : ctx_(Context::defaultContext()) {}
  explicit DeviceTransformationEstimation(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
  static constexpr int mode() { return MODE; }
  void setEnforceSameDirectionNormals(bool on) { enforce_ = on; }  // symmetric objective only
  bool getEnforceSameDirectionNormals() const { return enforce_; }
  void estimateRigidTransformation(const PointCloud<PointSource>& src, const PointCloud<PointTarget>& tgt,
                                   Matrix4& T) const override {
    if (src.size() != tgt.size()) return;  // "Number or points in source differs than target"
    run(src.points.data(), tgt.points.data(), src.size(), T);
  }
  void estimateRigidTransformation(const PointCloud<PointSource>& src, const Indices& indices_src,
                                   const PointCloud<PointTarget>& tgt, Matrix4& T) const override {
    if (indices_src.size() != tgt.size()) return;
    std::vector<PointSource> s;
    s.reserve(indices_src.size());
    for (index_t i : indices_src) s.push_back(src[std::size_t(i)]);
    run(s.data(), tgt.points.data(), s.size(), T);
  }
  void estimateRigidTransformation(const PointCloud<PointSource>& src, const Indices& indices_src,
                                   const PointCloud<PointTarget>& tgt, const Indices& indices_tgt, Matrix4& T) const override {
    if (indices_src.size() != indices_tgt.size()) return;
    std::vector<PointSource> s;
    std::vector<PointTarget> t;
    s.reserve(indices_src.size());
    t.reserve(indices_tgt.size());
    for (index_t i : indices_src) s.push_back(src[std::size_t(i)]);
    for (index_t i : indices_tgt) t.push_back(tgt[std::size_t(i)]);
    run(s.data(), t.data(), s.size(), T);
  }
  void estimateRigidTransformation(const PointCloud<PointSource>& src, const PointCloud<PointTarget>& tgt,
                                   const Correspondences& correspondences, Matrix4& T) const override {
    std::vector<PointSource> s;
    std::vector<PointTarget> t;
    s.reserve(correspondences.size());
    t.reserve(correspondences.size());
    for (const Correspondence& c : correspondences) {
      s.push_back(src[std::size_t(c.index_query)]);
      t.push_back(tgt[std::size_t(c.index_match)]);
    }
    run(s.data(), t.data(), s.size(), T);
  }
 private:
  void run(const PointSource* s, const PointTarget* t, std::size_t n, Matrix4& T) const {
    if (!ctx_ || !ctx_->ok()) return;
    const char* sb = reinterpret_cast<const char*>(s);
    const char* tb = reinterpret_cast<const char*>(t);
    const void* sn = (MODE == PCLHIP_ICP_SYMMETRIC && has_normal_fields<PointSource>()) ? sb + 16 : nullptr;
    const void* tn = (MODE != PCLHIP_ICP_POINT_TO_POINT && has_normal_fields<PointTarget>()) ? tb + 16 : nullptr;
    Matrix4 R;
    if (pclhip_estimate_rigid_transformation(ctx_->get(), MODE, sb, sizeof(PointSource), sn, sizeof(PointSource), tb,
                                             sizeof(PointTarget), tn, sizeof(PointTarget), n, enforce_ ? 1 : 0, R.m,
                                             nullptr) == PCLHIP_OK)
      T = R;
  }
  Context::Ptr ctx_;
  bool enforce_ = true;
};
template <typename S, typename T> using TransformationEstimationSVD = DeviceTransformationEstimation<S, T, PCLHIP_ICP_POINT_TO_POINT>;
template <typename S, typename T> using TransformationEstimationPointToPlaneLLS = DeviceTransformationEstimation<S, T, PCLHIP_ICP_POINT_TO_PLANE>;
template <typename S, typename T> using TransformationEstimationSymmetricPointToPlaneLLS = DeviceTransformationEstimation<S, T, PCLHIP_ICP_SYMMETRIC>;

// pcl::registration::CorrespondenceEstimationBase (correspondence_estimation.h:62-330)
template <typename PointSource, typename PointTarget>
class CorrespondenceEstimationBase : public PCLBase<PointSource> {
 public:
  using Ptr = std::shared_ptr<CorrespondenceEstimationBase<PointSource, PointTarget>>;
  using KdTree = search::KdTree<PointTarget>;
  using KdTreePtr = typename KdTree::Ptr;
  using PointCloudSourceConstPtr = typename PointCloud<PointSource>::ConstPtr;
  using PointCloudTargetConstPtr = typename PointCloud<PointTarget>::ConstPtr;
  void setInputSource(const PointCloudSourceConstPtr& cloud) { source_cloud_updated_ = true; PCLBase<PointSource>::setInputCloud(cloud); }
  PointCloudSourceConstPtr getInputSource() { return this->input_; }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) {  // impl/correspondence_estimation.hpp:53-69
    if (!cloud || cloud->points.empty()) return;
    target_ = cloud;
    target_cloud_updated_ = true;
  }
  PointCloudTargetConstPtr getInputTarget() { return target_; }
  void setIndicesSource(const IndicesPtr& indices) { this->setIndices(indices); source_cloud_updated_ = true; }
  IndicesPtr getIndicesSource() { return this->indices_; }
  void setIndicesTarget(const IndicesPtr& indices) { target_cloud_updated_ = true; target_indices_ = indices; }
  IndicesPtr getIndicesTarget() { return target_indices_; }
  void setSearchMethodTarget(const KdTreePtr& tree, bool force_no_recompute = false) {
    tree_ = tree;
    force_no_recompute_ = force_no_recompute;
    target_cloud_updated_ = true;
  }
  KdTreePtr getSearchMethodTarget() const { return tree_; }
  // correspondence_estimation.h:230-262: the reciprocal search's tree over the source.  The device builds its own index of
  // the (moving) source every iteration, so a tree handed in here is kept for the getter only.
  using KdTreeReciprocal = search::KdTree<PointSource>;
  using KdTreeReciprocalPtr = typename KdTreeReciprocal::Ptr;
  void setSearchMethodSource(const KdTreeReciprocalPtr& tree, bool force_no_recompute = false) {
    tree_reciprocal_ = tree;
    force_no_recompute_reciprocal_ = force_no_recompute;
    source_cloud_updated_ = true;
  }
  KdTreeReciprocalPtr getSearchMethodSource() const { return tree_reciprocal_; }
  // :111-131: estimators that need normals say so; the nearest-neighbour estimator does not
  virtual bool requiresSourceNormals() const { return false; }
  virtual bool requiresTargetNormals() const { return false; }
  // :144-155 (OpenMP threads of the host loop): one device launch covers all points
  void setNumberOfThreads(unsigned int nr_threads) { num_threads_ = nr_threads; }
  virtual void determineCorrespondences(Correspondences& correspondences,
                                        double max_distance = std::numeric_limits<double>::max()) = 0;
  virtual void determineReciprocalCorrespondences(Correspondences& correspondences,
                                                  double max_distance = std::numeric_limits<double>::max()) = 0;
  virtual Ptr clone() const = 0;
 protected:
  KdTreePtr tree_;
  PointCloudTargetConstPtr target_;
  IndicesPtr target_indices_;
  KdTreeReciprocalPtr tree_reciprocal_;
  bool target_cloud_updated_ = true, source_cloud_updated_ = true, force_no_recompute_ = false;
  bool force_no_recompute_reciprocal_ = false;
  unsigned int num_threads_ = 1;
  bool initCompute() {  // impl/correspondence_estimation.hpp:71-97
    if (!target_ || !tree_) return false;
    if (target_cloud_updated_ && !force_no_recompute_) {
      if (!(target_indices_ ? tree_->setInputCloud(target_, target_indices_) : tree_->setInputCloud(target_))) return false;
      target_cloud_updated_ = false;
    }
    return PCLBase<PointSource>::initCompute();
  }
};

// pcl::registration::CorrespondenceEstimation: all source points in one launch
template <typename PointSource, typename PointTarget>
class CorrespondenceEstimation : public CorrespondenceEstimationBase<PointSource, PointTarget> {
  using Base = CorrespondenceEstimationBase<PointSource, PointTarget>;
 public:
  using Ptr = std::shared_ptr<CorrespondenceEstimation<PointSource, PointTarget>>;
  CorrespondenceEstimation() : CorrespondenceEstimation(Context::defaultContext()) {}
  explicit CorrespondenceEstimation(Context::Ptr ctx) : ctx_(std::move(ctx)) { this->tree_ = std::make_shared<search::KdTree<PointTarget>>(ctx_); }
  CorrespondenceEstimation(const CorrespondenceEstimation& o) : Base(o), ctx_(o.ctx_) {}  // the device handle is not shared
  ~CorrespondenceEstimation() override { if (icp_) pclhip_icp_destroy(icp_); }
  void determineCorrespondences(Correspondences& out, double max_distance = std::numeric_limits<double>::max()) override {
    run(out, max_distance, false);
  }
  void determineReciprocalCorrespondences(Correspondences& out, double max_distance = std::numeric_limits<double>::max()) override {
    run(out, max_distance, true);
  }
  typename Base::Ptr clone() const override { return std::make_shared<CorrespondenceEstimation<PointSource, PointTarget>>(*this); }
 private:
  void run(Correspondences& out, double max_distance, bool reciprocal) {
    out.clear();
    if (!this->initCompute() || this->tree_->handle() == nullptr) return;
    if (icp_ && icp_target_ != this->tree_->handle()) { pclhip_icp_destroy(icp_); icp_ = nullptr; }
    if (!icp_) {
      if (pclhip_icp_create(this->tree_->handle(), &icp_) != PCLHIP_OK) return;
      icp_target_ = this->tree_->handle();
    }
    const bool subset = !this->usesAllPoints();
    static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double sums[PCLHIP_ICP_NSUMS];
    const double md = max_distance < 1e150 ? max_distance : 1e150;  // its square must stay finite
    if (pclhip_icp_set_source_indexed(icp_, this->input_->points.data(), sizeof(PointSource), this->input_->size(),
                                      subset ? this->indices_->data() : nullptr, subset ? this->indices_->size() : 0) == PCLHIP_OK &&
        pclhip_icp_set_reciprocal(icp_, reciprocal ? 1 : 0) == PCLHIP_OK &&
        pclhip_icp_iterate(icp_, I, md, PCLHIP_ICP_POINT_TO_POINT, sums) == PCLHIP_OK) {
      const std::size_t n = this->input_->size();
      std::uint64_t cnt = 0;
      if (!subset && sizeof(Correspondence) == 12) {  // the records compacted on the device, one copy
        out.resize(n);
        if (pclhip_icp_fetch_correspondence_records(icp_, out.data(), n, &cnt) == PCLHIP_OK) {
          out.resize(std::size_t(cnt));
          return;
        }
        out.clear();
      }
      Indices q(n), m(n);
      std::vector<float> d(n);
      if (pclhip_icp_fetch_correspondences(icp_, q.data(), m.data(), d.data(), &cnt) == PCLHIP_OK) {
        out.resize(std::size_t(cnt));
        for (std::uint64_t i = 0; i < cnt; ++i) out[std::size_t(i)] = Correspondence(q[std::size_t(i)], m[std::size_t(i)], d[std::size_t(i)]);
      }
    }
  }
  Context::Ptr ctx_;
  pclhip_icp* icp_ = nullptr;
  pclhip_index* icp_target_ = nullptr;
};

}  // namespace registration

// pcl::Registration<PointSource, PointTarget> (registration/include/pcl/registration/registration.h:56-700)
template <typename PointSource, typename PointTarget> class IterativeClosestPoint;

namespace registration {
// pcl::registration::DefaultConvergenceCriteria<Scalar> (default_convergence_criteria.h:61-286): the option holder a
// registration hands out through getConvergeCriteria(); hasConverged() itself runs on the device (closed_forms.hpp),
// its host twin is pclhip_convergence_has_converged.
class DefaultConvergenceCriteria {
 public:
  using Ptr = std::shared_ptr<DefaultConvergenceCriteria>;
  enum ConvergenceState {  // :73-81
    CONVERGENCE_CRITERIA_NOT_CONVERGED = 0,
    CONVERGENCE_CRITERIA_ITERATIONS = 1,
    CONVERGENCE_CRITERIA_TRANSFORM = 2,
    CONVERGENCE_CRITERIA_ABS_MSE = 3,
    CONVERGENCE_CRITERIA_REL_MSE = 4,
    CONVERGENCE_CRITERIA_NO_CORRESPONDENCES = 5,
    CONVERGENCE_CRITERIA_FAILURE_AFTER_MAX_ITERATIONS = 6
  };
  void setMaximumIterationsSimilarTransforms(int n) { max_iterations_similar_transforms_ = n; }
  int getMaximumIterationsSimilarTransforms() const { return max_iterations_similar_transforms_; }
  void setMaximumIterations(int n) { max_iterations_ = n; }
  int getMaximumIterations() const { return max_iterations_; }
  void setFailureAfterMaximumIterations(bool f) { failure_after_max_iter_ = f; }
  bool getFailureAfterMaximumIterations() const { return failure_after_max_iter_; }
  void setRotationThreshold(double t) { rotation_threshold_ = t; }
  double getRotationThreshold() const { return rotation_threshold_; }
  void setTranslationThreshold(double t) { translation_threshold_ = t; }
  double getTranslationThreshold() const { return translation_threshold_; }
  void setRelativeMSE(double m) { mse_threshold_relative_ = m; }
  double getRelativeMSE() const { return mse_threshold_relative_; }
  void setAbsoluteMSE(double m) { mse_threshold_absolute_ = m; }
  double getAbsoluteMSE() const { return mse_threshold_absolute_; }
  ConvergenceState getConvergenceState() const { return ConvergenceState(state_); }
  void setConvergenceState(ConvergenceState s) { state_ = int(s); }
 private:
  template <typename S, typename T> friend class ::pclhip::IterativeClosestPoint;
  int max_iterations_ = 100, max_iterations_similar_transforms_ = 0;  // :289-316
  bool failure_after_max_iter_ = false;
  double rotation_threshold_ = 0.99999, translation_threshold_ = 3e-4 * 3e-4;
  double mse_threshold_relative_ = 0.00001, mse_threshold_absolute_ = 1e-12;
  int state_ = 0;
};
}  // namespace registration

template <typename PointSource, typename PointTarget>
class Registration : public PCLBase<PointSource> {
 public:
  using Matrix4 = Matrix4f;
  using PointCloudSource = PointCloud<PointSource>;
  using PointCloudTarget = PointCloud<PointTarget>;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;
  using KdTree = search::KdTree<PointTarget>;
  using KdTreePtr = typename KdTree::Ptr;
  using PointRepresentationConstPtr = typename PointRepresentation<PointTarget>::ConstPtr;
  using TransformationEstimation = registration::TransformationEstimation<PointSource, PointTarget>;
  using TransformationEstimationPtr = typename TransformationEstimation::Ptr;
  using CorrespondenceEstimation = registration::CorrespondenceEstimationBase<PointSource, PointTarget>;
  using CorrespondenceEstimationPtr = typename CorrespondenceEstimation::Ptr;
  using CorrespondenceRejectorPtr = registration::CorrespondenceRejector::Ptr;

  explicit Registration(Context::Ptr ctx)
      : ctx_(std::move(ctx)), tree_(std::make_shared<KdTree>(ctx_)), correspondences_(std::make_shared<Correspondences>()) {}
  void setTransformationEstimation(const TransformationEstimationPtr& te) { transformation_estimation_ = te; }  // :144-148
  void setCorrespondenceEstimation(const CorrespondenceEstimationPtr& ce) { correspondence_estimation_ = ce; }  // :173-177
  virtual void setInputSource(const PointCloudSourceConstPtr& cloud) {  // impl/registration.hpp:45-56: every call counts
    if (!cloud || cloud->points.empty()) return;
    source_cloud_updated_ = true;
    PCLBase<PointSource>::setInputCloud(cloud);
  }
  PointCloudSourceConstPtr getInputSource() { return this->input_; }
  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) {  // :58-69
    if (!cloud || cloud->points.empty()) return;
    target_ = cloud;
    target_cloud_updated_ = true;
  }
  PointCloudTargetConstPtr getInputTarget() { return target_; }
  void setIndices(const IndicesPtr& indices) override { PCLBase<PointSource>::setIndices(indices); source_cloud_updated_ = true; }
  void setIndices(const IndicesConstPtr& indices) override { PCLBase<PointSource>::setIndices(indices); source_cloud_updated_ = true; }
  void setSearchMethodTarget(const KdTreePtr& tree, bool force_no_recompute = false) {  // :214-221
    tree_ = tree;
    force_no_recompute_ = force_no_recompute;
    target_cloud_updated_ = true;
  }
  KdTreePtr getSearchMethodTarget() const { return tree_; }
  // registration.h:230-262 (the reciprocal search's source tree; see CorrespondenceEstimationBase::setSearchMethodSource)
  using KdTreeReciprocal = search::KdTree<PointSource>;
  using KdTreeReciprocalPtr = typename KdTreeReciprocal::Ptr;
  void setSearchMethodSource(const KdTreeReciprocalPtr& tree, bool force_no_recompute = false) {
    tree_reciprocal_ = tree;
    force_no_recompute_reciprocal_ = force_no_recompute;
    source_cloud_updated_ = true;
  }
  KdTreeReciprocalPtr getSearchMethodSource() const { return tree_reciprocal_; }
  // :300-322: RANSAC refinement parameters; IterativeClosestPoint does not use them (nor does the reference's)
  void setRANSACIterations(int n) { ransac_iterations_ = n; }
  double getRANSACIterations() const { return ransac_iterations_; }
  void setRANSACOutlierRejectionThreshold(double t) { inlier_threshold_ = t; }
  double getRANSACOutlierRejectionThreshold() const { return inlier_threshold_; }
  Matrix4 getFinalTransformation() { return final_transformation_; }
  Matrix4 getLastIncrementalTransformation() { return transformation_; }
  void setMaximumIterations(int nr_iterations) { max_iterations_ = nr_iterations; }
  int getMaximumIterations() const { return max_iterations_; }
  void setMaxCorrespondenceDistance(double d) { corr_dist_threshold_ = d; }
  double getMaxCorrespondenceDistance() const { return corr_dist_threshold_; }
  void setTransformationEpsilon(double e) { transformation_epsilon_ = e; }
  double getTransformationEpsilon() const { return transformation_epsilon_; }
  void setTransformationRotationEpsilon(double e) { transformation_rotation_epsilon_ = e; }
  double getTransformationRotationEpsilon() const { return transformation_rotation_epsilon_; }
  void setEuclideanFitnessEpsilon(double e) { euclidean_fitness_epsilon_ = e; }
  double getEuclideanFitnessEpsilon() const { return euclidean_fitness_epsilon_; }
  void setPointRepresentation(const PointRepresentationConstPtr& rep) { point_representation_ = rep; }  // :422
  void addCorrespondenceRejector(const CorrespondenceRejectorPtr& r) { correspondence_rejectors_.push_back(r); }  // :518-547
  std::vector<CorrespondenceRejectorPtr> getCorrespondenceRejectors() { return correspondence_rejectors_; }
  bool removeCorrespondenceRejector(unsigned int i) {
    if (i >= correspondence_rejectors_.size()) return false;
    correspondence_rejectors_.erase(correspondence_rejectors_.begin() + i);
    return true;
  }
  void clearCorrespondenceRejectors() { correspondence_rejectors_.clear(); }
  bool hasConverged() const { return converged_; }
  const std::string& getClassName() const { return reg_name_; }
  std::string getLastError() const { return ctx_->getLastError(); }

  void align(PointCloudSource& output) { align(output, Matrix4::Identity()); }
  void align(PointCloudSource& output, const Matrix4& guess) {  // impl/registration.hpp:178-221
    converged_ = false;
    if (!initCompute()) return;
    output.points.resize(this->indices_->size());
    for (std::size_t i = 0; i < this->indices_->size(); ++i) output[i] = (*this->input_)[std::size_t((*this->indices_)[i])];
    output.width = std::uint32_t(output.size());
    output.height = 1;
    output.is_dense = this->input_->is_dense;
    if (point_representation_ && !force_no_recompute_) tree_->setPointRepresentation(point_representation_);
    final_transformation_ = transformation_ = Matrix4::Identity();
    computeTransformation(output, guess);
  }
  virtual double getFitnessScore(double max_range = std::numeric_limits<double>::max()) = 0;

 protected:
  bool initCompute() {  // impl/registration.hpp:73-101
    if (!ctx_ || !ctx_->ok() || !this->input_ || !tree_) return false;
    if (target_cloud_updated_ && !(force_no_recompute_ && tree_->handle())) {
      if (!target_ || !tree_->setInputCloud(target_)) return false;
      target_built_ = true;
    }
    target_cloud_updated_ = false;
    if (!tree_->handle()) return false;
    if (correspondence_estimation_) correspondence_estimation_->setSearchMethodTarget(tree_, true);
    return PCLBase<PointSource>::initCompute();
  }
  virtual void computeTransformation(PointCloudSource& output, const Matrix4& guess) = 0;  // :678-679

  Context::Ptr ctx_;
  std::string reg_name_;
  KdTreePtr tree_;
  PointCloudTargetConstPtr target_;
  int nr_iterations_ = 0, max_iterations_ = 10;
  Matrix4 final_transformation_, transformation_;
  double transformation_epsilon_ = 0.0, transformation_rotation_epsilon_ = 0.0;
  double euclidean_fitness_epsilon_ = -std::numeric_limits<double>::max();
  double corr_dist_threshold_ = std::sqrt(std::numeric_limits<double>::max());
  bool converged_ = false;
  int min_number_correspondences_ = 3;
  CorrespondencesPtr correspondences_;
  TransformationEstimationPtr transformation_estimation_;
  CorrespondenceEstimationPtr correspondence_estimation_;
  std::vector<CorrespondenceRejectorPtr> correspondence_rejectors_;
  PointRepresentationConstPtr point_representation_;
  bool target_cloud_updated_ = true, source_cloud_updated_ = true, force_no_recompute_ = false;
  bool target_built_ = false;  // the tree was (re)built by this object since the device handle was last refreshed
  KdTreeReciprocalPtr tree_reciprocal_;
  bool force_no_recompute_reciprocal_ = false;
  int ransac_iterations_ = 0;       // registration.h:570
  double inlier_threshold_ = 0.05;  // :600
};

// pcl::IterativeClosestPoint<PointSource, PointTarget> (icp.h:98-347)
template <typename PointSource, typename PointTarget>
class IterativeClosestPoint : public Registration<PointSource, PointTarget> {
  using Base = Registration<PointSource, PointTarget>;
 public:
  using PointCloudSource = typename Base::PointCloudSource;
  using Matrix4 = typename Base::Matrix4;
  using Ptr = std::shared_ptr<IterativeClosestPoint<PointSource, PointTarget>>;
  IterativeClosestPoint() : IterativeClosestPoint(Context::defaultContext()) {}
  explicit IterativeClosestPoint(Context::Ptr ctx) : Base(std::move(ctx)) {  // icp.h:136-151
    this->reg_name_ = "IterativeClosestPoint";
    this->transformation_estimation_ = std::make_shared<registration::TransformationEstimationSVD<PointSource, PointTarget>>(this->ctx_);
    this->correspondence_estimation_ = std::make_shared<registration::CorrespondenceEstimation<PointSource, PointTarget>>(this->ctx_);
    convergence_criteria_ = std::make_shared<registration::DefaultConvergenceCriteria>();  // icp.h:144-146
    pclhip_convergence_init(&criteria_);
  }
  ~IterativeClosestPoint() override { if (icp_) pclhip_icp_destroy(icp_); }
  IterativeClosestPoint(const IterativeClosestPoint&) = delete;             // icp.h:168-173
  IterativeClosestPoint& operator=(const IterativeClosestPoint&) = delete;

  void setUseReciprocalCorrespondences(bool on) { use_reciprocal_correspondence_ = on; }  // icp.h:251-256
  bool getUseReciprocalCorrespondences() const { return use_reciprocal_correspondence_; }
  // icp.h:180-184: the criteria object; its similar-transforms count, failure-after-max-iterations flag and absolute MSE
  // threshold are the options a caller sets there (the other thresholds are overwritten from the registration's own
  // setters at every align(), impl/icp.hpp:157-161)
  registration::DefaultConvergenceCriteria::Ptr getConvergeCriteria() { return convergence_criteria_; }
  // shortcuts for the same three options
  void setMaximumIterationsSimilarTransforms(int n) { convergence_criteria_->setMaximumIterationsSimilarTransforms(n); }
  void setFailureAfterMaximumIterations(bool f) { convergence_criteria_->setFailureAfterMaximumIterations(f); }
  void setAbsoluteMSE(double mse) { convergence_criteria_->setAbsoluteMSE(mse); }
  int getNumberOfIterations() const { return this->nr_iterations_; }
  int getConvergenceState() const { return criteria_.convergence_state; }
  double getLastMSE() const { return last_mse_; }
  // true when the last align() ran the fused device loop, false when it went through the virtual calls
  bool ranOnDeviceLoop() const { return device_loop_; }

  // Registration::getFitnessScore (registration/include/pcl/registration/impl/registration.hpp:132-168)
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    if (!this->initCompute() || !ensureHandle(modeOfEstimator() >= 0 ? modeOfEstimator() : PCLHIP_ICP_POINT_TO_POINT))
      return std::numeric_limits<double>::max();
    double score = std::numeric_limits<double>::max();
    pclhip_icp_fitness_score(icp_, this->final_transformation_.m, max_range, &score, nullptr);
    return score;
  }

 protected:
  virtual bool enforceSameDirectionNormals() const { return true; }
  // which stock estimator is plugged in (its device mode), or -1 for a foreign one
  int modeOfEstimator() const {
    using namespace registration;
    const auto* te = this->transformation_estimation_.get();
    if (te == nullptr) return -1;
    // exactly the stock classes: a subclass that overrides them is a foreign estimator like any other
    if (typeid(*te) == typeid(TransformationEstimationSymmetricPointToPlaneLLS<PointSource, PointTarget>)) return PCLHIP_ICP_SYMMETRIC;
    if (typeid(*te) == typeid(TransformationEstimationPointToPlaneLLS<PointSource, PointTarget>)) return PCLHIP_ICP_POINT_TO_PLANE;
    if (typeid(*te) == typeid(TransformationEstimationSVD<PointSource, PointTarget>)) return PCLHIP_ICP_POINT_TO_POINT;
    return -1;
  }
  void fillParams(pclhip_icp_params& p, int mode) const {
    pclhip_icp_params_default(&p);
    p.mode = mode;
    p.max_iterations = this->max_iterations_;
    p.max_correspondence_distance = this->corr_dist_threshold_;
    p.transformation_epsilon = this->transformation_epsilon_;
    p.transformation_rotation_epsilon = this->transformation_rotation_epsilon_;
    p.euclidean_fitness_epsilon = this->euclidean_fitness_epsilon_;
    p.min_number_correspondences = this->min_number_correspondences_;
    auto& cc = *convergence_criteria_;
    p.failure_after_max_iterations = cc.getFailureAfterMaximumIterations() ? 1 : 0;
    p.max_iterations_similar_transforms = cc.getMaximumIterationsSimilarTransforms();
    p.mse_threshold_absolute = cc.getAbsoluteMSE();
    // impl/icp.hpp:157-161: what the loop pushes into the criteria before it starts
    cc.setMaximumIterations(this->max_iterations_);
    cc.setRelativeMSE(this->euclidean_fitness_epsilon_);
    cc.setTranslationThreshold(this->transformation_epsilon_);
    if (this->transformation_rotation_epsilon_ > 0) cc.setRotationThreshold(this->transformation_rotation_epsilon_);
    else cc.setRotationThreshold(0.99999);
  }
  // device-side registration object bound to the tree; source (and normals) uploaded when they changed
  bool ensureHandle(int mode) {
    pclhip_index* ix = this->tree_->handle();
    if (icp_ && (icp_target_ != ix || this->target_built_)) { pclhip_icp_destroy(icp_); icp_ = nullptr; }
    if (mode != PCLHIP_ICP_POINT_TO_POINT && has_normal_fields<PointTarget>() && this->target_ &&
        (this->target_built_ || normals_of_ != this->target_.get())) {  // pcl::PointNormal target: normals at +16
      const char* base = reinterpret_cast<const char*>(this->target_->points.data());
      if (pclhip_index_set_normals(ix, base + 16, sizeof(PointTarget)) != PCLHIP_OK) return false;
      normals_of_ = this->target_.get();
    }
    this->target_built_ = false;
    if (!icp_) {
      if (pclhip_icp_create(ix, &icp_) != PCLHIP_OK) return false;
      icp_target_ = ix;
      this->source_cloud_updated_ = true;
    }
    if (this->source_cloud_updated_) {
      const bool subset = !this->usesAllPoints();
      if (pclhip_icp_set_source_indexed(icp_, this->input_->points.data(), sizeof(PointSource), this->input_->size(),
                                        subset ? this->indices_->data() : nullptr, subset ? this->indices_->size() : 0) != PCLHIP_OK)
        return false;
      if (has_normal_fields<PointSource>()) {  // pcl::PointNormal source: its normals feed the symmetric objective
        const char* base = reinterpret_cast<const char*>(this->input_->points.data());
        if (pclhip_icp_set_source_normals(icp_, base + 16, sizeof(PointSource)) != PCLHIP_OK) return false;
      }
      this->source_cloud_updated_ = false;
    }
    std::vector<pclhip_rejector> list;
    for (const auto& r : this->correspondence_rejectors_) list.push_back(r->desc);
    return pclhip_icp_set_rejectors(icp_, list.data(), int(list.size())) == PCLHIP_OK &&
           pclhip_icp_set_reciprocal(icp_, use_reciprocal_correspondence_ ? 1 : 0) == PCLHIP_OK &&
           pclhip_icp_set_enforce_same_direction_normals(icp_, enforceSameDirectionNormals() ? 1 : 0) == PCLHIP_OK;
  }
  // IterativeClosestPoint::transformCloud (impl/icp.hpp:49-111), in place on a host cloud
  virtual void transformCloud(PointCloudSource& cloud, const Matrix4& T, int mode) {
    pclhip_transform_cloud(this->ctx_->get(), T.m, mode == PCLHIP_ICP_POINT_TO_POINT ? 0 : 1, cloud.points.data(),
                           cloud.points.data(), sizeof(PointSource), cloud.size(),
                           (mode != PCLHIP_ICP_POINT_TO_POINT && has_normal_fields<PointSource>()) ? 16 : 0);
  }

  void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {  // impl/icp.hpp:113-268
    using namespace registration;
    const int mode = modeOfEstimator();
    const auto* cep = this->correspondence_estimation_.get();
    const bool own_ce = cep != nullptr && typeid(*cep) == typeid(registration::CorrespondenceEstimation<PointSource, PointTarget>);
    device_loop_ = mode >= 0 && own_ce && this->tree_->hasDefaultRepresentation();
    if (device_loop_) {
      if (!ensureHandle(mode)) return;
      pclhip_icp_params p;
      fillParams(p, mode);
      pclhip_icp_result r;
      if (pclhip_icp_align(icp_, &p, guess.m, &r) != PCLHIP_OK) return;
      if (r.nr_iterations > 0 || r.num_correspondences > 0)
        for (const auto& rej : this->correspondence_rejectors_) rej->readBack(icp_);
      std::memcpy(this->final_transformation_.m, r.final_transformation, sizeof r.final_transformation);
      std::memcpy(this->transformation_.m, r.last_transformation, sizeof r.last_transformation);
      this->converged_ = r.converged != 0;
      this->nr_iterations_ = r.nr_iterations;
      criteria_.convergence_state = r.convergence_state;
      convergence_criteria_->setConvergenceState(registration::DefaultConvergenceCriteria::ConvergenceState(r.convergence_state));
      last_mse_ = r.mse;
      output = *this->input_;  // icp.hpp:264-267: all fields of the WHOLE input cloud, then xyz (+ normals) moved
      transformCloud(output, this->final_transformation_, mode);
      return;
    }
    // ---- a foreign estimator is plugged in: PCL's loop, through the virtual interfaces -------------------
    if (!this->target_ || !this->transformation_estimation_ || !this->correspondence_estimation_) return;
    const int tmode = mode >= 0 ? mode : (has_normal_fields<PointSource>() ? PCLHIP_ICP_POINT_TO_PLANE : PCLHIP_ICP_POINT_TO_POINT);
    auto moved = std::make_shared<PointCloudSource>(output);  // input_transformed (:120-131), the indexed subset
    this->nr_iterations_ = 0;
    this->converged_ = false;
    this->final_transformation_ = guess;
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && guess.m[i] == Matrix4().m[i];
    if (!identity) transformCloud(*moved, guess, tmode);
    this->transformation_ = Matrix4::Identity();
    auto& ce = *this->correspondence_estimation_;
    ce.setInputTarget(this->target_);  // :145 (the tree itself was handed over in initCompute)
    ce.setSearchMethodTarget(this->tree_, true);
    pclhip_icp_params p;
    fillParams(p, tmode);
    if (!this->correspondence_rejectors_.empty()) return;  // the rejectors here are device-side parameter holders
    do {
      ce.setInputSource(moved);  // :178
      if (use_reciprocal_correspondence_) ce.determineReciprocalCorrespondences(*this->correspondences_, this->corr_dist_threshold_);
      else ce.determineCorrespondences(*this->correspondences_, this->corr_dist_threshold_);
      const std::size_t cnt = this->correspondences_->size();
      if (int(cnt) < this->min_number_correspondences_) {  // :204-213
        criteria_.convergence_state = 5;  // CONVERGENCE_CRITERIA_NO_CORRESPONDENCES
        this->converged_ = false;
        break;
      }
      this->transformation_estimation_->estimateRigidTransformation(*moved, *this->target_, *this->correspondences_,
                                                                    this->transformation_);  // :216-217
      transformCloud(*moved, this->transformation_, tmode);                                     // :220
      this->final_transformation_ = this->transformation_ * this->final_transformation_;        // :223
      ++this->nr_iterations_;
      double mse = 0.0;  // calculateMSE, default_convergence_criteria.h:262-270
      for (const Correspondence& c : *this->correspondences_) mse += double(c.distance);
      mse /= double(cnt);
      last_mse_ = mse;
      this->converged_ = pclhip_convergence_has_converged(&p, &criteria_, this->nr_iterations_, this->transformation_.m, mse) != 0;
    } while (criteria_.convergence_state == 0);
    convergence_criteria_->setConvergenceState(registration::DefaultConvergenceCriteria::ConvergenceState(criteria_.convergence_state));
    output = *this->input_;
    transformCloud(output, this->final_transformation_, tmode);
  }

  bool use_reciprocal_correspondence_ = false;
  registration::DefaultConvergenceCriteria::Ptr convergence_criteria_;
  pclhip_convergence_state criteria_;
  double last_mse_ = 0;
  bool device_loop_ = false;
  pclhip_icp* icp_ = nullptr;
  pclhip_index* icp_target_ = nullptr;
  const void* normals_of_ = nullptr;
};

// pcl::IterativeClosestPointWithNormals (icp.h:360-440)
template <typename PointSource, typename PointTarget>
class IterativeClosestPointWithNormals : public IterativeClosestPoint<PointSource, PointTarget> {
 public:
  using Ptr = std::shared_ptr<IterativeClosestPointWithNormals<PointSource, PointTarget>>;
  IterativeClosestPointWithNormals() : IterativeClosestPointWithNormals(Context::defaultContext()) {}
  explicit IterativeClosestPointWithNormals(Context::Ptr ctx) : IterativeClosestPoint<PointSource, PointTarget>(std::move(ctx)) {
    this->reg_name_ = "IterativeClosestPointWithNormals";
    setUseSymmetricObjective(false);
  }
  void setUseSymmetricObjective(bool on) {  // icp.h:380-400
    use_symmetric_objective_ = on;
    if (on) {
      auto te = std::make_shared<registration::TransformationEstimationSymmetricPointToPlaneLLS<PointSource, PointTarget>>(this->ctx_);
      te->setEnforceSameDirectionNormals(enforce_same_direction_normals_);
      this->transformation_estimation_ = te;
    } else {
      this->transformation_estimation_ =
          std::make_shared<registration::TransformationEstimationPointToPlaneLLS<PointSource, PointTarget>>(this->ctx_);
    }
  }
  bool getUseSymmetricObjective() const { return use_symmetric_objective_; }
  void setEnforceSameDirectionNormals(bool on) {  // icp.h:416-428
    enforce_same_direction_normals_ = on;
    if (use_symmetric_objective_) setUseSymmetricObjective(true);
  }
  bool getEnforceSameDirectionNormals() const { return enforce_same_direction_normals_; }
 protected:
  bool enforceSameDirectionNormals() const override { return enforce_same_direction_normals_; }
  bool use_symmetric_objective_ = false, enforce_same_direction_normals_ = true;
};

// pcl::GeneralizedIterativeClosestPoint<PointSource, PointTarget> with the Newton solver (registration/include/pcl/
// registration/gicp.h, impl/gicp.hpp:370-477, 768-933) on the C ABI's pclhip_gicp: covariances computed by the first
// align() and cached (setInputSource drops the source's, setInputTarget the target's), or the caller's.  useBFGS, source
// subsets (setIndices) are refused with std::logic_error.
template <typename PointSource, typename PointTarget>
class GeneralizedIterativeClosestPoint : public IterativeClosestPoint<PointSource, PointTarget> {
  using Base = IterativeClosestPoint<PointSource, PointTarget>;
 public:
  using PointCloudSource = typename Base::PointCloudSource;
  using Matrix4 = typename Base::Matrix4;
  using PointCloudSourceConstPtr = typename Registration<PointSource, PointTarget>::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Registration<PointSource, PointTarget>::PointCloudTargetConstPtr;
  using MatricesVector = std::vector<std::array<double, 9>>;  // gicp.h:104 (Eigen::Matrix3d each; row-major here)
  using MatricesVectorPtr = std::shared_ptr<MatricesVector>;
  using Ptr = std::shared_ptr<GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
  GeneralizedIterativeClosestPoint() : GeneralizedIterativeClosestPoint(Context::defaultContext()) {}
  explicit GeneralizedIterativeClosestPoint(Context::Ptr ctx) : Base(std::move(ctx)) {  // gicp.h:136-152
    this->reg_name_ = "GeneralizedIterativeClosestPoint";
    pclhip_gicp_params_default(&p_);
    this->max_iterations_ = p_.max_iterations;
    this->transformation_epsilon_ = p_.transformation_epsilon;
    this->corr_dist_threshold_ = p_.max_correspondence_distance;
    this->min_number_correspondences_ = p_.min_number_correspondences;
  }
  ~GeneralizedIterativeClosestPoint() override { if (gicp_) pclhip_gicp_destroy(gicp_); }

  void setInputSource(const PointCloudSourceConstPtr& cloud) override {  // gicp.h:160-166
    src_cov_.reset();
    Base::setInputSource(cloud);
  }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {  // gicp.h:174-180
    tgt_cov_.reset();
    if (gicp_) { pclhip_gicp_destroy(gicp_); gicp_ = nullptr; }
    Base::setInputTarget(cloud);
  }
  void setSourceCovariances(const MatricesVectorPtr& c) { src_cov_ = c; src_cov_dirty_ = true; }  // gicp.h:184-199
  void setTargetCovariances(const MatricesVectorPtr& c) { tgt_cov_ = c; tgt_cov_dirty_ = true; }  // :201-215
  void setIndices(const IndicesPtr& indices) override { refuseIndices(indices != nullptr); }
  void setIndices(const IndicesConstPtr& indices) override { refuseIndices(indices != nullptr); }
  void useBFGS() { throw std::logic_error("GeneralizedIterativeClosestPoint: the BFGS solver is not supported (Newton only)"); }
  // gicp.h:386-431
  void setRotationEpsilon(double e) { p_.rotation_epsilon = e; }
  double getRotationEpsilon() const { return p_.rotation_epsilon; }
  void setCorrespondenceRandomness(int k) { p_.k_correspondences = k; }
  int getCorrespondenceRandomness() const { return p_.k_correspondences; }
  void setMaximumOptimizerIterations(int n) { p_.max_inner_iterations = n; }
  int getMaximumOptimizerIterations() const { return p_.max_inner_iterations; }
  void setTranslationGradientTolerance(double t) { p_.translation_gradient_tolerance = t; }
  double getTranslationGradientTolerance() const { return p_.translation_gradient_tolerance; }
  void setRotationGradientTolerance(double t) { p_.rotation_gradient_tolerance = t; }
  double getRotationGradientTolerance() const { return p_.rotation_gradient_tolerance; }
  // the last alignment's record: Newton iterations, passes, covariance time
  const pclhip_gicp_result& lastResult() const { return result_; }

  // Registration::getFitnessScore (impl/registration.hpp:132-168)
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    double score = std::numeric_limits<double>::max();
    if (!this->initCompute() || !ensureGicp()) return score;
    pclhip_gicp_fitness_score(gicp_, this->final_transformation_.m, max_range, &score, nullptr);
    return score;
  }

 protected:
  void refuseIndices(bool given) {
    if (given) throw std::logic_error("GeneralizedIterativeClosestPoint: source subsets (setIndices) are not supported");
  }
  bool ensureGicp() {
    pclhip_index* ix = this->tree_->handle();
    if (gicp_ && (gicp_target_ != ix || this->target_built_)) { pclhip_gicp_destroy(gicp_); gicp_ = nullptr; }
    this->target_built_ = false;
    if (!gicp_) {
      if (pclhip_gicp_create(ix, &gicp_) != PCLHIP_OK) return false;
      gicp_target_ = ix;
      this->source_cloud_updated_ = true;
      tgt_cov_dirty_ = tgt_cov_ != nullptr;
    }
    if (this->source_cloud_updated_) {
      if (pclhip_gicp_set_source(gicp_, this->input_->points.data(), sizeof(PointSource), this->input_->size()) != PCLHIP_OK)
        return false;
      this->source_cloud_updated_ = false;
      src_cov_dirty_ = src_cov_ != nullptr;
    }
    if (src_cov_dirty_ && src_cov_) {
      if (pclhip_gicp_set_source_covariances(gicp_, src_cov_->front().data(), src_cov_->size()) != PCLHIP_OK) return false;
      src_cov_dirty_ = false;
    }
    if (tgt_cov_dirty_ && tgt_cov_) {
      if (pclhip_gicp_set_target_covariances(gicp_, tgt_cov_->front().data(), tgt_cov_->size()) != PCLHIP_OK) return false;
      tgt_cov_dirty_ = false;
    }
    return true;
  }
  void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {  // impl/gicp.hpp:768-930
    this->converged_ = false;
    if (!ensureGicp()) return;
    p_.max_iterations = this->max_iterations_;
    p_.transformation_epsilon = this->transformation_epsilon_;
    p_.max_correspondence_distance = this->corr_dist_threshold_;
    p_.min_number_correspondences = this->min_number_correspondences_;
    if (pclhip_gicp_align(gicp_, &p_, guess.m, &result_) != PCLHIP_OK) return;
    std::memcpy(this->final_transformation_.m, result_.final_transformation, sizeof result_.final_transformation);
    std::memcpy(this->transformation_.m, result_.last_transformation, sizeof result_.last_transformation);
    this->converged_ = result_.converged != 0;
    this->nr_iterations_ = result_.nr_iterations;
    output = *this->input_;  // :929: transformPointCloud(*input_, output, final_transformation_)
    pclhip_transform_cloud(this->ctx_->get(), this->final_transformation_.m, 1, output.points.data(), output.points.data(),
                           sizeof(PointSource), output.size(), 0);
  }

  pclhip_gicp_params p_;
  pclhip_gicp_result result_ = {};
  pclhip_gicp* gicp_ = nullptr;
  pclhip_index* gicp_target_ = nullptr;
  MatricesVectorPtr src_cov_, tgt_cov_;
  bool src_cov_dirty_ = false, tgt_cov_dirty_ = false;
};

// pcl::NormalDistributionsTransform<PointSource, PointTarget> (registration/include/pcl/registration/ndt.h, impl/ndt.hpp)
// on the C ABI's pclhip_ndt: the voxel Gaussians of the target are built by the first align() and cached until the target,
// the resolution or the minimum points per voxel changes.  Only NeighborSearchMethod::RADIUS (the reference's default) is
// built; the DIRECT neighbourhoods and source subsets (setIndices) are refused with std::logic_error.
enum class NeighborSearchMethod { RADIUS, DIRECT27, DIRECT26, DIRECT7, DIRECT1 };  // ndt.h:59-65

template <typename PointSource, typename PointTarget>
class NormalDistributionsTransform : public Registration<PointSource, PointTarget> {
  using Base = Registration<PointSource, PointTarget>;
 public:
  using PointCloudSource = typename Base::PointCloudSource;
  using Matrix4 = typename Base::Matrix4;
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
  using Ptr = std::shared_ptr<NormalDistributionsTransform<PointSource, PointTarget>>;
  NormalDistributionsTransform() : NormalDistributionsTransform(Context::defaultContext()) {}
  explicit NormalDistributionsTransform(Context::Ptr ctx) : Base(std::move(ctx)) {  // impl/ndt.hpp:68-77
    this->reg_name_ = "NormalDistributionsTransform";
    pclhip_ndt_params_default(&p_);
    this->transformation_epsilon_ = p_.transformation_epsilon;
    this->max_iterations_ = p_.max_iterations;
  }
  ~NormalDistributionsTransform() override { if (ndt_) pclhip_ndt_destroy(ndt_); }

  void setInputSource(const PointCloudSourceConstPtr& cloud) override { Base::setInputSource(cloud); source_dirty_ = true; }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override { Base::setInputTarget(cloud); target_dirty_ = true; }  // ndt.h:121-127
  void setIndices(const IndicesPtr& indices) override { refuseIndices(indices != nullptr); }
  void setIndices(const IndicesConstPtr& indices) override { refuseIndices(indices != nullptr); }
  void setResolution(float resolution) { p_.resolution = resolution; }  // ndt.h:133-141: the grid is rebuilt by the next align
  float getResolution() const { return p_.resolution; }
  void setMinPointPerVoxel(unsigned int n) { p_.min_points_per_voxel = int(n); }  // ndt.h:130
  void setStepSize(double step_size) { p_.step_size = step_size; }
  double getStepSize() const { return p_.step_size; }
  void setOutlierRatio(double r) { p_.outlier_ratio = r; }
  double getOutlierRatio() const { return p_.outlier_ratio; }
  void setNeighborhoodSearchMethod(NeighborSearchMethod method) {  // ndt.h:243-254
    if (method != NeighborSearchMethod::RADIUS)
      throw std::logic_error("NormalDistributionsTransform: the DIRECT27 / DIRECT26 / DIRECT7 / DIRECT1 neighbourhoods are "
                             "not supported (RADIUS only)");
  }
  NeighborSearchMethod getNeighborhoodSearchMethod() const { return NeighborSearchMethod::RADIUS; }
  void setNumberOfThreads(unsigned int) {}  // the OpenMP thread count of the reference's derivative loop: no effect
  double getTransformationLikelihood() const { return result_.transformation_likelihood; }
  double getTransformationProbability() const { return result_.transformation_likelihood; }
  int getFinalNumIteration() const { return this->nr_iterations_; }
  const pclhip_ndt_result& lastResult() const { return result_; }

  // Registration::getFitnessScore (impl/registration.hpp:132-168)
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    double score = std::numeric_limits<double>::max();
    if (!this->initCompute() || !ensureNdt()) return score;
    pclhip_ndt_fitness_score(ndt_, this->final_transformation_.m, max_range, &score, nullptr);
    return score;
  }

 protected:
  void refuseIndices(bool given) {
    if (given) throw std::logic_error("NormalDistributionsTransform: source subsets (setIndices) are not supported");
  }
  bool ensureNdt() {
    if (!ndt_ && pclhip_ndt_create(this->ctx_->get(), &ndt_) != PCLHIP_OK) return false;
    if (target_dirty_) {
      if (!this->target_ ||
          pclhip_ndt_set_target(ndt_, this->target_->points.data(), sizeof(PointTarget), this->target_->size()) != PCLHIP_OK)
        return false;
      target_dirty_ = false;
    }
    if (source_dirty_) {
      if (pclhip_ndt_set_source(ndt_, this->input_->points.data(), sizeof(PointSource), this->input_->size()) != PCLHIP_OK)
        return false;
      source_dirty_ = false;
    }
    return true;
  }
  void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {  // impl/ndt.hpp:79-207
    this->converged_ = false;
    this->nr_iterations_ = 0;
    if (!ensureNdt()) return;
    p_.max_iterations = this->max_iterations_;
    p_.transformation_epsilon = this->transformation_epsilon_;
    p_.transformation_rotation_epsilon = this->transformation_rotation_epsilon_;
    if (pclhip_ndt_align(ndt_, &p_, guess.m, &result_) != PCLHIP_OK) return;
    std::memcpy(this->final_transformation_.m, result_.final_transformation, sizeof result_.final_transformation);
    std::memcpy(this->transformation_.m, result_.last_transformation, sizeof result_.last_transformation);
    this->converged_ = result_.converged != 0;
    this->nr_iterations_ = result_.nr_iterations;
    output = *this->input_;  // the trial clouds are transformPointCloud(*input_, output, final_transformation_) (:841)
    pclhip_transform_cloud(this->ctx_->get(), this->final_transformation_.m, 1, output.points.data(), output.points.data(),
                           sizeof(PointSource), output.size(), 0);
  }

  pclhip_ndt_params p_;
  pclhip_ndt_result result_ = {};
  pclhip_ndt* ndt_ = nullptr;
  bool target_dirty_ = true, source_dirty_ = true;
};

// pcl::SampleConsensusPrerejective<PointSource, PointTarget, FeatureT> (registration/include/pcl/registration/
// sample_consensus_prerejective.h, impl/sample_consensus_prerejective.hpp:78-348) on the C ABI's pclhip_scp: FeatureT is a
// record of floats (pcl::FPFHSignature33).  The draws are a pure function of (seed, iteration, slot) (include/pclhip.h):
// setSeed.  An error of :161-212 leaves converged_ false, as the reference's early returns do; lastStatus() tells which.
template <typename PointSource, typename PointTarget, typename FeatureT>
class SampleConsensusPrerejective : public Registration<PointSource, PointTarget> {
  using Base = Registration<PointSource, PointTarget>;
  static_assert(sizeof(FeatureT) % sizeof(float) == 0 && sizeof(FeatureT) / sizeof(float) <= 64, "FeatureT: at most 64 floats");
 public:
  using PointCloudSource = typename Base::PointCloudSource;
  using Matrix4 = typename Base::Matrix4;
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
  using FeatureCloud = PointCloud<FeatureT>;
  using FeatureCloudConstPtr = std::shared_ptr<const FeatureCloud>;
  using Ptr = std::shared_ptr<SampleConsensusPrerejective<PointSource, PointTarget, FeatureT>>;
  SampleConsensusPrerejective() : SampleConsensusPrerejective(Context::defaultContext()) {}
  explicit SampleConsensusPrerejective(Context::Ptr ctx) : Base(std::move(ctx)) {  // sample_consensus_prerejective.h:121-131
    this->reg_name_ = "SampleConsensusPrerejective";
    pclhip_scp_params_default(&p_);
    this->max_iterations_ = p_.max_iterations;
  }
  ~SampleConsensusPrerejective() override { if (scp_) pclhip_scp_destroy(scp_); }

  void setSourceFeatures(const FeatureCloudConstPtr& features) { input_features_ = features; src_feat_dirty_ = true; }  // :140
  FeatureCloudConstPtr getSourceFeatures() const { return input_features_; }
  void setTargetFeatures(const FeatureCloudConstPtr& features) { target_features_ = features; tgt_feat_dirty_ = true; }  // :153
  FeatureCloudConstPtr getTargetFeatures() const { return target_features_; }
  void setIndices(const IndicesPtr& indices) override { refuseIndices(indices != nullptr); }
  void setIndices(const IndicesConstPtr& indices) override { refuseIndices(indices != nullptr); }
  void setNumberOfSamples(int nr_samples) { p_.nr_samples = nr_samples; }  // :166-194
  int getNumberOfSamples() const { return p_.nr_samples; }
  void setCorrespondenceRandomness(int k) { p_.k_correspondences = k; }
  int getCorrespondenceRandomness() const { return p_.k_correspondences; }
  void setSimilarityThreshold(float similarity_threshold) { p_.similarity_threshold = similarity_threshold; }  // :203-215
  float getSimilarityThreshold() const { return p_.similarity_threshold; }
  void setInlierFraction(float inlier_fraction) { p_.inlier_fraction = inlier_fraction; }  // :221-233
  float getInlierFraction() const { return p_.inlier_fraction; }
  void setSeed(std::uint64_t seed) { p_.seed = seed; }
  std::uint64_t getSeed() const { return p_.seed; }
  const Indices& getInliers() const { return inliers_; }  // :240
  const pclhip_scp_result& lastResult() const { return result_; }
  pclhip_status lastStatus() const { return status_; }

  // Registration::getFitnessScore (impl/registration.hpp:132-168)
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    double score = std::numeric_limits<double>::max();
    if (!this->initCompute() || !ensureScp()) return score;
    pclhip_scp_fitness_score(scp_, this->final_transformation_.m, max_range, &score, nullptr);
    return score;
  }

 protected:
  void refuseIndices(bool given) {
    if (given) throw std::logic_error("SampleConsensusPrerejective: source subsets (setIndices) are not supported");
  }
  bool ensureScp() {
    pclhip_index* ix = this->tree_->handle();
    if (scp_ && (scp_target_ != ix || this->target_built_)) { pclhip_scp_destroy(scp_); scp_ = nullptr; }
    this->target_built_ = false;
    if (!scp_) {
      if ((status_ = pclhip_scp_create(ix, &scp_)) != PCLHIP_OK) return false;
      scp_target_ = ix;
      this->source_cloud_updated_ = true;
      src_feat_dirty_ = tgt_feat_dirty_ = true;
    }
    if (this->source_cloud_updated_) {
      status_ = pclhip_scp_set_source(scp_, this->input_->points.data(), sizeof(PointSource), this->input_->size());
      if (status_ != PCLHIP_OK) return false;
      this->source_cloud_updated_ = false;
    }
    if (src_feat_dirty_ && input_features_) {
      status_ = pclhip_scp_set_source_features(scp_, input_features_->points.data(), sizeof(FeatureT), input_features_->size(),
                                               int(sizeof(FeatureT) / sizeof(float)));
      if (status_ != PCLHIP_OK) return false;
      src_feat_dirty_ = false;
    }
    if (tgt_feat_dirty_ && target_features_) {
      status_ = pclhip_scp_set_target_features(scp_, target_features_->points.data(), sizeof(FeatureT), target_features_->size(),
                                               int(sizeof(FeatureT) / sizeof(float)));
      if (status_ != PCLHIP_OK) return false;
      tgt_feat_dirty_ = false;
    }
    return true;
  }
  void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {  // :157-306
    this->converged_ = false;
    inliers_.clear();
    this->final_transformation_ = guess;
    if (!ensureScp()) return;
    p_.max_iterations = this->max_iterations_;
    p_.max_correspondence_distance = this->corr_dist_threshold_;
    if ((status_ = pclhip_scp_align(scp_, &p_, guess.m, &result_)) != PCLHIP_OK) return;
    std::memcpy(this->final_transformation_.m, result_.final_transformation, sizeof result_.final_transformation);
    this->converged_ = result_.converged != 0;
    std::uint64_t n = 0;
    pclhip_scp_inliers(scp_, nullptr, 0, &n);
    inliers_.resize(n);
    if (n) pclhip_scp_inliers(scp_, inliers_.data(), n, &n);
    if (this->converged_) {  // :297-298: the output is written only then
      output = *this->input_;
      pclhip_transform_cloud(this->ctx_->get(), this->final_transformation_.m, 1, output.points.data(), output.points.data(),
                             sizeof(PointSource), output.size(), 0);
    }
  }

  pclhip_scp_params p_;
  pclhip_scp_result result_ = {};
  pclhip_status status_ = PCLHIP_OK;
  pclhip_scp* scp_ = nullptr;
  pclhip_index* scp_target_ = nullptr;
  FeatureCloudConstPtr input_features_, target_features_;
  bool src_feat_dirty_ = true, tgt_feat_dirty_ = true;
  Indices inliers_;
};

// pcl::io::loadPCDFile / savePCDFile{ASCII,Binary,BinaryCompressed} (io/include/pcl/io/pcd_io.h:685-800)
// for the point types of this header: records of sizeof(PointT) bytes, normals at +16 when the type has them.
namespace io {
template <typename PointT>
int loadPCDFile(const std::string& file_name, PointCloud<PointT>& cloud) {
  pclhip_pcd_info info;
  if (pclhip_pcd_read_header(file_name.c_str(), &info) != PCLHIP_OK) return -1;
  cloud.points.assign(info.points, PointT());
  uint64_t n = 0;
  int dense = 1;
  const std::size_t nrm_off = sizeof(PointT) >= 28 ? 16 : 0;
  if (pclhip_pcd_read(file_name.c_str(), cloud.points.data(), sizeof(PointT), nrm_off, info.points, &n, &dense) != PCLHIP_OK)
    return -1;
  cloud.width = info.width;
  cloud.height = info.height;
  cloud.is_dense = dense != 0;
  for (int i = 0; i < 3; ++i) cloud.sensor_origin_[i] = info.viewpoint[i];   // VIEWPOINT tx ty tz qw qx qy qz
  cloud.sensor_origin_[3] = 0.0f;
  for (int i = 0; i < 4; ++i) cloud.sensor_orientation_[i] = info.viewpoint[3 + i];
  return 0;
}
template <typename PointT>
int savePCDFile(const std::string& file_name, const PointCloud<PointT>& cloud, int data_type, int precision = 8) {
  const std::size_t nrm_off = sizeof(PointT) >= 28 ? 16 : 0;
  // width, height and the acquisition pose travel with the cloud (PCDWriter::generateHeader, pcd_io.cpp:848-1043)
  const float vp[7] = {cloud.sensor_origin_[0], cloud.sensor_origin_[1], cloud.sensor_origin_[2],
                       cloud.sensor_orientation_[0], cloud.sensor_orientation_[1], cloud.sensor_orientation_[2],
                       cloud.sensor_orientation_[3]};
  const bool organized = std::uint64_t(cloud.width) * cloud.height == cloud.size();
  const std::uint32_t w = organized ? cloud.width : std::uint32_t(cloud.size()), h = organized ? cloud.height : 1;
  return pclhip_pcd_write_organized(file_name.c_str(), cloud.points.data(), sizeof(PointT), nrm_off, w, h, vp, data_type,
                                    precision) == PCLHIP_OK ? 0 : -1;
}
template <typename PointT> int savePCDFileASCII(const std::string& f, const PointCloud<PointT>& c) { return savePCDFile(f, c, 0); }
template <typename PointT> int savePCDFileBinary(const std::string& f, const PointCloud<PointT>& c) { return savePCDFile(f, c, 1); }
template <typename PointT> int savePCDFileBinaryCompressed(const std::string& f, const PointCloud<PointT>& c) { return savePCDFile(f, c, 2); }
}  // namespace io

// pcl::VoxelGrid<PointT> (filters/include/pcl/filters/voxel_grid.h:210-533) for pcl::PointXYZ and pcl::PointNormal
template <typename PointT = PointXYZ>
class VoxelGrid {
 public:
  VoxelGrid() : VoxelGrid(Context::defaultContext()) {}
  explicit VoxelGrid(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
  typename PointCloud<PointT>::ConstPtr getInputCloud() const { return input_; }
  void setLeafSize(float lx, float ly, float lz) { leaf_[0] = lx; leaf_[1] = ly; leaf_[2] = lz; }
  std::array<float, 3> getLeafSize() const { return {leaf_[0], leaf_[1], leaf_[2]}; }
  // :293-301: false -> only x, y, z are averaged, every other field of the output keeps its default
  void setDownsampleAllData(bool downsample) { downsample_all_data_ = downsample; }
  bool getDownsampleAllData() const { return downsample_all_data_; }
  void setMinimumPointsNumberPerVoxel(unsigned n) { min_pts_ = n; }
  unsigned getMinimumPointsNumberPerVoxel() const { return min_pts_; }
  // :440-476: pass-through filter on one field of the point type before the grid is laid out
  void setFilterFieldName(const std::string& f) { field_ = f; }
  const std::string& getFilterFieldName() const { return field_; }
  void setFilterLimits(double lo, double hi) { lo_ = lo; hi_ = hi; }
  void getFilterLimits(double& lo, double& hi) const { lo = lo_; hi = hi_; }
  void setFilterLimitsNegative(bool negative) { negative_ = negative; }  // true: keep what lies OUTSIDE the interval
  bool getFilterLimitsNegative() const { return negative_; }
  // Filter::filter -> applyFilter (filters/include/pcl/filters/impl/voxel_grid.hpp:597-814); when the
  // voxel index would overflow the reference warns and returns the input unchanged (:620-629)
  void filter(PointCloud<PointT>& output) {
    output.points.clear();
    output.height = 1;
    output.is_dense = true;
    if (!input_) { output.width = 0; return; }
    const int limits = limitFlags();
    if (limits < 0) { output.width = 0; return; }  // "could not find field": refused, not silently ignored
    constexpr std::size_t noff = has_normal_fields<PointT>() ? 16 : 0;
    std::vector<PointT> out(input_->size());
    std::uint64_t n = 0;
    leaf_layout_.clear();
    dims_ = pclhip_voxelgrid_dims{};
    if (save_leaf_layout_ && !input_->empty()) {  // one int per grid cell: learn the grid first (bounding-box pass)
      if (pclhip_voxelgrid_grid(ctx_->get(), input_->points.data(), sizeof(PointT), input_->size(), leaf_, limits,
                                lo_, hi_, &dims_) == PCLHIP_OK)
        leaf_layout_.assign(std::size_t(dims_.div_b[0]) * std::size_t(dims_.div_b[1]) * std::size_t(dims_.div_b[2]), -1);
    }
    const pclhip_status st = pclhip_voxelgrid_ex2(ctx_->get(), input_->points.data(), sizeof(PointT), input_->size(), leaf_,
                                                  min_pts_, limits, lo_, hi_, downsample_all_data_ ? 1 : 0, noff,
                                                  out.data(), sizeof(PointT), &n,
                                                  leaf_layout_.empty() ? nullptr : leaf_layout_.data(), leaf_layout_.size(),
                                                  &dims_);
    if (st == PCLHIP_ERR_OVERFLOW) { output = *input_; return; }
    if (st != PCLHIP_OK) { output.width = 0; return; }
    out.resize(std::size_t(n));
    output.points.swap(out);
    output.width = std::uint32_t(n);
  }
  // the grid of the last filter() and the leaf layout (filters/include/pcl/filters/voxel_grid.h:316-421)
  void setSaveLeafLayout(bool save) { save_leaf_layout_ = save; }
  bool getSaveLeafLayout() const { return save_leaf_layout_; }
  std::array<int, 3> getMinBoxCoordinates() const { return {dims_.min_b[0], dims_.min_b[1], dims_.min_b[2]}; }
  std::array<int, 3> getMaxBoxCoordinates() const { return {dims_.max_b[0], dims_.max_b[1], dims_.max_b[2]}; }
  std::array<int, 3> getNrDivisions() const { return {dims_.div_b[0], dims_.div_b[1], dims_.div_b[2]}; }
  std::array<int, 3> getDivisionMultiplier() const { return {dims_.divb_mul[0], dims_.divb_mul[1], dims_.divb_mul[2]}; }
  std::vector<int> getLeafLayout() const { return std::vector<int>(leaf_layout_.begin(), leaf_layout_.end()); }
  std::array<int, 3> getGridCoordinates(float x, float y, float z) const {
    return {int(std::floor(x * (1.0f / leaf_[0]))), int(std::floor(y * (1.0f / leaf_[1]))), int(std::floor(z * (1.0f / leaf_[2])))};
  }
  int getCentroidIndexAt(const std::array<int, 3>& ijk) const {
    long long idx = 0;
    for (int d = 0; d < 3; ++d) idx += (long long)(ijk[d] - dims_.min_b[d]) * dims_.divb_mul[d];
    if (idx < 0 || idx >= (long long)leaf_layout_.size()) return -1;
    return leaf_layout_[std::size_t(idx)];
  }
  int getCentroidIndex(const PointT& p) const { return getCentroidIndexAt(getGridCoordinates(p.x, p.y, p.z)); }
  // :353-376: centroid indices of the cells at the given offsets around the reference point's cell
  std::vector<int> getNeighborCentroidIndices(const PointT& reference_point, const std::vector<std::array<int, 3>>& relative_coordinates) const {
    const std::array<int, 3> c = getGridCoordinates(reference_point.x, reference_point.y, reference_point.z);
    std::vector<int> neighbors;
    for (const auto& r : relative_coordinates) {
      const std::array<int, 3> cell = {c[0] + r[0], c[1] + r[1], c[2] + r[2]};
      bool inside = true;  // the reference clamps by min_b_/max_b_
      for (int d = 0; d < 3; ++d) inside = inside && cell[d] >= dims_.min_b[d] && cell[d] <= dims_.max_b[d];
      neighbors.push_back(inside ? getCentroidIndexAt(cell) : -1);
    }
    return neighbors;
  }
 private:
  // the `has_z_limits` word of the C ABI: where the named field sits in PointT (point_types.hpp:315-321, 843-853)
  int limitFlags() const {
    if (field_.empty()) return 0;
    int idx = -1;
    if (field_ == "x") idx = 0;
    else if (field_ == "y") idx = 1;
    else if (field_ == "z") idx = 2;
    else if (has_normal_fields<PointT>()) {
      if (field_ == "normal_x") idx = 4;
      else if (field_ == "normal_y") idx = 5;
      else if (field_ == "normal_z") idx = 6;
      else if (field_ == "curvature") idx = 8;
    }
    return idx < 0 ? -1 : PCLHIP_VOXELGRID_LIMITS(idx, negative_);
  }
  Context::Ptr ctx_;
  typename PointCloud<PointT>::ConstPtr input_;
  bool save_leaf_layout_ = false, downsample_all_data_ = true;  // voxel_grid.h:501
  bool negative_ = false;
  std::vector<std::int32_t> leaf_layout_;
  pclhip_voxelgrid_dims dims_{};
  float leaf_[3] = {0, 0, 0};
  unsigned min_pts_ = 0;
  std::string field_;
  double lo_ = -FLT_MAX, hi_ = FLT_MAX;
};


// ---- outlier removal: FilterIndices<PointT> (filters/include/pcl/filters/filter_indices.h, impl/filter_indices.hpp:77-107)
// over pclhip_statistical_outlier_removal / pclhip_radius_outlier_removal.  Every filter call indexes the input cloud (the
// whole cloud: setIndices selects the queries, as in the reference, not the searched points).
template <typename PointT>
class OutlierRemovalBase : public PCLBase<PointT> {
 public:
  explicit OutlierRemovalBase(Context::Ptr ctx, bool extract_removed_indices)
      : ctx_(std::move(ctx)), extract_removed_indices_(extract_removed_indices) {}
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  void setKeepOrganized(bool keep) { keep_organized_ = keep; }
  bool getKeepOrganized() const { return keep_organized_; }
  void setUserFilterValue(float value) { user_filter_value_ = value; }
  void setNumberOfThreads(unsigned) {}  // accepted: the GPU decides its own parallelism
  IndicesConstPtr getRemovedIndices() const { return removed_indices_; }
  const std::string& getLastError() const { return error_; }
  // filter(Indices&): the kept ids in input (or setIndices) order
  void filter(Indices& indices) {
    indices.clear();
    removed_indices_ = std::make_shared<Indices>();
    if (!this->input_ || !ctx_ || !ctx_->ok()) return;
    const PointCloud<PointT>& in = *this->input_;
    pclhip_index* ix = nullptr;
    if (pclhip_index_build(ctx_->get(), in.points.data(), sizeof(PointT), in.size(), nullptr, 0, &ix) != PCLHIP_OK) {
      error_ = pclhip_last_error(ctx_->get());
      return;
    }
    const bool all = !this->indices_ || this->fake_indices_;
    const std::size_t m = all ? in.size() : this->indices_->size();
    Indices kept(m), removed(m);
    std::uint64_t nk = 0, nr = 0;
    const pclhip_status st = run(ix, all ? nullptr : this->indices_->data(), m, in.is_dense, kept.data(), &nk,
                                 (extract_removed_indices_ || keep_organized_) ? removed.data() : nullptr, &nr);
    if (st != PCLHIP_OK) error_ = pclhip_last_error(ctx_->get());
    pclhip_index_destroy(ix);
    if (st != PCLHIP_OK) return;
    kept.resize(std::size_t(nk));
    indices.swap(kept);
    if (extract_removed_indices_ || keep_organized_) {
      removed.resize(std::size_t(nr));
      removed_indices_ = std::make_shared<Indices>(std::move(removed));
    }
  }
  // filter(PointCloud&): copyPointCloud of the kept points (width = kept, height 1, is_dense of the input); with
  // setKeepOrganized the input with the xyz of removed points set to the user filter value
  void filter(PointCloud<PointT>& output) {
    if (keep_organized_) extract_removed_indices_ = true;  // filter_indices.hpp:82-86
    Indices kept;
    filter(kept);
    if (!this->input_) {
      output = PointCloud<PointT>();
      output.width = 0;
      return;
    }
    const PointCloud<PointT>& in = *this->input_;
    if (keep_organized_) {
      output = in;
      for (const index_t r : *removed_indices_) {
        output.points[std::size_t(r)].x = user_filter_value_;
        output.points[std::size_t(r)].y = user_filter_value_;
        output.points[std::size_t(r)].z = user_filter_value_;
      }
      if (!std::isfinite(user_filter_value_)) output.is_dense = false;
      return;
    }
    PointCloud<PointT> out;
    out.points.reserve(kept.size());
    for (const index_t i : kept) out.points.push_back(in.points[std::size_t(i)]);
    out.width = std::uint32_t(kept.size());
    out.height = 1;
    out.is_dense = in.is_dense;
    output = std::move(out);
  }

 protected:
  virtual pclhip_status run(pclhip_index* ix, const index_t* idx, std::size_t m, bool dense, index_t* kept,
                            std::uint64_t* nk, index_t* removed, std::uint64_t* nr) = 0;
  Context::Ptr ctx_;
  bool extract_removed_indices_ = false, negative_ = false, keep_organized_ = false;
  float user_filter_value_ = std::numeric_limits<float>::quiet_NaN();
  IndicesPtr removed_indices_ = std::make_shared<Indices>();
  std::string error_;
};

// filters/include/pcl/filters/statistical_outlier_removal.h, impl/statistical_outlier_removal.hpp:47-132
template <typename PointT>
class StatisticalOutlierRemoval : public OutlierRemovalBase<PointT> {
 public:
  explicit StatisticalOutlierRemoval(bool extract_removed_indices = false)
      : StatisticalOutlierRemoval(Context::defaultContext(), extract_removed_indices) {}
  StatisticalOutlierRemoval(Context::Ptr ctx, bool extract_removed_indices)
      : OutlierRemovalBase<PointT>(std::move(ctx), extract_removed_indices) {}
  void setMeanK(int k) { mean_k_ = k; }
  int getMeanK() const { return mean_k_; }
  void setStddevMulThresh(double m) { std_mul_ = m; }
  double getStddevMulThresh() const { return std_mul_; }
  const pclhip_sor_stats& lastStatistics() const { return stats_; }

 protected:
  pclhip_status run(pclhip_index* ix, const index_t* idx, std::size_t m, bool, index_t* kept, std::uint64_t* nk,
                    index_t* removed, std::uint64_t* nr) override {
    return pclhip_statistical_outlier_removal(ix, idx, m, mean_k_, std_mul_, this->negative_ ? 1 : 0, kept, nk, removed, nr,
                                              nullptr, &stats_);
  }
  int mean_k_ = 1;
  double std_mul_ = 0.0;
  pclhip_sor_stats stats_{};
};

// filters/include/pcl/filters/radius_outlier_removal.h, impl/radius_outlier_removal.hpp:48-172 (the cloud's is_dense
// picks the boundary of "within")
template <typename PointT>
class RadiusOutlierRemoval : public OutlierRemovalBase<PointT> {
 public:
  explicit RadiusOutlierRemoval(bool extract_removed_indices = false)
      : RadiusOutlierRemoval(Context::defaultContext(), extract_removed_indices) {}
  RadiusOutlierRemoval(Context::Ptr ctx, bool extract_removed_indices)
      : OutlierRemovalBase<PointT>(std::move(ctx), extract_removed_indices) {}
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }
  void setMinNeighborsInRadius(int n) { min_pts_ = n; }
  int getMinNeighborsInRadius() const { return min_pts_; }

 protected:
  pclhip_status run(pclhip_index* ix, const index_t* idx, std::size_t m, bool dense, index_t* kept, std::uint64_t* nk,
                    index_t* removed, std::uint64_t* nr) override {
    return pclhip_radius_outlier_removal(ix, idx, m, radius_, min_pts_, dense ? 1 : 0, this->negative_ ? 1 : 0, kept, nk,
                                         removed, nr);
  }
  double radius_ = 0.0;
  int min_pts_ = 1;
};

// ---- segmentation: pcl::PointIndices (common/include/pcl/PointIndices.h; `indices` only) and
// pcl::EuclideanClusterExtraction<PointT> (segmentation/include/pcl/segmentation/extract_clusters.h:330-435,
// impl/extract_clusters.hpp:223-253) over pclhip_euclidean_clusters.  Largest cluster first; clusters of equal size by their
// smallest index (the reference leaves that order to an unstable sort).
struct PointIndices {
  using Ptr = std::shared_ptr<PointIndices>;
  using ConstPtr = std::shared_ptr<const PointIndices>;
  Indices indices;
};

template <typename PointT>
class EuclideanClusterExtraction : public PCLBase<PointT> {
 public:
  using KdTree = search::Search<PointT>;
  using KdTreePtr = typename KdTree::Ptr;
  EuclideanClusterExtraction() : EuclideanClusterExtraction(Context::defaultContext()) {}
  explicit EuclideanClusterExtraction(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
  // a pclhip::search::KdTree is rebuilt over (input, indices) and used, as the reference does with its tree (:242); any
  // other Search is ignored and the extraction builds its own index
  void setSearchMethod(const KdTreePtr& tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setClusterTolerance(double tolerance) { cluster_tolerance_ = tolerance; }
  double getClusterTolerance() const { return cluster_tolerance_; }
  void setMinClusterSize(uindex_t n) { min_pts_per_cluster_ = n; }
  uindex_t getMinClusterSize() const { return min_pts_per_cluster_; }
  void setMaxClusterSize(uindex_t n) { max_pts_per_cluster_ = n; }
  uindex_t getMaxClusterSize() const { return max_pts_per_cluster_; }
  const std::string& getLastError() const { return error_; }
  // per record of the input: the rank of its cluster in the last extract(), -1 for a record in no returned cluster
  const std::vector<std::int32_t>& getLabels() const { return labels_; }

  void extract(std::vector<PointIndices>& clusters) {
    clusters.clear();
    labels_.clear();
    error_.clear();
    if (!this->input_ || this->input_->empty() || !ctx_ || !ctx_->ok()) return;
    const bool subset = this->indices_ && !this->fake_indices_;
    if (subset && this->indices_->empty()) return;  // :226-232
    auto tree = std::dynamic_pointer_cast<search::KdTree<PointT>>(tree_);
    if (!tree) tree = std::make_shared<search::KdTree<PointT>>(ctx_);
    if (!tree->setInputCloud(this->input_, subset ? IndicesConstPtr(this->indices_) : IndicesConstPtr())) {
      error_ = pclhip_last_error(ctx_->get());
      return;
    }
    const std::size_t n = this->input_->size();
    std::vector<std::uint64_t> offsets(n + 1, 0);
    Indices flat(n);
    labels_.assign(n, -1);
    std::uint64_t k = 0, nc = 0;
    if (pclhip_euclidean_clusters(tree->handle(), cluster_tolerance_, min_pts_per_cluster_, max_pts_per_cluster_,
                                  labels_.data(), offsets.data(), n + 1, flat.data(), n, &k, &nc) != PCLHIP_OK) {
      error_ = pclhip_last_error(tree->context()->get());
      labels_.clear();
      return;
    }
    clusters.resize(std::size_t(k));
    for (std::size_t c = 0; c < std::size_t(k); ++c)
      clusters[c].indices.assign(flat.begin() + long(offsets[c]), flat.begin() + long(offsets[c + 1]));
  }

 private:
  Context::Ptr ctx_;
  KdTreePtr tree_;
  double cluster_tolerance_ = 0.0;  // extract_clusters.h:425-431: the reference's defaults
  uindex_t min_pts_per_cluster_ = 1;
  uindex_t max_pts_per_cluster_ = std::numeric_limits<uindex_t>::max();
  std::vector<std::int32_t> labels_;
  std::string error_;
};

// pcl::RegionGrowing<PointT, NormalT> (segmentation/include/pcl/segmentation/region_growing.h:66-340,
// impl/region_growing.hpp:231-548) over pclhip_region_growing: smooth mode with the curvature test and without the residual
// test (the reference's defaults).  The segments come in the order their seeds were taken, indices ascending.  What is
// not built leaves the output empty and says why in getLastError(): the residual test, setCurvatureTestFlag(false) (the
// reference switches the residual test on with it, :120-126), setSmoothModeFlag(false), more than 64 neighbours, a NaN
// curvature.  NormalT needs normal_x/y/z and curvature (Normal, PointNormal).
template <typename PointT, typename NormalT>
class RegionGrowing : public PCLBase<PointT> {
 public:
  using KdTree = search::Search<PointT>;
  using KdTreePtr = typename KdTree::Ptr;
  using Normal = PointCloud<NormalT>;
  using NormalPtr = typename Normal::ConstPtr;
  RegionGrowing() : RegionGrowing(Context::defaultContext()) {}
  explicit RegionGrowing(Context::Ptr ctx) : ctx_(std::move(ctx)) { pclhip_region_growing_params_default(&prm_); }
  uindex_t getMinClusterSize() const { return prm_.min_cluster_size; }
  void setMinClusterSize(uindex_t n) { prm_.min_cluster_size = n; }
  uindex_t getMaxClusterSize() const { return prm_.max_cluster_size; }
  void setMaxClusterSize(uindex_t n) { prm_.max_cluster_size = n; }
  bool getSmoothModeFlag() const { return prm_.smooth_mode != 0; }
  void setSmoothModeFlag(bool value) { prm_.smooth_mode = value ? 1 : 0; }
  bool getCurvatureTestFlag() const { return prm_.curvature_test != 0; }
  void setCurvatureTestFlag(bool value) {  // :120-126
    prm_.curvature_test = value ? 1 : 0;
    if (!value && prm_.residual_test == 0) prm_.residual_test = 1;
  }
  bool getResidualTestFlag() const { return prm_.residual_test != 0; }
  void setResidualTestFlag(bool value) {  // :137-143
    prm_.residual_test = value ? 1 : 0;
    if (!value && prm_.curvature_test == 0) prm_.curvature_test = 1;
  }
  float getSmoothnessThreshold() const { return prm_.smoothness_threshold; }
  void setSmoothnessThreshold(float theta) { prm_.smoothness_threshold = theta; }
  float getResidualThreshold() const { return prm_.residual_threshold; }
  void setResidualThreshold(float residual) { prm_.residual_threshold = residual; }
  float getCurvatureThreshold() const { return prm_.curvature_threshold; }
  void setCurvatureThreshold(float curvature) { prm_.curvature_threshold = curvature; }
  unsigned int getNumberOfNeighbours() const { return unsigned(prm_.number_of_neighbours); }
  void setNumberOfNeighbours(unsigned int k) { prm_.number_of_neighbours = int(k > 0x7FFFFFFFu ? 0x7FFFFFFFu : k); }
  // a pclhip::search::KdTree is rebuilt over (input, indices) and used; any other Search is ignored
  void setSearchMethod(const KdTreePtr& tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setInputNormals(const NormalPtr& normals) { normals_ = normals; }
  NormalPtr getInputNormals() const { return normals_; }
  const std::string& getLastError() const { return error_; }
  // per record of the input: the number of its segment in the last extract(), -1 for a record in no returned segment
  const std::vector<std::int32_t>& getLabels() const { return labels_; }

  void extract(std::vector<PointIndices>& clusters) {
    clusters.clear();
    clusters_.clear();
    labels_.clear();
    error_.clear();
    // prepareForSegmentation (:278-304): no cloud, no normals, normals of another size, no neighbours -> no segment
    if (!this->input_ || this->input_->empty() || !ctx_ || !ctx_->ok()) return;
    if (!normals_ || normals_->size() != this->input_->size() || prm_.number_of_neighbours == 0) return;
    const bool subset = this->indices_ && !this->fake_indices_;
    if (subset && this->indices_->empty()) return;
    auto tree = std::dynamic_pointer_cast<search::KdTree<PointT>>(tree_);
    if (!tree) tree = std::make_shared<search::KdTree<PointT>>(ctx_);
    if (!tree->setInputCloud(this->input_, subset ? IndicesConstPtr(this->indices_) : IndicesConstPtr())) {
      error_ = pclhip_last_error(ctx_->get());
      return;
    }
    const std::size_t n = this->input_->size();
    std::vector<float> rec(4 * n);
    for (std::size_t i = 0; i < n; ++i) {
      const NormalT& p = (*normals_)[i];
      rec[4 * i] = p.normal_x; rec[4 * i + 1] = p.normal_y; rec[4 * i + 2] = p.normal_z; rec[4 * i + 3] = p.curvature;
    }
    std::vector<std::uint64_t> offsets(n + 1, 0);
    Indices flat(n);
    labels_.assign(n, -1);
    std::uint64_t k = 0, nc = 0;
    if (pclhip_region_growing(tree->handle(), rec.data(), 16, &prm_, labels_.data(), offsets.data(), n + 1, flat.data(), n, &k,
                              &nc) != PCLHIP_OK) {
      error_ = pclhip_last_error(tree->context()->get());
      labels_.clear();
      return;
    }
    clusters_.resize(std::size_t(k));
    for (std::size_t c = 0; c < std::size_t(k); ++c)
      clusters_[c].indices.assign(flat.begin() + long(offsets[c]), flat.begin() + long(offsets[c + 1]));
    clusters = clusters_;
  }

  // the segment of the last extract() that holds record `index` (the segmentation is run if it has not been); empty when
  // the record is in no returned segment
  void getSegmentFromPoint(index_t index, PointIndices& cluster) {
    cluster.indices.clear();
    if (labels_.empty() && error_.empty()) {
      std::vector<PointIndices> all;
      extract(all);
    }
    if (index < 0 || std::size_t(index) >= labels_.size() || labels_[std::size_t(index)] < 0) return;
    cluster = clusters_[std::size_t(labels_[std::size_t(index)])];
  }

 private:
  Context::Ptr ctx_;
  KdTreePtr tree_;
  NormalPtr normals_;
  pclhip_region_growing_params prm_;
  std::vector<PointIndices> clusters_;
  std::vector<std::int32_t> labels_;
  std::string error_;
};

// pcl::Keypoint<PointInT, PointOutT> (keypoints/include/pcl/keypoints/keypoint.h:52-209): compute() checks the input, calls
// the detector's detectKeypoints() and leaves the keypoints' indices behind for getKeypointsIndices().
template <typename PointInT, typename PointOutT>
class Keypoint : public PCLBase<PointInT> {
 public:
  using KdTree = search::Search<PointInT>;
  using KdTreePtr = typename KdTree::Ptr;
  using PointCloudOut = PointCloud<PointOutT>;
  void setSearchMethod(const KdTreePtr& tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setSearchSurface(const typename PointCloud<PointInT>::ConstPtr& cloud) { surface_ = cloud; }
  typename PointCloud<PointInT>::ConstPtr getSearchSurface() const { return surface_; }
  PointIndices::ConstPtr getKeypointsIndices() const { return keypoints_indices_; }
  const std::string& getLastError() const { return error_; }
  void compute(PointCloudOut& output) {  // impl/keypoint.hpp:123-147
    output.points.clear();
    output.width = 0;
    output.height = 1;
    output.is_dense = true;
    keypoints_indices_ = std::make_shared<PointIndices>();
    error_.clear();
    if (!initCompute()) return;
    detectKeypoints(output);
  }
 protected:
  virtual bool initCompute() { return bool(this->input_); }
  virtual void detectKeypoints(PointCloudOut& output) = 0;
  KdTreePtr tree_;
  typename PointCloud<PointInT>::ConstPtr surface_;
  std::shared_ptr<PointIndices> keypoints_indices_ = std::make_shared<PointIndices>();
  std::string error_;
};

// pcl::ISSKeypoint3D<PointInT, PointOutT> (keypoints/include/pcl/keypoints/iss_3d.h, impl/iss_3d.hpp:164-253, 302-473)
// without boundary estimation, over pclhip_iss_keypoints: the keypoints in ascending index order (the reference's with one
// thread).  compute() leaves the output empty and says why in getLastError() for what this path does not build: a positive
// border radius (BoundaryEstimation and the normals behind it), setIndices, another search surface, a foreign Search.
template <typename PointInT, typename PointOutT = PointInT>
class ISSKeypoint3D : public Keypoint<PointInT, PointOutT> {
 public:
  using PointCloudOut = typename Keypoint<PointInT, PointOutT>::PointCloudOut;
  ISSKeypoint3D(double salient_radius = 0.0001) : ISSKeypoint3D(Context::defaultContext(), salient_radius) {}
  explicit ISSKeypoint3D(Context::Ptr ctx, double salient_radius = 0.0001) : ctx_(std::move(ctx)), salient_radius_(salient_radius) {}
  void setSalientRadius(double r) { salient_radius_ = r; }
  void setNonMaxRadius(double r) { non_max_radius_ = r; }
  void setNormalRadius(double r) { normal_radius_ = r; }
  void setBorderRadius(double r) { border_radius_ = r; }
  void setThreshold21(double gamma_21) { gamma_21_ = gamma_21; }
  void setThreshold32(double gamma_32) { gamma_32_ = gamma_32; }
  void setMinNeighbors(int min_neighbors) { min_neighbors_ = min_neighbors; }
  void setNumberOfThreads(unsigned int nr_threads = 0) { threads_ = nr_threads; }  // only stored
  unsigned int getNumberOfThreads() const { return threads_; }
  // per record of the input, after compute(): the saliency (0: not salient) and the eigenvalues of its scatter matrix
  const std::vector<double>& getSaliency() const { return saliency_; }
  const std::vector<double>& getEigenvalues() const { return eigenvalues_; }

 protected:
  bool initCompute() override {  // impl/iss_3d.hpp:213-253
    if (!Keypoint<PointInT, PointOutT>::initCompute()) return false;
    const char* why = nullptr;
    if (!(salient_radius_ > 0.0)) why = "the salient radius must be > 0";
    else if (!(non_max_radius_ > 0.0)) why = "the non maxima radius must be > 0";
    else if (!(gamma_21_ > 0.0) || !(gamma_32_ > 0.0)) why = "the thresholds must be > 0";
    else if (min_neighbors_ <= 0) why = "the minimum number of neighbors must be > 0";
    else if (border_radius_ > 0.0 || normal_radius_ > 0.0) why = "boundary estimation (border_radius, normal_radius > 0) is not built";
    else if (this->indices_ && !this->fake_indices_) why = "setIndices is not built";
    else if (this->surface_ && this->surface_ != this->input_) why = "a search surface other than the input is not built";
    else if (!ctx_ || !ctx_->ok()) why = "no device";
    if (why != nullptr) this->error_ = why;
    return why == nullptr;
  }
  void detectKeypoints(PointCloudOut& output) override {
    const auto& input = this->input_;
    if (!this->tree_) this->tree_ = std::make_shared<search::KdTree<PointInT>>(ctx_);
    auto* dev = dynamic_cast<search::KdTree<PointInT>*>(this->tree_.get());
    if (dev == nullptr) {
      this->error_ = "the search method is not a pclhip::search::KdTree";
      return;
    }
    if (dev->getInputCloud() != input || dev->handle() == nullptr) {
      if (!dev->setInputCloud(input)) {
        this->error_ = pclhip_last_error(ctx_->get());
        return;
      }
    }
    const std::size_t n = input->size();
    Indices& idx = this->keypoints_indices_->indices;
    idx.resize(n);
    saliency_.assign(n, 0.0);
    eigenvalues_.assign(3 * n, 0.0);
    std::uint64_t k = 0;
    if (pclhip_iss_keypoints(dev->handle(), salient_radius_, non_max_radius_, gamma_21_, gamma_32_, min_neighbors_, idx.data(),
                             n, &k, saliency_.data(), eigenvalues_.data()) != PCLHIP_OK) {
      this->error_ = pclhip_last_error(dev->context()->get());
      idx.clear();
      return;
    }
    idx.resize(std::size_t(k));
    output.points.reserve(idx.size());
    for (const index_t i : idx) {  // impl/iss_3d.hpp:461-466
      PointOutT p{};
      p.x = (*input)[std::size_t(i)].x;
      p.y = (*input)[std::size_t(i)].y;
      p.z = (*input)[std::size_t(i)].z;
      output.push_back(p);
    }
    output.height = 1;
    output.is_dense = true;
  }

 private:
  Context::Ptr ctx_;
  double salient_radius_;
  double non_max_radius_ = 0.0;  // iss_3d.h:117-131: the reference's defaults
  double normal_radius_ = 0.0;
  double border_radius_ = 0.0;
  double gamma_21_ = 0.975;
  double gamma_32_ = 0.975;
  int min_neighbors_ = 5;
  unsigned int threads_ = 0;
  std::vector<double> saliency_, eigenvalues_;
};

// pcl::MLSResult's projection methods (surface/include/pcl/surface/mls.h:68) and pcl::MovingLeastSquares<PointInT, PointOutT>
// (mls.h:260-520, impl/mls.hpp:72-290) without upsampling, over pclhip_mls_process: polynomial orders 0 .. 2, the projection
// methods NONE and SIMPLE; one output record per input point with at least 3 neighbours, in ascending index.  process()
// leaves the output empty and says why in getLastError() for what this path does not build: the ORTHOGONAL projection,
// order > 2, an upsampling method, setIndices, another search surface, cached MLS results, a foreign Search.
struct MLSResult {
  enum ProjectionMethod { NONE, SIMPLE, ORTHOGONAL };
};

template <typename PointInT, typename PointOutT>
class MovingLeastSquares : public PCLBase<PointInT> {
 public:
  using KdTree = search::Search<PointInT>;
  using KdTreePtr = typename KdTree::Ptr;
  using PointCloudOut = PointCloud<PointOutT>;
  enum UpsamplingMethod { NONE, DISTINCT_CLOUD, SAMPLE_LOCAL_PLANE, RANDOM_UNIFORM_DENSITY, VOXEL_GRID_DILATION };
  MovingLeastSquares() : MovingLeastSquares(Context::defaultContext()) {}
  explicit MovingLeastSquares(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
  void setSearchMethod(const KdTreePtr& tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setSearchRadius(double radius) { search_radius_ = radius; sqr_gauss_param_ = radius * radius; }  // mls.h:365
  double getSearchRadius() const { return search_radius_; }
  void setSqrGaussParam(double sqr_gauss_param) { sqr_gauss_param_ = sqr_gauss_param; }
  double getSqrGaussParam() const { return sqr_gauss_param_; }
  void setPolynomialOrder(int order) { order_ = order; }
  int getPolynomialOrder() const { return order_; }
  void setProjectionMethod(MLSResult::ProjectionMethod method) { projection_method_ = method; }
  MLSResult::ProjectionMethod getProjectionMethod() const { return projection_method_; }
  void setComputeNormals(bool compute_normals) { compute_normals_ = compute_normals; }
  void setUpsamplingMethod(UpsamplingMethod method) { upsample_method_ = method; }
  void setCacheMLSResults(bool cache_mls_results) { cache_mls_results_ = cache_mls_results; }
  bool getCacheMLSResults() const { return cache_mls_results_; }
  void setSearchSurface(const typename PointCloud<PointInT>::ConstPtr& cloud) { surface_ = cloud; }
  void setNumberOfThreads(unsigned int threads = 1) { threads_ = threads; }  // only stored
  PointIndices::Ptr getCorrespondingIndices() const { return corresponding_input_indices_; }
  const std::string& getLastError() const { return error_; }
  // per output record, after process(): the unrounded point (3), normal (3), curvature and the neighbour count
  const std::vector<double>& getUnrounded() const { return unrounded_; }

  void process(PointCloudOut& output) {  // impl/mls.hpp:72-160
    output.points.clear();
    output.width = 0;
    output.height = 1;
    output.is_dense = true;
    corresponding_input_indices_ = std::make_shared<PointIndices>();
    unrounded_.clear();
    error_.clear();
    const char* why = nullptr;
    if (!this->input_) why = "no input cloud";
    else if (!(search_radius_ > 0.0) || !(sqr_gauss_param_ > 0.0)) why = "invalid search radius or Gaussian parameter";  // :109
    else if (order_ < 0 || order_ > 2) why = "polynomial orders 0, 1 and 2 are built";
    else if (projection_method_ == MLSResult::ORTHOGONAL) why = "the ORTHOGONAL projection is not built";
    else if (upsample_method_ != NONE) why = "upsampling is not built";
    else if (cache_mls_results_) why = "cached MLS results are not built";
    else if (this->indices_ && !this->fake_indices_) why = "setIndices is not built";
    else if (surface_ && surface_ != this->input_) why = "a search surface other than the input is not built";
    else if (!ctx_ || !ctx_->ok()) why = "no device";
    if (why != nullptr) {
      error_ = why;
      return;
    }
    const auto& input = this->input_;
    if (input->empty()) return;
    if (!tree_) tree_ = std::make_shared<search::KdTree<PointInT>>(ctx_);
    auto* dev = dynamic_cast<search::KdTree<PointInT>*>(tree_.get());
    if (dev == nullptr) {
      error_ = "the search method is not a pclhip::search::KdTree";
      return;
    }
    if (dev->getInputCloud() != input || dev->handle() == nullptr) {
      if (!dev->setInputCloud(input)) {
        error_ = pclhip_last_error(ctx_->get());
        return;
      }
    }
    const std::size_t n = input->size();
    const bool normals = compute_normals_ && has_normal_fields<PointOutT>();
    std::vector<float> xyz(3 * n), nrm(normals ? 4 * n : 0);
    Indices& idx = corresponding_input_indices_->indices;
    idx.resize(n);
    unrounded_.assign(8 * n, 0.0);
    std::uint64_t k = 0;
    if (pclhip_mls_process(dev->handle(), search_radius_, sqr_gauss_param_, order_, int(projection_method_), xyz.data(),
                           normals ? nrm.data() : nullptr, idx.data(), n, &k, unrounded_.data()) != PCLHIP_OK) {
      error_ = pclhip_last_error(dev->context()->get());
      idx.clear();
      unrounded_.clear();
      return;
    }
    idx.resize(std::size_t(k));
    unrounded_.resize(8 * std::size_t(k));
    output.points.reserve(std::size_t(k));
    for (std::size_t i = 0; i < std::size_t(k); ++i) {  // addProjectedPointNormal, impl/mls.hpp:258-283
      PointOutT p{};
      p.x = xyz[3 * i];
      p.y = xyz[3 * i + 1];
      p.z = xyz[3 * i + 2];
      if (normals) set_normal(p, &nrm[4 * i]);
      output.push_back(p);
    }
    output.height = 1;
    output.is_dense = true;
  }

 private:
  template <typename P> static typename std::enable_if<(sizeof(P) >= 48)>::type set_normal(P& p, const float* v) {
    p.normal_x = v[0];
    p.normal_y = v[1];
    p.normal_z = v[2];
    p.curvature = v[3];
  }
  template <typename P> static typename std::enable_if<(sizeof(P) < 48)>::type set_normal(P&, const float*) {}
  Context::Ptr ctx_;
  KdTreePtr tree_;
  typename PointCloud<PointInT>::ConstPtr surface_;
  double search_radius_ = 0.0;  // mls.h:297-313: the reference's defaults
  double sqr_gauss_param_ = 0.0;
  int order_ = 2;
  MLSResult::ProjectionMethod projection_method_ = MLSResult::SIMPLE;
  bool compute_normals_ = false;
  UpsamplingMethod upsample_method_ = NONE;
  bool cache_mls_results_ = false;  // (the reference's default is true: it keeps what getMLSResults hands out, not built here)
  unsigned int threads_ = 1;
  PointIndices::Ptr corresponding_input_indices_ = std::make_shared<PointIndices>();
  std::vector<double> unrounded_;
  std::string error_;
};

// ---- pcl::ModelCoefficients (common/include/pcl/ModelCoefficients.h; `values` only), the model and method constants
// (sample_consensus/model_types.h:45-47, method_types.h:45) and pcl::SACSegmentation<PointT> (segmentation/include/pcl/
// segmentation/sac_segmentation.h:77-330, impl/sac_segmentation.hpp:79-133,230-262) for SACMODEL_PLANE,
// SACMODEL_PERPENDICULAR_PLANE and SACMODEL_PARALLEL_PLANE under SAC_RANSAC over pclhip_sac_segment_plane and
// pclhip_sac_segment_model.  Any other model or method leaves both outputs empty and says so in getLastError().
struct ModelCoefficients {
  using Ptr = std::shared_ptr<ModelCoefficients>;
  using ConstPtr = std::shared_ptr<const ModelCoefficients>;
  std::vector<float> values;
};
enum SacModel {
  SACMODEL_PLANE = 0,
  SACMODEL_PERPENDICULAR_PLANE = 9,
  SACMODEL_NORMAL_PLANE = 11,
  SACMODEL_PARALLEL_PLANE = 15,
  SACMODEL_NORMAL_PARALLEL_PLANE = 16
};
constexpr int SAC_RANSAC = 0;
// What setAxis uses of Eigen::Vector3f: three floats.
struct Vector3f {
  float v[3] = {0, 0, 0};
  Vector3f() = default;
  Vector3f(float a, float b, float c) : v{a, b, c} {}
  static Vector3f Zero() { return Vector3f(); }
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
};

template <typename PointT>
class SACSegmentation : public PCLBase<PointT> {
 public:
  SACSegmentation() : SACSegmentation(Context::defaultContext()) {}
  explicit SACSegmentation(Context::Ptr ctx) : ctx_(std::move(ctx)) {
    pclhip_sac_plane_params_default(&params_);
    pclhip_sac_model_params_default(&model_);
  }
  void setModelType(int model) { model_type_ = model; }
  int getModelType() const { return model_type_; }
  // the axis and the largest angle to it (radians; 0: no constraint) of the constrained planes
  void setAxis(const Vector3f& ax) { for (int i = 0; i < 3; ++i) model_.axis[i] = ax[i]; }
  Vector3f getAxis() const { return Vector3f(model_.axis[0], model_.axis[1], model_.axis[2]); }
  void setEpsAngle(double ea) { model_.eps_angle = ea; }
  double getEpsAngle() const { return model_.eps_angle; }
  void setMethodType(int method) { method_type_ = method; }
  int getMethodType() const { return method_type_; }
  void setDistanceThreshold(double threshold) { params_.distance_threshold = threshold; }
  double getDistanceThreshold() const { return params_.distance_threshold; }
  void setMaxIterations(int max_iterations) { params_.max_iterations = max_iterations; }
  int getMaxIterations() const { return params_.max_iterations; }
  void setProbability(double probability) { params_.probability = probability; }
  double getProbability() const { return params_.probability; }
  void setOptimizeCoefficients(bool optimize) { params_.optimize_coefficients = optimize ? 1 : 0; }
  bool getOptimizeCoefficients() const { return params_.optimize_coefficients != 0; }
  // the draws are a pure function of (seed, trial, slot): include/pclhip.h
  void setSeed(std::uint64_t seed) { params_.seed = seed; }
  std::uint64_t getSeed() const { return params_.seed; }
  const std::string& getLastError() const { return error_; }
  const pclhip_sac_plane_stats& getLastStats() const { return stats_; }
  // the entries of the point set the last segment() left over, in its order (ExtractIndices::setNegative(true))
  const Indices& getOutliers() const { return outliers_; }

  void segment(PointIndices& inliers, ModelCoefficients& model_coefficients) {
    inliers.indices.clear();
    model_coefficients.values.clear();
    outliers_.clear();
    error_.clear();
    stats_ = pclhip_sac_plane_stats();
    stats_.best_trial = -1;
    if (!builds(model_type_) || method_type_ != SAC_RANSAC) {
      error_ = getClassName() + ": only the plane models of this class with SAC_RANSAC are built";
      return;
    }
    if (!this->input_ || this->input_->empty() || !ctx_ || !ctx_->ok()) return;
    const bool subset = this->indices_ && !this->fake_indices_;
    if (subset && this->indices_->empty()) return;
    const std::size_t n = this->input_->size(), m = subset ? this->indices_->size() : n;
    std::vector<float> normals;  // (nx, ny, nz, curvature) records, one per point
    if (!normalRecords(n, normals)) return;
    Indices in(m), out(m);
    float coeff[4] = {0, 0, 0, 0};
    std::uint64_t n_in = 0, n_out = 0;
    pclhip_status rc;
    if (model_type_ == SACMODEL_PLANE && normals.empty()) {
      rc = pclhip_sac_segment_plane(ctx_->get(), this->input_->points.data(), n, sizeof(PointT),
                                    subset ? this->indices_->data() : nullptr, subset ? m : 0, &params_, coeff, in.data(), m,
                                    &n_in, out.data(), m, &n_out, &stats_);
    } else {
      model_.model_type = model_type_;
      rc = pclhip_sac_segment_model(ctx_->get(), this->input_->points.data(), n, sizeof(PointT),
                                    normals.empty() ? nullptr : normals.data(), 16, subset ? this->indices_->data() : nullptr,
                                    subset ? m : 0, &params_, &model_, coeff, in.data(), m, &n_in, out.data(), m, &n_out, &stats_);
    }
    if (rc != PCLHIP_OK) {
      error_ = pclhip_last_error(ctx_->get());
      return;
    }
    out.resize(std::size_t(n_out));
    outliers_.swap(out);
    if (stats_.best_trial < 0) return;  // no model: both stay empty (impl/sac_segmentation.hpp:106-114)
    in.resize(std::size_t(n_in));
    inliers.indices.swap(in);
    model_coefficients.values.assign(coeff, coeff + 4);
  }

 protected:
  virtual std::string getClassName() const { return "SACSegmentation"; }
  // the models initSACModel builds (impl/sac_segmentation.hpp:136-370: none with normals)
  virtual bool builds(int model) const {
    return model == SACMODEL_PLANE || model == SACMODEL_PERPENDICULAR_PLANE || model == SACMODEL_PARALLEL_PLANE;
  }
  // the normals of the call as contiguous records; false: refuse the call (error_ says why)
  virtual bool normalRecords(std::size_t, std::vector<float>&) { return true; }

  Context::Ptr ctx_;
  pclhip_sac_plane_params params_;
  pclhip_sac_model_params model_;
  pclhip_sac_plane_stats stats_ = pclhip_sac_plane_stats();
  int model_type_ = -1;  // sac_segmentation.h:83-84
  int method_type_ = 0;
  Indices outliers_;
  std::string error_;
};

// pcl::SACSegmentationFromNormals<PointT, PointNT> (sac_segmentation.h:305-415, impl/sac_segmentation.hpp:374-531) for the
// plane models: SACMODEL_NORMAL_PLANE and SACMODEL_NORMAL_PARALLEL_PLANE score with the normals (include/pclhip.h), the
// three of SACSegmentation fall through to it.  Every call needs normals, one per point (:376-386).
template <typename PointT, typename PointNT>
class SACSegmentationFromNormals : public SACSegmentation<PointT> {
 public:
  using PointCloudNConstPtr = typename PointCloud<PointNT>::ConstPtr;
  SACSegmentationFromNormals() = default;
  explicit SACSegmentationFromNormals(Context::Ptr ctx) : SACSegmentation<PointT>(std::move(ctx)) {}
  void setInputNormals(const PointCloudNConstPtr& normals) { normals_ = normals; }
  PointCloudNConstPtr getInputNormals() const { return normals_; }
  void setNormalDistanceWeight(double w) { this->model_.normal_distance_weight = w; }
  double getNormalDistanceWeight() const { return this->model_.normal_distance_weight; }
  // (the class passes no tolerance with it, :452-456: it constrains nothing; pclhip_sac_model_params has eps_dist)
  void setDistanceFromOrigin(double d) { this->model_.distance_from_origin = d; }
  double getDistanceFromOrigin() const { return this->model_.distance_from_origin; }

 protected:
  std::string getClassName() const override { return "SACSegmentationFromNormals"; }
  bool builds(int model) const override {
    return SACSegmentation<PointT>::builds(model) || model == SACMODEL_NORMAL_PLANE || model == SACMODEL_NORMAL_PARALLEL_PLANE;
  }
  bool normalRecords(std::size_t n, std::vector<float>& out) override {
    if (!normals_ || normals_->size() != n) {
      this->error_ = "SACSegmentationFromNormals: setInputNormals with one normal per point first";
      return false;
    }
    out.resize(4 * n);
    for (std::size_t i = 0; i < n; ++i) {
      const PointNT& p = (*normals_)[i];
      out[4 * i] = p.normal_x; out[4 * i + 1] = p.normal_y; out[4 * i + 2] = p.normal_z; out[4 * i + 3] = p.curvature;
    }
    return true;
  }

 private:
  PointCloudNConstPtr normals_;
};

// ---- pcl::SampleConsensusModelCylinder<PointT, PointNT> (sample_consensus/include/pcl/sample_consensus/
// sac_model_cylinder.h, impl/sac_model_cylinder.hpp) and pcl::RandomSampleConsensus<PointT> (ransac.h, impl/ransac.hpp:
// 56-217) over the pclhip_sac_cylinder_* calls; include/pclhip.h states the semantics.  SACSegmentation above still refuses
// SACMODEL_CYLINDER: the cylinder lives at this level.  Not built: refineModel, setNumberOfThreads, projectPoints,
// doSamplesVerifyModel, setSamplesMaxDist.
// What the model interface uses of Eigen::VectorXf: a resizable array of floats.
struct VectorXf {
  std::vector<float> v;
  VectorXf() = default;
  explicit VectorXf(std::size_t n) : v(n, 0.0f) {}
  std::size_t size() const { return v.size(); }
  void resize(std::size_t n) { v.resize(n); }
  float& operator[](std::size_t i) { return v[i]; }
  float operator[](std::size_t i) const { return v[i]; }
  const float* data() const { return v.data(); }
  float* data() { return v.data(); }
};

// what RandomSampleConsensus needs of a model: the one call that scores, replays and selects
template <typename PointT>
class SampleConsensusModel {
 public:
  using Ptr = std::shared_ptr<SampleConsensusModel<PointT>>;
  virtual ~SampleConsensusModel() = default;
  virtual unsigned int getSampleSize() const = 0;
  virtual unsigned int getModelSize() const = 0;
  const std::string& getLastError() const { return error_; }
  // computeModel (optimize false) or what SACSegmentation::segment does; false: refused (getLastError) or no model
  virtual bool runRansac(const pclhip_sac_plane_params& params, bool optimize, Indices& sample, Indices& inliers,
                         Indices& outliers, VectorXf& coefficients, pclhip_sac_plane_stats& stats) = 0;

 protected:
  std::string error_;
};

template <typename PointT, typename PointNT>
class SampleConsensusModelCylinder : public SampleConsensusModel<PointT> {
 public:
  using Ptr = std::shared_ptr<SampleConsensusModelCylinder<PointT, PointNT>>;
  using PointCloudConstPtr = typename PointCloud<PointT>::ConstPtr;
  using PointCloudNConstPtr = typename PointCloud<PointNT>::ConstPtr;
  explicit SampleConsensusModelCylinder(const PointCloudConstPtr& cloud, bool = false)
      : SampleConsensusModelCylinder(cloud, Context::defaultContext()) {}
  SampleConsensusModelCylinder(const PointCloudConstPtr& cloud, Context::Ptr ctx) : ctx_(std::move(ctx)), input_(cloud) {
    pclhip_sac_cylinder_params_default(&model_);
  }
  SampleConsensusModelCylinder(const PointCloudConstPtr& cloud, const Indices& indices, bool = false)
      : SampleConsensusModelCylinder(cloud, indices, Context::defaultContext()) {}
  SampleConsensusModelCylinder(const PointCloudConstPtr& cloud, const Indices& indices, Context::Ptr ctx)
      : SampleConsensusModelCylinder(cloud, std::move(ctx)) {
    setIndices(indices);
  }
  void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setIndices(const Indices& indices) { indices_ = indices; subset_ = true; }
  void setInputNormals(const PointCloudNConstPtr& normals) { normals_ = normals; }
  PointCloudNConstPtr getInputNormals() const { return normals_; }
  void setNormalDistanceWeight(double w) { model_.normal_distance_weight = w; }
  double getNormalDistanceWeight() const { return model_.normal_distance_weight; }
  void setRadiusLimits(const double& min_radius, const double& max_radius) { model_.radius_min = min_radius; model_.radius_max = max_radius; }
  void getRadiusLimits(double& min_radius, double& max_radius) const { min_radius = model_.radius_min; max_radius = model_.radius_max; }
  void setAxis(const Vector3f& ax) { for (int i = 0; i < 3; ++i) model_.axis[i] = ax[i]; }
  Vector3f getAxis() const { return Vector3f(model_.axis[0], model_.axis[1], model_.axis[2]); }
  void setEpsAngle(double ea) { model_.eps_angle = ea; }
  double getEpsAngle() const { return model_.eps_angle; }
  unsigned int getSampleSize() const override { return 2; }
  unsigned int getModelSize() const override { return 7; }

  bool computeModelCoefficients(const Indices& samples, VectorXf& model_coefficients) {
    if (samples.size() != 2 || !stage()) return false;
    float c[7];
    int found = 0;
    if (!ok(pclhip_sac_cylinder_model(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), records_.data(), 16,
                                      samples.data(), &model_, c, &found)) || !found)
      return false;
    model_coefficients.v.assign(c, c + 7);
    return true;
  }
  std::size_t countWithinDistance(const VectorXf& model_coefficients, double threshold) {
    if (model_coefficients.size() != 7 || !stage()) return 0;
    std::uint32_t count = 0;
    if (!ok(pclhip_sac_cylinder_evaluate(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), records_.data(), 16,
                                         ip(), ni(), threshold, &model_, model_coefficients.data(), 1, &count, nullptr)))
      return 0;
    return count;
  }
  void selectWithinDistance(const VectorXf& model_coefficients, double threshold, Indices& inliers) {
    inliers.clear();
    if (model_coefficients.size() != 7 || !stage()) return;
    const std::size_t m = subset_ ? indices_.size() : input_->size();
    Indices in(m > 0 ? m : 1);
    std::uint64_t n_in = 0;
    if (!ok(pclhip_sac_cylinder_select(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), records_.data(), 16, ip(),
                                       ni(), threshold, &model_, model_coefficients.data(), in.data(), m, &n_in)))
      return;
    in.resize(std::size_t(n_in));
    inliers.swap(in);
  }
  void getDistancesToModel(const VectorXf& model_coefficients, std::vector<double>& distances) {
    distances.clear();
    if (model_coefficients.size() != 7 || !stage()) return;
    const std::size_t m = subset_ ? indices_.size() : input_->size();
    std::vector<double> d(m > 0 ? m : 1);
    std::uint64_t n_d = 0;
    if (!ok(pclhip_sac_cylinder_distances(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), records_.data(), 16,
                                          ip(), ni(), &model_, model_coefficients.data(), d.data(), m, &n_d)))
      return;
    d.resize(std::size_t(n_d));
    distances.swap(d);
  }
  void optimizeModelCoefficients(const Indices& inliers, const VectorXf& model_coefficients, VectorXf& optimized_coefficients) {
    optimized_coefficients = model_coefficients;
    this->error_.clear();
    if (model_coefficients.size() != 7 || !input_ || !ctx_ || !ctx_->ok()) return;
    float c[7];
    if (!ok(pclhip_sac_cylinder_optimize(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), inliers.data(),
                                         inliers.size(), &model_, model_coefficients.data(), c, &refined_, &lm_iterations_)))
      return;
    optimized_coefficients.v.assign(c, c + 7);
  }
  // of the last optimizeModelCoefficients: whether it replaced the coefficients, and the Levenberg-Marquardt steps it tried
  bool lastRefined() const { return refined_ != 0; }
  int lastIterations() const { return lm_iterations_; }

  bool runRansac(const pclhip_sac_plane_params& params, bool optimize, Indices& sample, Indices& inliers, Indices& outliers,
                 VectorXf& coefficients, pclhip_sac_plane_stats& stats) override {
    sample.clear(); inliers.clear(); outliers.clear(); coefficients.v.clear();
    stats = pclhip_sac_plane_stats();
    stats.best_trial = -1;
    if (!stage()) return false;
    const std::size_t m = subset_ ? indices_.size() : input_->size();
    Indices in(m > 0 ? m : 1), out(m > 0 ? m : 1);
    pclhip_sac_plane_params p = params;
    p.optimize_coefficients = optimize ? 1 : 0;
    float c[7];
    std::uint64_t n_in = 0, n_out = 0;
    if (!ok(pclhip_sac_cylinder_segment(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), records_.data(), 16,
                                        ip(), ni(), &p, &model_, c, in.data(), m, &n_in, out.data(), m, &n_out, &stats)))
      return false;
    out.resize(std::size_t(n_out));
    outliers.swap(out);
    if (stats.best_trial < 0) return false;
    in.resize(std::size_t(n_in));
    inliers.swap(in);
    coefficients.v.assign(c, c + 7);
    std::vector<pclhip_sac_cylinder_trace> tr(std::size_t(stats.best_trial) + 1);
    std::uint64_t count = 0;
    if (ok(pclhip_sac_last_cylinder_trace(ctx_->get(), tr.data(), tr.size(), &count)) && count > std::uint64_t(stats.best_trial)) {
      for (int k = 0; k < 2; ++k) {
        const int pos = tr[std::size_t(stats.best_trial)].samples[k];
        sample.push_back(subset_ ? indices_[std::size_t(pos)] : index_t(pos));
      }
    }
    return true;
  }

 private:
  bool ok(pclhip_status rc) {
    if (rc != PCLHIP_OK) this->error_ = pclhip_last_error(ctx_->get());
    return rc == PCLHIP_OK;
  }
  const index_t* ip() const { return subset_ ? (indices_.empty() ? &none_ : indices_.data()) : nullptr; }
  std::uint64_t ni() const { return subset_ ? indices_.size() : 0; }
  // the normals as contiguous (nx, ny, nz, curvature) records; false: refuse the call (error_ says why)
  bool stage() {
    this->error_.clear();
    if (!input_ || !ctx_ || !ctx_->ok()) {
      this->error_ = "SampleConsensusModelCylinder: no input cloud or no device";
      return false;
    }
    if (!normals_ || normals_->size() != input_->size()) {  // impl/sac_model_cylinder.hpp:85-89
      this->error_ = "SampleConsensusModelCylinder: setInputNormals with one normal per point first";
      return false;
    }
    const std::size_t n = input_->size();
    records_.resize(4 * (n > 0 ? n : 1));
    for (std::size_t i = 0; i < n; ++i) {
      const PointNT& p = (*normals_)[i];
      records_[4 * i] = p.normal_x; records_[4 * i + 1] = p.normal_y; records_[4 * i + 2] = p.normal_z;
      records_[4 * i + 3] = p.curvature;
    }
    return true;
  }

  Context::Ptr ctx_;
  PointCloudConstPtr input_;
  PointCloudNConstPtr normals_;
  Indices indices_;
  bool subset_ = false;
  index_t none_ = 0;
  pclhip_sac_cylinder_params model_;
  std::vector<float> records_;
  int refined_ = 0, lm_iterations_ = 0;
};

template <typename PointT>
class RandomSampleConsensus {
 public:
  using SampleConsensusModelPtr = typename SampleConsensusModel<PointT>::Ptr;
  explicit RandomSampleConsensus(const SampleConsensusModelPtr& model) : RandomSampleConsensus(model, std::numeric_limits<double>::max()) {}
  RandomSampleConsensus(const SampleConsensusModelPtr& model, double threshold) : model_(model) {
    pclhip_sac_plane_params_default(&params_);
    params_.distance_threshold = threshold;
    params_.max_iterations = 10000;  // ransac.h:90,101
    params_.optimize_coefficients = 0;
  }
  void setDistanceThreshold(double threshold) { params_.distance_threshold = threshold; }
  double getDistanceThreshold() const { return params_.distance_threshold; }
  void setMaxIterations(int max_iterations) { params_.max_iterations = max_iterations; }
  int getMaxIterations() const { return params_.max_iterations; }
  void setProbability(double probability) { params_.probability = probability; }
  double getProbability() const { return params_.probability; }
  // the draws are a pure function of (seed, trial, slot): include/pclhip.h
  void setSeed(std::uint64_t seed) { params_.seed = seed; }
  void setBatchSize(int n) { params_.batch_size = n; }
  bool computeModel(int = 0) { return model_ && model_->runRansac(params_, false, sample_, inliers_, outliers_, coeff_, stats_); }
  // what SACSegmentation::segment does with this model and method in one call (impl/sac_segmentation.hpp:79-133)
  bool segment(bool optimize_coefficients = true) {
    return model_ && model_->runRansac(params_, optimize_coefficients, sample_, inliers_, outliers_, coeff_, stats_);
  }
  void getModel(Indices& model) const { model = sample_; }
  void getInliers(Indices& inliers) const { inliers = inliers_; }
  void getOutliers(Indices& outliers) const { outliers = outliers_; }
  void getModelCoefficients(VectorXf& model_coefficients) const { model_coefficients = coeff_; }
  const pclhip_sac_plane_stats& getLastStats() const { return stats_; }
  SampleConsensusModelPtr getSampleConsensusModel() const { return model_; }

 private:
  SampleConsensusModelPtr model_;
  pclhip_sac_plane_params params_;
  pclhip_sac_plane_stats stats_ = pclhip_sac_plane_stats();
  Indices sample_, inliers_, outliers_;
  VectorXf coeff_;
};

}  // namespace pclhip
