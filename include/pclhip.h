/*
 * pclhip.h -- C ABI of the MI355X-native ICP hot path (k-NN correspondence search, normal
 * estimation, point-to-point / point-to-plane ICP, VoxelGrid prefilter).
 *
 * PCL has no FFI: the path sits behind C++ virtual plugin points.  Each entry point below names
 * the reference interface it replaces (file:line relative to the PCL tree); the adapter classes
 * in include/pclhip/pcl_compat.hpp (and the real-PCL subclasses shown in INTEGRATION.md) are the
 * only intended callers.
 *
 * Conventions
 *  - plain C, opaque handles, no exceptions across the boundary; every function returns
 *    PCLHIP_OK (0) or a negative pclhip_status; pclhip_last_error() gives the message.
 *  - point buffers are arrays of records with a byte stride; x,y,z are three consecutive floats
 *    at byte 0 of each record (pcl::PointXYZ = 16 B, pcl::PointNormal = 48 B with the normal at
 *    +16, common/include/pcl/impl/point_types.hpp:315-321,843-853).  Buffers may live in host OR
 *    device memory -- the library detects which (hipPointerGetAttributes) and stages host data.
 *    A DEVICE buffer must be complete when it is handed over: the context works on its own stream and
 *    does not wait for the stream that is still producing the buffer (create the context on that stream
 *    with pclhip_ctx_create_on_stream, or synchronise the producer first).
 *  - index_t is int32 (common/include/pcl/types.h:110-133); "no neighbour" is -1, distance +inf.
 *  - a handle is not thread-safe, with one exception: the QUERY entry points pclhip_knn and
 *    pclhip_radius_search may be called concurrently on one index / context (PCL calls its `const`
 *    search virtuals from OpenMP loops: registration/.../impl/correspondence_estimation.hpp:163-175,
 *    features/.../impl/normal_3d_omp.hpp:76-81, search/.../impl/search.hpp:164-190); such callers are
 *    served one after the other (a lock of the context), not in parallel.  Building, destroying or
 *    aligning on the same context meanwhile is the caller's race.  Distinct contexts may be used
 *    concurrently.  All work of a context is issued on its HIP stream; entry points that return host
 *    results synchronise it.
 *  - results: k-NN indices/distances are bit-exact w.r.t. the CPU oracle (float L2_Simple
 *    ((dx*dx)+dy*dy)+dz*dz, ascending (distance, index), ties -> lower index).
 */
#ifndef PCLHIP_H_
#define PCLHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define PCLHIP_API __attribute__((visibility("default")))
#else
#define PCLHIP_API
#endif

typedef int pclhip_status;
enum {
  PCLHIP_OK = 0,
  PCLHIP_ERR_INVALID = -1,  /* bad argument */
  PCLHIP_ERR_HIP = -2,      /* HIP runtime failure (message has hipGetErrorString) */
  PCLHIP_ERR_NO_DEVICE = -3,
  PCLHIP_ERR_STATE = -4,    /* call order (e.g. point-to-plane without target normals) */
  PCLHIP_ERR_OVERFLOW = -5  /* VoxelGrid: leaf too small, int32 voxel index would overflow */
};

typedef struct pclhip_ctx pclhip_ctx;
typedef struct pclhip_index pclhip_index;
typedef struct pclhip_icp pclhip_icp;

/* ---- context --------------------------------------------------------------------------------
 * stream: a hipStream_t to issue work on (e.g. torch.cuda.current_stream().cuda_stream), or NULL
 * to let the context create its own non-blocking stream. */
PCLHIP_API pclhip_status pclhip_ctx_create(int device, void* stream, pclhip_ctx** out);
/* Same, but `stream` is adopted as given -- including NULL, which then means the device's legacy default
 * stream (what torch.cuda.current_stream().cuda_stream is when torch runs on its default stream), not
 * "create one".  Use this whenever the caller orders its own work (collectives, copies) on that stream. */
PCLHIP_API pclhip_status pclhip_ctx_create_on_stream(int device, void* stream, pclhip_ctx** out);
/* the hipStream_t the context issues its work on */
PCLHIP_API void* pclhip_ctx_stream(const pclhip_ctx* ctx);
PCLHIP_API void pclhip_ctx_destroy(pclhip_ctx* ctx);
PCLHIP_API const char* pclhip_last_error(const pclhip_ctx* ctx /* may be NULL */);
PCLHIP_API pclhip_status pclhip_ctx_synchronize(pclhip_ctx* ctx);
/* Reserve `bytes` of device memory as the context's arena: index arrays, registration state and every temporary are
 * carved out of it (what does not fit falls back to hipMalloc), so the first index build of a context costs what a
 * rebuild costs.  Without this call the context reserves 288 bytes per point of the first cloud of a million points or
 * more that it sees (option "arena_mb" overrides; 0 = no arena).  No PCL counterpart: PCL's containers allocate on the
 * host (common/include/pcl/point_cloud.h:393-409); this is the device side of that. */
PCLHIP_API pclhip_status pclhip_ctx_reserve(pclhip_ctx* ctx, uint64_t bytes);
/* The tuning knobs of a context, in one place (the library reads no environment variable; none of these changes a result):
 *   "served_groups"  0 | 1  target sharding: pclhip_icp_align / pclhip_icp_run_steps walk only the 64-point groups the rank
 *                           serves (default 1; 0 = every launch walks the whole source -- the reference of the tests)
 *   "icp_lookahead"  n      pclhip_icp_align: iterations queued ahead of the host's knowledge (default 1)
 *   "step_events"    0 | 1  1: the chain-free device-driven loop brackets the kernels of a step with HIP events, like the
 *                           loops with rejectors / reciprocal / served groups / per-lane search do (default 0: its kernels
 *                           stamp their own times and the step record is the completion signal; an A/B switch)
 *   "cache_mb"       n      device blocks kept for reuse between calls, MiB (default 16384, at most a quarter of the device)
 *   "arena_mb"       n      size of the automatic arena (pclhip_ctx_reserve), MiB; 0 = none (default: 288 B per point);
 *                           PCLHIP_ERR_STATE once the arena exists
 *   "cell_start"     0 | 1  seeded descents test the kd CELL of the level-2 / level-3 node of a seed (pclhip_index_cells)
 *                           instead of its tight box when they look for a start level (default 1)
 *   "reseed"         0 | 1  a 64-query group whose seeds are all farther than two leaf diagonals gets one fresh seed from a
 *                           greedy walk down the hierarchy (default 1)
 *   "lane_search"    0 | 1  the seeded launches of an ICP iteration run one lane per query over the quad levels and their
 *                           cells (lane.hip) instead of the wave-cooperative traversal (default 0: exact, measured 2.5x
 *                           slower at 10M points -- and in the device-driven loop every iteration then queues the
 *                           fall-through search kernel plus three lane kernels, launch overhead that figure does not
 *                           separate out); "lane_max_up" n (default 2) quad levels the first pass climbs,
 *                           "lane_far" x (default 0.25) squared mean leaf diagonals beyond which a seed is replaced
 *   "standoff_thickness" x, "standoff_max_mb" n   which indices the launch that starts an alignment searches by the stand-off
 *                           body (leaf discs): leaves thinner than x against their width (default 0.3) and an index of at
 *                           most n MiB (default: no limit); everything else goes through the seeded body with disc bounds
 * No PCL counterpart (PCL's knobs are the setters of its classes, which the bindings map onto the calls below). */
PCLHIP_API pclhip_status pclhip_ctx_set_option(pclhip_ctx* ctx, const char* name, double value);
PCLHIP_API const char* pclhip_version(void);
/* Optional traversal work counters (diagnostics): enable != 0 allocates/zeroes 8 device counters
 * that every search kernel of this context adds to; out (8 x uint64, may be NULL) receives the
 * current values: [0] interior nodes scanned, [1] leaves past the group test, [2] leaves past the
 * per-lane test (16-candidate all-pairs blocks), [3] stack pushes, [4] 64-query groups.  (With "lane_search" the lane
 * kernels count in the same slots: [0] queries, [1] done with their own leaf, [2] done in the first pass, [3] greedy
 * descents, [4] finished by the second pass.) */
PCLHIP_API pclhip_status pclhip_ctx_stats(pclhip_ctx* ctx, int enable, uint64_t* out);

/* ---- spatial index over the target cloud ------------------------------------------------------
 * Replaces pcl::KdTreeFLANN<PointT>::setInputCloud (kdtree/include/pcl/kdtree/impl/
 * kdtree_flann.hpp:99-136) as called from pcl::search::KdTree<PointT>::setInputCloud
 * (search/include/pcl/search/impl/kdtree.hpp:87-97) and Registration::initCompute
 * (registration/include/pcl/registration/impl/registration.hpp:84-87).
 * Non-finite points are dropped (kdtree_flann.hpp:443-452).  `indices` (optional) selects a subset
 * exactly like the (cloud, indices) overload (:428-498): returned neighbour indices are indices
 * into the ORIGINAL cloud. */
PCLHIP_API pclhip_status pclhip_index_build(pclhip_ctx* ctx, const void* points, size_t stride_bytes,
                                            uint64_t n, const int32_t* indices, uint64_t n_indices,
                                            pclhip_index** out);
/* The same through a pcl::PointRepresentation that maps a point to (x, y, z) times per-axis rescale values
 * (pcl::search::KdTree::setPointRepresentation, search/include/pcl/search/kdtree.h:110; KdTreeFLANN vectorises
 * every point with it, kdtree_flann.hpp:463-498; CustomPointRepresentation / setRescaleValues,
 * common/include/pcl/point_representation.h:150-190,546-579): the index holds coordinate * scale[axis], queries of
 * pclhip_knn / pclhip_radius_search are mapped the same way, distances are those of the rescaled space.  A
 * scale of 0 removes the axis (e.g. {1, 1, 0}: the x-y representation; that coordinate need not be finite).
 * scale == NULL: the default representation.  Registration (pclhip_icp_create) needs the default one. */
PCLHIP_API pclhip_status pclhip_index_build_scaled(pclhip_ctx* ctx, const void* points, size_t stride_bytes,
                                                   uint64_t n, const int32_t* indices, uint64_t n_indices,
                                                   const float scale[3], pclhip_index** out);
/* The same, and the records' own normals -- (nx, ny, nz, curvature) at `normals_offset_bytes` inside every record, 0 =
 * none -- attached to the index from the same upload (pclhip_index_set_normals would stage the cloud a second time):
 * pcl::PointNormal clouds as IterativeClosestPointWithNormals takes them (registration/include/pcl/registration/icp.h
 * :330-345; the normals sit at +16). */
PCLHIP_API pclhip_status pclhip_index_build_ex(pclhip_ctx* ctx, const void* points, size_t stride_bytes, uint64_t n,
                                               const int32_t* indices, uint64_t n_indices, const float* scale,
                                               size_t normals_offset_bytes, pclhip_index** out);
PCLHIP_API void pclhip_index_destroy(pclhip_index* index);
/* number of finite points indexed */
PCLHIP_API uint64_t pclhip_index_size(const pclhip_index* index);
/* milliseconds of GPU time spent in the last build (bbox + kd ordering by radix-sort rounds + gather + boxes) */
PCLHIP_API double pclhip_index_build_ms(const pclhip_index* index);
/* The order the index keeps its points in: out[j] = original index of the point at position j (pclhip_index_size entries,
 * host or device memory).  Consecutive positions are spatial neighbours -- every aligned run of 16 * 4^k positions is one
 * cell of a kd partition -- so a caller can lay per-point attributes out the same way.  (KdTreeFLANN keeps the
 * corresponding permutation private: kdtree_flann.h `index_mapping_`; tests use this to check the cells.) */
PCLHIP_API pclhip_status pclhip_index_order(pclhip_index* index, int32_t* out);
/* The structure the per-lane search of the seeded ICP launches walks (round 5): the kd order seen as a 4-ary tree over
 * the 16-point leaves.  Level q has ceil(leaves / 4^q) nodes; node i covers positions [16 i 4^q, 16 (i+1) 4^q) of
 * pclhip_index_order.  For one level: boxes[6 i ..] = tight AABB (lo xyz, hi xyz) of node i, cells[6 i ..] = its CELL --
 * an axis-aligned region, +-inf where unbounded, whose INTERIOR holds no point of any other node (what lets a search
 * stop inside the node; an inverted cell, lo > hi, marks a node whose siblings the build could not separate).
 * *count receives the number of nodes of the level, *top_level the root's level; buffers (host memory, `capacity` nodes
 * each, either may be NULL) are filled when capacity suffices.  No counterpart in PCL (FLANN keeps its tree private);
 * tests check the cells against the points with it.  PCLHIP_ERR_STATE for an index without the structure. */
PCLHIP_API pclhip_status pclhip_index_cells(pclhip_index* index, int level, float* boxes, float* cells, uint64_t capacity,
                                            uint64_t* count, int* top_level);

/* Exact k nearest neighbours of nq query points.
 * Replaces pcl::KdTreeFLANN<PointT>::nearestKSearch (kdtree_flann.hpp:234-274) and the batch
 * overloads of pcl::search::Search<PointT>::nearestKSearch (search/include/pcl/search/impl/
 * search.hpp:113-136).  k is clamped to the index size (:241-242); unused slots get -1 / +inf.
 * out_idx: nq*k int32, out_d2: nq*k float (squared L2), both host or device memory.
 * Non-finite queries return no neighbours. */
PCLHIP_API pclhip_status pclhip_knn(pclhip_index* index, const void* queries, size_t stride_bytes,
                                    uint64_t nq, int k, int32_t* out_idx, float* out_d2);

/* All neighbours within `radius` of nq query points, as a CSR list.
 * Replaces pcl::KdTreeFLANN<PointT>::radiusSearch (kdtree_flann.hpp:372-414) and the batch overload of
 * pcl::search::Search<PointT>::radiusSearch (search/include/pcl/search/impl/search.hpp:164-190):
 * squared distance < float(radius*radius), ascending (distance, index); max_nn > 0 keeps only the
 * max_nn nearest of each query (max_nn = 0: all).  out_offsets: nq+1 uint64 in HOST memory (always
 * written); *out_total = out_offsets[nq].  out_idx/out_d2 (host or device) must hold `capacity`
 * entries; if capacity < *out_total the call returns PCLHIP_ERR_OVERFLOW after writing the offsets,
 * so a caller sizes the buffers with a first call (capacity 0) and fetches with a second. */
PCLHIP_API pclhip_status pclhip_radius_search(pclhip_index* index, const void* queries, size_t stride_bytes,
                                              uint64_t nq, double radius, uint32_t max_nn, uint64_t* out_offsets,
                                              int32_t* out_idx, float* out_d2, uint64_t capacity,
                                              uint64_t* out_total);

/* Surface normals + curvature of every indexed point from its k nearest neighbours in the index.
 * Replaces pcl::NormalEstimation<PointInT,PointOutT>::computeFeature (features/include/pcl/
 * features/impl/normal_3d.hpp:48-95) with setKSearch(k), search surface == input:
 * computeMeanAndCovarianceMatrix (common/include/pcl/common/impl/centroid.hpp:581-650) ->
 * solvePlaneParameters/eigen33 (features/include/pcl/features/impl/feature.hpp:64-89,
 * common/include/pcl/common/impl/eigen.hpp:295-325) -> flipNormalTowardsViewpoint
 * (features/include/pcl/features/normal_3d.h:169-188).
 * out (optional, host or device): one record per ORIGINAL cloud point (n of pclhip_index_build):
 * 4 floats nx,ny,nz,curvature at byte 0 of each out_stride_bytes record; NaN for dropped points.
 * The normals are also retained inside the index for point-to-plane ICP.  out_nan_count optional. */
PCLHIP_API pclhip_status pclhip_normals(pclhip_index* index, int k, const float viewpoint[3],
                                        void* out, size_t out_stride_bytes, uint64_t* out_nan_count);
/* The same normals (k >= 1 and radius 0, or k 0 and radius > 0) written as WHOLE output records, the way
 * Feature::compute leaves a PointCloud<pcl::Normal> (impl/feature.hpp:195-229: the cloud is resized -- value-initialised
 * records -- and computeFeature fills normal[0..2] and curvature, normal_3d.hpp:60-66): every record_bytes record is
 * zeroed, the normal goes to normal_offset, the curvature to curvature_offset (pcl::Normal: 32 / 0 / 16).  A host `out`
 * costs one linear copy instead of 16-byte rows into a staging array plus the caller's unpacking loop: a repeated
 * NormalEstimation::compute of 10M points through the binding 87 -> 7.6 ms, a first one 185 -> 94 ms (of which 60 are
 * PCL's own resize of the output cloud; scratch/boundary_probe.cpp). */
PCLHIP_API pclhip_status pclhip_normals_records(pclhip_index* index, int k, double radius, const float viewpoint[3],
                                                void* out, size_t record_bytes, size_t normal_offset,
                                                size_t curvature_offset, uint64_t* out_nan_count);
/* Same with setRadiusSearch(radius) (Feature::compute, features/include/pcl/features/impl/feature.hpp:140-155):
 * the plane is fitted to ALL indexed points with squared distance < float(radius^2), taken in the
 * order radiusSearch returns them (ascending distance); fewer than 3 neighbours -> NaN. */
PCLHIP_API pclhip_status pclhip_normals_radius(pclhip_index* index, double radius, const float viewpoint[3],
                                               void* out, size_t out_stride_bytes, uint64_t* out_nan_count);
/* The same two searches with a SEARCH SURFACE different from the input cloud, and/or over an index subset of the
 * input: Feature::setSearchSurface / PCLBase::setIndices (features/include/pcl/features/feature.h:139-153,
 * impl/feature.hpp:104-118; common/include/pcl/pcl_base.h:102-125) as NormalEstimation::computeFeature uses them
 * (impl/normal_3d.hpp:48-95): `index` holds the surface; query j is record indices[j] of `queries` (record j when
 * indices is NULL); its plane is fitted to the surface points the search returns, in that order, and the normal is
 * flipped towards the viewpoint as seen from the QUERY point.  Exactly one of k >= 1 / radius > 0.
 * out (host or device): nx,ny,nz,curvature at byte 0 of out_stride_bytes records, one per query; NaN where the query
 * is non-finite or has fewer than 3 neighbours.  Nothing is retained in the index.
 * Radius mode accumulates the covariance inside the traversal, shifted by the QUERY point and summed in double in
 * traversal order; the reference shifts by the first neighbour returned and sums in float in ascending-distance order
 * (common/include/pcl/common/impl/centroid.hpp:581-650).  For self-queries the two shifts coincide; for a search surface
 * that is not the input the results meet the 1e-5 contract on normals and curvature, not bit parity. */
PCLHIP_API pclhip_status pclhip_normals_at(pclhip_index* surface, const void* queries, size_t stride_bytes, uint64_t n_queries,
                                           const int32_t* indices, uint64_t n_indices, int k, double radius,
                                           const float viewpoint[3], void* out, size_t out_stride_bytes,
                                           uint64_t* out_nan_count);
/* GeneralizedIterativeClosestPoint::computeCovariances (registration/include/pcl/registration/impl/gicp.hpp
 * :70-147): for every indexed point the covariance of its k nearest neighbours (k_correspondences_, default
 * 20, <= 32 here), regularised to singular values (1, 1, epsilon) (gicp_epsilon_, default 0.001).
 * out (host or device): 9 doubles (row-major 3x3) per ORIGINAL cloud point; NaN for dropped points. */
PCLHIP_API pclhip_status pclhip_gicp_covariances(pclhip_index* index, int k, double epsilon, double* out);

/* ---- outlier removal over an index built over the WHOLE input cloud (no indices, unscaled) ----------
 * Queries: every record of the cloud (indices == NULL) or indices[0..n_indices) in that order, each against the whole
 * index; kept / removed (host or device, each room for as many ids as there are queries, either may be NULL) receive
 * the queries' record ids in query order (FilterIndices::filter(Indices&), filters/include/pcl/filters/impl/
 * filter_indices.hpp:77-107; getRemovedIndices).  A record the index dropped (non-finite) has no neighbours.  Organized
 * clouds are searched with the same exact index where the reference would pick OrganizedNeighbor.
 * pclhip_index_last_kernel_ms gives the GPU time of the whole call. */
typedef struct pclhip_sor_stats {
  double mean;       /* of the valid (finite) queries' mean distances */
  double stddev;
  double threshold;  /* mean + std_mul * stddev */
  double sum;        /* sum of the distances (non-finite queries add 0) */
  double sq_sum;     /* sum of fl(d * d) */
  uint64_t valid;    /* finite queries */
} pclhip_sor_stats;
/* pcl::StatisticalOutlierRemoval<PointT>::applyFilterIndices (filters/include/pcl/filters/impl/
 * statistical_outlier_removal.hpp:47-132).  Per query the mean of sqrt(d2) over its neighbours 1..K-1, K =
 * min(mean_k + 1, finite points) (the query itself is neighbour 0): the square root is taken in double of the float d2,
 * summed in ascending order in double, divided by K - 1 and rounded to float, as :96-99.  Non-finite queries get 0 and
 * are not counted in `valid`.  The statistics (:104-117) are sums in double over a fixed-order tree -- bitwise
 * repeatable, but not the reference's sequential sum (agreement to ~1e-15 relative).  A query is removed iff d >
 * threshold (negative: d <= threshold); a NaN distance or threshold removes nothing.  mean_distances (host or device,
 * optional): the per-query mean distances; stats (optional).  mean_k < 1 is PCLHIP_ERR_INVALID (the reference divides
 * by zero). */
PCLHIP_API pclhip_status pclhip_statistical_outlier_removal(pclhip_index* index, const int32_t* indices, uint64_t n_indices,
                                                            int mean_k, double std_mul, int negative, int32_t* kept,
                                                            uint64_t* n_kept, int32_t* removed, uint64_t* n_removed,
                                                            float* mean_distances, pclhip_sor_stats* stats);
/* pcl::RadiusOutlierRemoval<PointT>::applyFilterIndices (filters/include/pcl/filters/impl/radius_outlier_removal.hpp
 * :48-172).  A query has enough neighbours when at least min_pts + 1 points of the index (itself included) lie within
 * the radius; "within" is (double)d2 <= r*r for is_dense (the nearestKSearch path, :84-115) and d2 < float(r*r)
 * otherwise (the radiusSearch path, :119-147, as pclhip_radius_search).  is_dense: kept iff enough XOR negative;
 * otherwise a non-finite query is always removed and a finite one kept iff enough XOR negative.  radius == 0 is
 * PCLHIP_ERR_INVALID (:52-58). */
PCLHIP_API pclhip_status pclhip_radius_outlier_removal(pclhip_index* index, const int32_t* indices, uint64_t n_indices,
                                                       double radius, int min_pts, int is_dense, int negative,
                                                       int32_t* kept, uint64_t* n_kept, int32_t* removed,
                                                       uint64_t* n_removed);
/* pcl::FPFHEstimation<PointInT, PointNT, PointOutT>::computeFeature with setRadiusSearch (features/include/pcl/features/
 * impl/fpfh.hpp:51-303, pcl::computePairFeatures of features/src/pfh.cpp:45-103): search surface == input, 11 / 11 / 11
 * bins.  `index` is built over the whole unscaled cloud and holds normals (pclhip_normals* or pclhip_index_set_normals):
 * PCLHIP_ERR_STATE without them; radius <= 0 is PCLHIP_ERR_INVALID.  The neighbourhood is every indexed point with float
 * d2 < float(radius * radius), the point itself included (as pclhip_radius_search).  A positive radius whose float square
 * is 0 (below about 2.6e-23) is a valid call in which no point has a neighbour, not even itself, as in the reference:
 * every SPFH row of a point with a finite normal is all-zero, every FPFH row is NaN and counted in out_nan_count.
 *   out       (host or device) 33 floats (f1, f2, f3 histograms) at byte 0 of each out_stride_bytes record, one per query:
 *             every record of the cloud, or indices[0..n_indices) in that order
 *   out_spfh  (host or device, optional) the 33-float SPFH rows (computePointSPFHSignature), dense, one per ORIGINAL
 *             record
 * The SPFH values are the reference's bit for bit wherever its float pair features and this device's fall into the same
 * bins (hist_incr added once per hit, in float: independent of the neighbours' order).  The weighting sums the exact
 * double products of SPFH value and float weight 1.0f / d2 in double, in traversal order, where the reference sums float
 * products in float in ascending distance; each histogram is then scaled by 100.0 / sum in double as the reference does.
 * A point with no neighbour but itself gets an all-zero row.  A record the index dropped (non-finite) gets 33 NaN in
 * both outputs and is counted in out_nan_count.
 * Deviation -- non-finite normals (the reference casts a NaN feature to int: undefined): a point whose own normal is not
 * finite gets 33 NaN in both outputs and is counted; a neighbour whose normal is not finite is skipped in both passes
 * but still counts towards hist_incr = 100 / (neighbours - 1).
 * Cost with `indices`: the SPFH pass still runs over the WHOLE cloud (the reference computes only the union of the
 * queries' neighbourhoods); only the weighting pass is restricted to the queries.
 * A neighbourhood of more than 65536 points is PCLHIP_ERR_OVERFLOW (a bin counter holds 16 bits; nothing is truncated).
 * pclhip_index_last_kernel_ms gives the GPU time of the whole call, pclhip_index_last_fpfh_ms that of its two passes. */
PCLHIP_API pclhip_status pclhip_fpfh(pclhip_index* index, const int32_t* indices, uint64_t n_indices, double radius,
                                     void* out, size_t out_stride_bytes, float* out_spfh, uint64_t* out_nan_count);
/* GPU time (ms) of the SPFH kernel and of the weighting kernel of the last pclhip_fpfh on this index. */
PCLHIP_API void pclhip_index_last_fpfh_ms(const pclhip_index* index, double* spfh_ms, double* weight_ms);
/* pcl::ISSKeypoint3D<PointInT, PointOutT>::detectKeypoints without boundary estimation (keypoints/include/pcl/keypoints/
 * impl/iss_3d.hpp:164-208, 302-473; border_radius == 0): search surface == input.  A neighbourhood is every indexed point
 * with float d2 < float(r * r), the point itself included (as pclhip_radius_search).
 *   1. Per finite point i with m >= min_neighbors points within salient_radius: C = sum (p_j - p_i)(p_j - p_i)^T with the
 *      coordinates widened to double before the subtraction and all sums in double; eigenvalues e1 >= e2 >= e3 in double;
 *      the saliency is s_i = e3 iff e2 / e1 < gamma_21 && e3 / e2 < gamma_32 (both in double, a NaN ratio fails), else 0.
 *   2. A point with s_i > 0 is a keypoint iff its non_max_radius neighbourhood holds >= min_neighbors points and no
 *      neighbour j has s_i < s_j (strict: equal saliencies all win).
 *   3. out_indices receives the keypoints' original indices, ascending (the reference's order with one thread).
 *   out_indices      (host or device) room for `capacity` ids; *n_keypoints is always written, a capacity that is too
 *                    small gives PCLHIP_ERR_OVERFLOW after it is (n_orig always suffices)
 *   out_saliency     (host or device, optional) n_orig doubles: s_i, 0 for a record that is not salient (a non-finite one
 *                    included)
 *   out_eigenvalues  (host or device, optional) 3 * n_orig doubles, descending: 0, 0, 0 below min_neighbors, NaN for a
 *                    non-finite record
 * A radius, gamma or min_neighbors that is <= 0 or not finite is PCLHIP_ERR_INVALID (ISSKeypoint3D::initCompute refuses
 * them).  A positive radius whose float square is 0 is a valid call in which no point has a neighbour, not even itself:
 * m = 0 < min_neighbors, no keypoints.  The index must cover the whole unscaled cloud: one built with `indices` or with
 * rescale values is PCLHIP_ERR_STATE.
 * Deviations: a point with e3 < 0 or a non-finite eigenvalue is not salient (the reference skips the store and later reads
 * uninitialised memory for it); boundary estimation (border_radius > 0, normal_radius) is not built; non-finite records
 * are never keypoints and never neighbours; the eigenvalues come from a cyclic Jacobi iteration in double and the sums run
 * in traversal order (the reference: Eigen's QR iteration, ascending distance) -- each eigenvalue lies within
 * (m + 32) * 2^-53 * trace(C) of the exact one.  Two calls give the same bytes.
 * pclhip_index_last_kernel_ms gives the GPU time of the whole call, pclhip_index_last_iss_ms that of its two passes. */
PCLHIP_API pclhip_status pclhip_iss_keypoints(pclhip_index* index, double salient_radius, double non_max_radius,
                                              double gamma_21, double gamma_32, int min_neighbors, int32_t* out_indices,
                                              uint64_t capacity, uint64_t* n_keypoints, double* out_saliency,
                                              double* out_eigenvalues);
/* GPU time (ms) of the scatter kernel and of the non-maximum kernel of the last pclhip_iss_keypoints on this index. */
PCLHIP_API void pclhip_index_last_iss_ms(const pclhip_index* index, double* scatter_ms, double* nms_ms);
/* pcl::MovingLeastSquares<PointInT, PointOutT>::process (surface/include/pcl/surface/mls.h, impl/mls.hpp: process,
 * performProcessing, computeMLSPointNormal, MLSResult::computeMLSSurface and ::projectQueryPoint) with
 * setUpsamplingMethod(NONE), polynomial_order 0, 1 or 2 and projection_method NONE or SIMPLE: search surface == input.  A
 * neighbourhood is every indexed point with float d2 < float(r * r), the point itself included (as pclhip_radius_search).
 * Per indexed point q with m neighbours, in ascending original index:
 *   1. m < 3: no output record.
 *   2. Plane: the centroid c and C = sum (p_j - c)(p_j - c)^T in double; the smallest eigenvalue l0 of C and its unit
 *      eigenvector n; mean = q - ((q - c) . n) n; curvature = |l0 / trace(C)| (0 when the trace is 0);
 *      v = unitOrthogonal(n) by Eigen's rule for 3-vectors, u = n x v.
 *   3. Fit, only with polynomial_order == 2 and m >= 6: d = p_j - mean, w = exp(-d.d / sqr_gauss_param),
 *      (u_j, v_j, f_j) = (d.u, d.v, d.n), P_j = (1, v, v^2, u, uv, u^2); (sum w P P^T) coeff = sum w P f by Cholesky in
 *      double.  A pivot that is not positive or a coeff[0] that is not finite leaves the point with its plane.
 *   4. With a fit and PCLHIP_MLS_SIMPLE: point = mean + coeff[0] n, normal = normalize(n - coeff[3] u - coeff[1] v);
 *      otherwise point = mean, normal = n.
 *   out_points   (host or device, optional) 3 floats per output record
 *   out_normals  (host or device, optional: setComputeNormals) 4 floats per output record: nx ny nz curvature
 *   out_indices  (host or device, optional) corresponding_input_indices: the record's original index, ascending
 *   out_double   (host or device, optional) 8 doubles per output record, unrounded: point (3), normal (3), curvature, m
 * Each has room for `capacity` records; *n_out is always written, a capacity that is too small gives
 * PCLHIP_ERR_OVERFLOW after it is (n_orig always suffices).
 * search_radius or sqr_gauss_param <= 0 or not finite, an order outside 0 .. 2 and the ORTHOGONAL projection are
 * PCLHIP_ERR_INVALID with an empty output.  A positive radius whose float square is 0 is a valid call in which no point
 * has a neighbour: no output.  The index must cover the whole unscaled cloud: one built with `indices` or with rescale
 * values is PCLHIP_ERR_STATE.
 * Deviations: the sign of n is a function of C alone -- its component of largest magnitude is positive, ties go to the
 * lowest axis (the reference's eigen33 leaves the sign to its cross products; points and curvature do not depend on it);
 * the sums run in traversal order, one-pass and shifted by the query, the 6 x 6 matrix is assembled from 15 moments (the
 * reference: ascending distance, two-pass, P diag(w) P^T); the eigenvector comes from a cyclic Jacobi iteration (the
 * reference: the closed-form eigen33); non-finite records are neither queries nor neighbours and produce no output.  Not
 * built: the ORTHOGONAL projection (the reference's Newton loop, impl/mls.hpp:551-579, has no iteration cap), order > 2,
 * upsampling, setIndices, another search surface, cached MLS results.  Two calls give the same bytes.
 * Accuracy of out_double against an exact evaluation of 1 .. 4 on the float inputs, with kappa = max(1, trace(C) / (l1 - l0),
 * the condition number of the fit matrix with u, v in units of r) and away from kappa of about 1e10:
 *   normal (up to sign), curvature   within (m + 32) * 2^-53 * kappa, wherever the cloud lies: every intermediate is kept
 *                                    relative to q (p_j - q is exact in double, the call works with mean - q and adds q once)
 *   point                            within (m + 32) * 2^-53 * kappa * r + 2 * 2^-53 * max(|q_x|, |q_y|, |q_z|): the second
 *                                    term is the rounding of the final q + offset and of the value it is compared with; it
 *                                    matters where |q| exceeds (m + 32) * kappa * r, as in a map frame
 * The float outputs are out_double rounded once.
 * pclhip_index_last_kernel_ms gives the GPU time of the whole call, pclhip_index_last_mls_ms that of its two passes. */
enum { PCLHIP_MLS_NONE = 0, PCLHIP_MLS_SIMPLE = 1, PCLHIP_MLS_ORTHOGONAL = 2 }; /* MLSResult::ProjectionMethod */
PCLHIP_API pclhip_status pclhip_mls_process(pclhip_index* index, double search_radius, double sqr_gauss_param,
                                            int polynomial_order, int projection_method, float* out_points,
                                            float* out_normals, int32_t* out_indices, uint64_t capacity, uint64_t* n_out,
                                            double* out_double);
/* GPU time (ms) of the plane kernel and of the fit kernel (0 when it did not run) of the last pclhip_mls_process. */
PCLHIP_API void pclhip_index_last_mls_ms(const pclhip_index* index, double* plane_ms, double* fit_ms);
/* pcl::BoundaryEstimation<PointInT, PointNT, PointOutT>::computeFeature and ::isBoundaryPoint (features/include/pcl/
 * features/impl/boundary.hpp:87-137, 141-209; getCoordinateSystemOnPlane, boundary.h:161-168): search surface == input.
 * `index` is built over the whole unscaled cloud and holds normals (pclhip_normals* or pclhip_index_set_normals).
 * Per query q with normal n:
 *   1. The neighbourhood: with radius > 0 every indexed point with float d2 < float(radius * radius), q included (as
 *      pclhip_radius_search); with k >= 1 the k nearest, q included (the lists of pclhip_knn).  Fewer than
 *      max(3, min_neighbors) entries: flag 0.
 *   2. v = (nx, ny, nz, 0).unitOrthogonal() by Eigen's rule for 4-vectors (maxi the first index of the largest |component|,
 *      sndi = maxi == 0 ? 1 : 0, v[maxi] = -n[sndi] * inv, v[sndi] = n[maxi] * inv, inv = 1 / sqrt(n[sndi]^2 + n[maxi]^2)),
 *      u = n x v, in float.
 *   3. Per neighbour p: delta = p - q in float, an all-zero delta (q itself, a duplicate) is skipped; the angle is
 *      atan2f(v . delta, u . delta).  No angle left: flag 0.
 *   4. flag = (the largest difference of consecutive sorted angles, the wrap-around 2 * float(pi) - last + first
 *      included) > float(angle_threshold).
 *   out_flags          (host or device) one byte per query, 0 or 1: every record of the cloud, or indices[0..n_indices) in
 *                      that order (repeats allowed; an index out of range is PCLHIP_ERR_INVALID)
 *   out_invalid_count  (optional) the queries without a defined feature, see the deviations
 * Exactly one of radius > 0 and k >= 1 must be given: anything else is PCLHIP_ERR_INVALID, as is an angle_threshold that
 * is not finite or below pi / 8.  min_neighbors < 3 acts as 3 (the reference's rule); a keypoint detector's edge pass is
 * the same call with its own minimum.  An index without normals, or one built with `indices` or rescale values, is
 * PCLHIP_ERR_STATE.  A positive radius whose float square is 0 is a valid call in which nobody has a neighbour: every flag
 * is 0 and every query is counted invalid.
 * The flag is the reference's wherever no gap lies within rounding of the threshold: the angles are computed with the
 * reference's float operations and the decisive gap is the float difference of the same two angles; nothing is sorted and no
 * neighbour list is kept (pcl_amd/csrc/boundary.hpp).  A flag depends on the set of angles only, so two calls give the same
 * bytes.
 * Deviations: a query with no neighbour, a non-finite query and a query whose normal is non-finite or zero get flag 0 and
 * are counted in out_invalid_count (the reference stores quiet_NaN() cast to uint8_t and clears is_dense, or sorts NaN
 * angles); non-finite records are never neighbours.  Not built: angle_threshold < pi / 8, another search surface, the
 * border exclusion of ISSKeypoint3D (it is not wired to this call), a pcl_plugin.hpp class.
 * pclhip_index_last_kernel_ms gives the GPU time of the whole call, pclhip_index_last_boundary_ms that of its mask pass
 * and of its resolve passes together (k mode: of its one kernel, and 0). */
PCLHIP_API pclhip_status pclhip_boundary(pclhip_index* index, const int32_t* indices, uint64_t n_indices, double radius,
                                         int k, double angle_threshold, int min_neighbors, uint8_t* out_flags,
                                         uint64_t* out_invalid_count);
PCLHIP_API void pclhip_index_last_boundary_ms(const pclhip_index* index, double* mask_ms, double* resolve_ms);
/* How many queries of the last pclhip_boundary on this index the mask pass left to the resolve pass. */
PCLHIP_API uint64_t pclhip_index_last_boundary_resolved(const pclhip_index* index);
/* pcl::EuclideanClusterExtraction<PointT>::extract (segmentation/.../impl/extract_clusters.hpp:124-253): the clusters are
 * the connected components of the graph over the index's points with an edge wherever float d2 < float(r * r),
 * r = double(float(tolerance)) -- the relation of pclhip_radius_search.  The index defines the set of points: built with
 * `indices`, only those are clustered (the reference's (cloud, indices) overload with a tree over the same set) and the
 * ids are original ones; a scaled index clusters in its rescaled space.  A component is kept when min_size <= size <=
 * max_size; the kept clusters are ordered by size descending, ties by their smallest original index ascending (the
 * reference's std::sort leaves ties unspecified); every cluster's indices ascend.
 *   out_labels   (host or device, n_orig entries, optional) rank of the record's cluster in output order; -1 for a record
 *                in no returned cluster (non-finite, not selected, or in a cluster outside the size range)
 *   out_offsets  (HOST, optional) n_clusters + 1 entries: cluster c is out_indices[out_offsets[c] .. out_offsets[c + 1])
 *   out_indices  (host or device, optional) n_clustered entries
 * The counts are always written; a capacity that is too small gives PCLHIP_ERR_OVERFLOW after the counts and the labels
 * are written (n_orig indices and n_orig + 1 offsets always suffice).  tolerance < 0 or not finite is PCLHIP_ERR_INVALID;
 * tolerance == 0, or a positive tolerance whose float square is 0, is a valid call in which no point has a neighbour and
 * every finite point is its own cluster (:177-181).  min_size > max_size or an empty index give zero clusters.
 * The result does not depend on the order the device worked in: two calls give the same bytes.
 * Deviation: a non-finite record belongs to no cluster (the reference asserts on such a query and, in a release build,
 * makes it a singleton).
 * pclhip_index_last_kernel_ms gives the GPU time of the whole call, pclhip_index_last_cluster_stats that of its union-find
 * kernels. */
PCLHIP_API pclhip_status pclhip_euclidean_clusters(pclhip_index* index, double tolerance, uint32_t min_size,
                                                   uint32_t max_size, int32_t* out_labels, uint64_t* out_offsets,
                                                   uint64_t offsets_capacity, int32_t* out_indices,
                                                   uint64_t indices_capacity, uint64_t* n_clusters, uint64_t* n_clustered);
/* GPU time (ms) of the hook and of the flatten kernel of the last pclhip_euclidean_clusters on this index, and the number
 * of unions its hook kernel attempted (a hit under another root; depends on the order the device worked in). */
PCLHIP_API void pclhip_index_last_cluster_stats(const pclhip_index* index, double* hook_ms, double* flatten_ms,
                                                uint64_t* unions);
/* pcl::RegionGrowing<PointT, NormalT>::extract (segmentation/.../impl/region_growing.hpp:231-548) in smooth mode: the
 * segmentation of the index's points into smooth regions from normals and curvatures.  The reference floods breadth-first
 * from seeds in curvature order; the kernels (pcl_amd/csrc/region_growing.hpp) compute the same labels from an order-free
 * restatement, so two calls give the same bytes.  The index defines the set of points, as for pclhip_euclidean_clusters.
 * Segments are numbered in the order their seeds are taken (ascending curvature); those outside [min_cluster_size,
 * max_cluster_size] are dropped and the rest keeps that order; every segment's indices ascend.
 * Deviations: curvature ties are broken by the lower original index (the reference's std::sort leaves them open; -0 ties
 * with +0); k-NN ties go to the lower index; a non-finite point is in no segment, label -1 (the reference makes it a
 * segment of one); a NaN normal passes the smoothness test as in the reference (NaN < c is false).
 * Refused (PCLHIP_ERR_INVALID, with a message): residual_test != 0 (whether a point expands would depend on who reached
 * it first, i.e. on the flood's order inside a region); smooth_mode == 0; number_of_neighbours > 64 (an edge mask is one
 * 64-bit word) or < 0; a NaN curvature of an indexed point (the reference's sort has no defined order there); a NaN
 * smoothness threshold.  An index built with rescale values, or with indices that name a record twice, is
 * PCLHIP_ERR_STATE.  number_of_neighbours == 0 and an empty
 * index give zero segments (:303-304).  curvature_test == 0 (every point expands) is reachable from this interface only:
 * the reference's setter switches the residual test on with it.
 * Not built: RegionGrowingRGB, a search surface other than the input, a pcl_plugin.hpp class, multi-GPU. */
typedef struct {
  int number_of_neighbours;     /* 30 */
  float smoothness_threshold;   /* 30.0f / 180.0f * float(M_PI) */
  float curvature_threshold;    /* 0.05f */
  int curvature_test;           /* 1 */
  int smooth_mode;              /* 1 */
  int residual_test;            /* 0 */
  float residual_threshold;     /* 0.05f, stored only */
  uint32_t min_cluster_size;    /* 1 */
  uint32_t max_cluster_size;    /* UINT32_MAX */
} pclhip_region_growing_params;
PCLHIP_API void pclhip_region_growing_params_default(pclhip_region_growing_params* params);
/*   normals      (host or device) one byte-strided (nx, ny, nz, curvature) float record per ORIGINAL point
 *   out_labels, out_offsets, out_indices, the capacities and the counts: as for pclhip_euclidean_clusters -- the counts are
 *   always written, PCLHIP_ERR_OVERFLOW comes after the counts and the labels. */
PCLHIP_API pclhip_status pclhip_region_growing(pclhip_index* index, const void* normals, size_t normals_stride,
                                               const pclhip_region_growing_params* params, int32_t* out_labels,
                                               uint64_t* out_offsets, uint64_t offsets_capacity, int32_t* out_indices,
                                               uint64_t indices_capacity, uint64_t* n_clusters, uint64_t* n_clustered);
/* Of the last pclhip_region_growing on this index: the GPU time (ms) of the k-NN lists, of the collapse and of the two
 * round loops; the rounds of phase 1 (propagation) and of phase 2 (leftover points); the unions the collapse attempted
 * (depends on the order the device worked in); the number of leftover points.  Every pointer is optional. */
PCLHIP_API void pclhip_index_last_region_growing_stats(const pclhip_index* index, double* lists_ms, double* collapse_ms,
                                                       double* phase1_ms, double* phase2_ms, uint32_t* phase1_rounds,
                                                       uint32_t* phase2_rounds, uint64_t* unions, uint64_t* leftover);
/* GPU time (ms) of the last pclhip_knn / pclhip_normals traversal kernel on this index. */
PCLHIP_API double pclhip_index_last_kernel_ms(const pclhip_index* index);
/* Supply target normals computed elsewhere (e.g. a pcl::PointNormal target: normals = points + 16,
 * stride 48).  One record per ORIGINAL cloud point. */
PCLHIP_API pclhip_status pclhip_index_set_normals(pclhip_index* index, const void* normals,
                                                  size_t stride_bytes);

/* ---- ICP --------------------------------------------------------------------------------------*/
enum { PCLHIP_ICP_POINT_TO_POINT = 0, /* TransformationEstimationSVD, icp.h:149-151 */
       PCLHIP_ICP_POINT_TO_PLANE = 1, /* TransformationEstimationPointToPlaneLLS, icp.h:395-398 */
       PCLHIP_ICP_SYMMETRIC = 2       /* TransformationEstimationSymmetricPointToPlaneLLS,
                                         IterativeClosestPointWithNormals::setUseSymmetricObjective, icp.h:380-400;
                                         needs source normals too (pclhip_icp_set_source_normals) */ };

/* number of doubles in the per-iteration reduction record */
#define PCLHIP_ICP_NSUMS 32
/* layout of sums[]:
 *   point-to-plane: [0..20] upper triangle of ATA (row-major, order of impl/
 *                   transformation_estimation_point_to_plane_lls.hpp:213-233), [21..26] ATb
 *   symmetric:      same slots, for v = [(p+q) x n ; n] and rhs v ((q-p).n)
 *                   (impl/transformation_estimation_symmetric_point_to_plane_lls.hpp:161-190)
 *   point-to-point: [0..2] sum s, [3..5] sum t, [6..14] sum t_i*s_j (row-major), rest 0
 *   [27] sum of squared correspondence distances, [28] number of correspondences,
 *   [29] number of pairs skipped for non-finite normals, [30..31] reserved */

typedef struct {
  int max_iterations;                     /* registration.h:566, default 10 */
  double max_correspondence_distance;     /* registration.h:117, default sqrt(DBL_MAX) */
  double transformation_epsilon;          /* registration.h:588, default 0 */
  double transformation_rotation_epsilon; /* registration.h:592, default 0 = unset */
  double euclidean_fitness_epsilon;       /* registration.h:116, default -DBL_MAX */
  int min_number_correspondences;         /* registration.h:621, default 3 */
  int mode;                               /* PCLHIP_ICP_POINT_TO_POINT / _PLANE */
  int failure_after_max_iterations;       /* default_convergence_criteria.h:294 */
  int max_iterations_similar_transforms;  /* default_convergence_criteria.h:318 */
  double mse_threshold_absolute;          /* default_convergence_criteria.h:310, 1e-12 */
} pclhip_icp_params;

typedef struct {
  float final_transformation[16];   /* row-major 4x4 */
  float last_transformation[16];    /* transformation_ of the last iteration */
  int nr_iterations;
  int converged;
  int convergence_state;            /* DefaultConvergenceCriteria::ConvergenceState values */
  uint64_t num_correspondences;     /* of the last iteration */
  double mse;                       /* mean squared correspondence distance, last iteration */
  double gpu_ms;                    /* GPU time of all iterate launches (events on ctx stream) */
  double gpu_ms_search_kernel;      /* ... of which the search + accumulate kernels of the iterations */
} pclhip_icp_result;

/* Optional hook run on the 32-double DEVICE record of every iteration before the host reads it:
 * multi-GPU runs all-reduce (sum) it over RCCL here.  `stream` is the context's hipStream_t on
 * which the record was produced.  Return 0 on success. */
typedef int (*pclhip_allreduce_fn)(void* user, double* device_sums, int count, void* stream);

PCLHIP_API void pclhip_icp_params_default(pclhip_icp_params* p);

/* Registration object bound to a target index.  Replaces the state held by
 * pcl::IterativeClosestPoint (registration/include/pcl/registration/icp.h:98-347). */
PCLHIP_API pclhip_status pclhip_icp_create(pclhip_index* target, pclhip_icp** out);
PCLHIP_API void pclhip_icp_destroy(pclhip_icp* icp);
/* Registration::setInputSource (registration.h:195-196): uploads + kd-orders the source. */
PCLHIP_API pclhip_status pclhip_icp_set_source(pclhip_icp* icp, const void* points,
                                               size_t stride_bytes, uint64_t n);
/* The same with PCLBase::setIndices (common/include/pcl/pcl_base.h:102-125) / CorrespondenceEstimationBase::
 * setIndicesSource (registration/include/pcl/registration/correspondence_estimation.h:194): only
 * points[indices[j]] take part in the correspondence search and the estimation; correspondences still carry
 * index_query into the ORIGINAL cloud.  indices == NULL: every point.  (The registered output of align() is
 * the whole input cloud moved by the final transformation either way, impl/icp.hpp:264-267.) */
PCLHIP_API pclhip_status pclhip_icp_set_source_indexed(pclhip_icp* icp, const void* points, size_t stride_bytes,
                                                       uint64_t n, const int32_t* indices, uint64_t n_indices);
/* Normals of the source cloud, one record per source point in the order given to
 * pclhip_icp_set_source (a pcl::PointNormal source: normals = points + 16, stride 48).  Required by
 * PCLHIP_ICP_SYMMETRIC; call after pclhip_icp_set_source. */
PCLHIP_API pclhip_status pclhip_icp_set_source_normals(pclhip_icp* icp, const void* normals, size_t stride_bytes);
/* setEnforceSameDirectionNormals (icp.h:416-428), default 1 */
PCLHIP_API pclhip_status pclhip_icp_set_enforce_same_direction_normals(pclhip_icp* icp, int enforce);
PCLHIP_API pclhip_status pclhip_icp_set_allreduce(pclhip_icp* icp, pclhip_allreduce_fn fn, void* user);
/* Rewind the working copy of the source to the input cloud (start of computeTransformation). */
PCLHIP_API pclhip_status pclhip_icp_reset(pclhip_icp* icp);

/* Correspondence rejectors applied on the device between the search and the accumulation of every
 * iteration (the chain of impl/icp.hpp:187-201), in the given order:
 *   DISTANCE         registration/src/correspondence_rejection_distance.cpp:43-68      param = max distance
 *   MEDIAN_DISTANCE  registration/src/correspondence_rejection_median_distance.cpp:43-69 param = factor
 *   ONE_TO_ONE       registration/src/correspondence_rejection_one_to_one.cpp:43-66
 *   TRIMMED          registration/src/correspondence_rejection_trimmed.cpp:43-60        param = overlap ratio
 * Exact ties, whose order the reference leaves to an unstable sort, go to the lower query index.
 * Multi-GPU (pclhip_icp_set_comm / _set_allreduce): DISTANCE is per pair; MEDIAN_DISTANCE and TRIMMED cut at the one
 * cloud-global order statistic (the histograms of their selection are all-reduced: the hook / communicator sees buffers
 * of 2048 doubles besides the 32-double record); ONE_TO_ONE resolves its conflicts over the ranks by a minimum
 * all-reduce of the per-target (distance, query) keys -- with the native communicator and a sharded TARGET
 * (pclhip_icp_set_region: every rank holds the whole source, so query indices are global; 8 bytes per target point
 * travel per iteration); with source slabs or an all-reduce hook it is refused.  PRECONDITION of that mode: the keys are
 * indexed by the ORIGINAL target index, so every rank must have built its index over the same WHOLE cloud plus its own
 * subset list (pclhip_index_build(points, ..., indices = pclhip_select_region(...)), as pcl_amd.dist.ShardedTarget does) --
 * not over a cloud that holds only its slab; the first iteration checks that all ranks report the same cloud size and
 * returns PCLHIP_ERR_STATE on every rank otherwise.  A rank whose share
 * of the source is empty still issues those collectives (with zero histograms), in step with its peers.  With the SOURCE
 * cut into slabs, TRIMMED breaks exact distance ties at the cut by the rank-LOCAL query index (every rank's indices
 * restart at 0): the number of pairs kept is the single-GPU run's, which of several exactly tied pairs survive may not
 * be. */
enum { PCLHIP_REJ_DISTANCE = 0, PCLHIP_REJ_MEDIAN_DISTANCE = 1, PCLHIP_REJ_ONE_TO_ONE = 2, PCLHIP_REJ_TRIMMED = 3 };
typedef struct {
  int kind;
  double param;
  uint32_t min_correspondences; /* TRIMMED: nr_min_correspondences_ */
  uint32_t reserved;
} pclhip_rejector;
PCLHIP_API pclhip_status pclhip_icp_set_rejectors(pclhip_icp* icp, const pclhip_rejector* list, int n);
/* median found by the last MEDIAN_DISTANCE rejector (getMedianDistance()) */
PCLHIP_API double pclhip_icp_last_median_distance(const pclhip_icp* icp);
/* use_reciprocal_correspondence_ (registration.h / impl/correspondence_estimation.hpp:220-311): keep
 * (i, m) only if the nearest source point of target[m] is i again (the reference rebuilds the source tree per iteration;
 * here the source index is built once, refitted to the moved cloud and searched from its root: same answers).
 * Multi-GPU: supported when the TARGET is sharded (pclhip_icp_set_region: every rank holds the whole source), refused
 * when the source is cut into slabs. */
PCLHIP_API pclhip_status pclhip_icp_set_reciprocal(pclhip_icp* icp, int enable);

/* ---- CorrespondenceRejectorSampleConsensus: RANSAC over a rigid transform ------------------------------
 * Replaces pcl::registration::CorrespondenceRejectorSampleConsensus<PointT>::getRemainingCorrespondences
 * (registration/include/pcl/registration/impl/correspondence_rejection_sample_consensus.hpp:55-142) with
 * SampleConsensusModelRegistration (sample_consensus/.../impl/sac_model_registration.hpp:48-97,203-249,289-322,
 * sac_model_registration.h:264-289, sac_model.h:162-197) under RandomSampleConsensus (impl/ransac.hpp:56-217).
 * Input: n correspondences (index_query[j], index_match[j]) over a source and a target cloud; samples, inliers and the
 * trace speak of list positions j.  In the chain of pclhip_icp_set_rejectors (kind PCLHIP_REJ_SAMPLE_CONSENSUS) the list is
 * the pairs still kept, in ascending original query index, over the MOVED source (impl/icp.hpp:192-193).
 * Sample distance threshold (sac_model_registration.h:264-289): the nine sums of computeMeanAndCovarianceMatrix over the
 * list's finite source points (shifted by the list's first source point when that is finite) in double in a fixed order
 * that depends on n alone, the covariance formed in double and rounded once to float, pcl::eigen33's eigenvalues in the
 * reference's float order, sample_dist_thresh = (float(sqrtf(l0) + sqrtf(l1) + sqrtf(l2)) / 3.0)^2 in double.  A NaN
 * threshold (a negative eigenvalue) makes every sample bad: no model, as in the reference.
 * Trial t = 0, 1, 2, ... (sac_model.h:162-197): attempt a = 0 .. 999 draws three distinct list positions -- draw j is
 * int((n - j) * u) with u from the keyed splitmix of scp_draw.hpp over (seed, trial, attempt, slot j), placed by
 * insert_samples -- and uses them in ascending order; the sample is good (isSampleGood, :48-66) when each of the three
 * float squared edge lengths (dx dx + dy dy) + dz dz of its SOURCE points, as a double, exceeds sample_dist_thresh.  The
 * first good attempt is the trial's sample; a trial whose 1,000 attempts all fail ends the loop there ("No samples could
 * be selected", ransac.hpp:120-124).  n < 3: no model.
 * Hypothesis: pcl::umeyama(src, tgt, false) of the three pairs in double on the demeaned points, rounded once to a float
 * 4x4 T with last row (0, 0, 0, 1) (the routine of SampleConsensusPrerejective above).
 * Score (countWithinDistance / selectWithinDistance, :203-249): in float without contraction
 *   p.x = ((T00 s.x + T01 s.y) + T02 s.z) + T03 (y, z alike), e = p - t, d2 = (e.x e.x + e.z e.z) + e.y e.y;
 * the pair is an inlier iff double(d2) < threshold * threshold (a double product).  A non-finite point is never an inlier.
 * Counting and selecting use this one expression.
 * Stopping rule (ransac.hpp:154-201, sac_replay.hpp's without its skip branch), trials in order: a count > best (strict:
 * the earliest wins) becomes the model and sets k = log(1 - probability) / log(clamp(1 - (best / n)^3, DBL_EPSILON,
 * 1 - DBL_EPSILON)); ++iterations; the loop ends when iterations > k or iterations > max_iterations.
 * Result: without a trial whose count is above 0, or when the winner selects fewer than 3 pairs, the whole list remains
 * and the best transformation is the identity (:101-119); otherwise the winner's inliers remain, in the list's order
 * (:120-127), and the best transformation is the winner's T.  Two calls give the same bytes; batch_size never changes a
 * result; the chain's result is the standalone call's on the same list.
 * Deviations: the draws (the reference's rand() sequence; its samples are used in draw order); one float order without
 * contraction where the reference leaves the order of the 4x4 product and of squaredNorm to Eigen; the covariance sums
 * are double tree sums rounded once (the reference adds in float); the loop is replayed on the device, so the stopping
 * rule's log and pow are the device's; duplicate query indices in a standalone list are refused (the reference's map
 * silently keeps the last one).
 * Refused: refine != 0 (refineModel is a host loop of up to 1,000 data-dependent rounds with a median per round:
 * PCLHIP_ERR_INVALID with a message); duplicate query indices and indices outside a cloud (PCLHIP_ERR_INVALID);
 * max_iterations above 1,000,000 or negative, a threshold that is negative or NaN, a probability outside ]0, 1[
 * (PCLHIP_ERR_INVALID); the chain kind over a source whose index list (pclhip_icp_set_source_indexed) names a record
 * twice -- the same duplicate query indices, refused when the chain is applied (PCLHIP_ERR_INVALID; the other kinds take
 * such a source as before); the chain kind under multi-GPU iterations (PCLHIP_ERR_STATE).  Not built:
 * CorrespondenceRejectorSampleConsensus2D.
 *
 * In the chain: pclhip_rejector.param = inlier threshold, .min_correspondences = max_iterations, .reserved = seed;
 * probability 0.99 (the class has no setter).  Kinds 0..3 ignore `reserved` as before. */
enum { PCLHIP_REJ_SAMPLE_CONSENSUS = 4 };
typedef struct {
  double inlier_threshold;          /* correspondence_rejection_sample_consensus.h: default 0.05 */
  int max_iterations;               /* default 1000 */
  double probability;               /* default 0.99 */
  uint64_t seed;                    /* of the draws, default 0 */
  int batch_size;                   /* trials per scoring pass (<= 1024); 0 (default): 16 first, then doubling */
  int refine;                       /* setRefineModel: must be 0 */
} pclhip_rejector_sac_params;
typedef struct {
  uint64_t trials;                  /* trials the replay consumed */
  int iterations;                   /* iterations_ */
  int best_trial;                   /* the trial with the highest count; -1: none had a count above 0 */
  uint32_t best_count;              /* its count */
  uint32_t remaining;               /* pairs that remain (n without a model) */
  int has_model;                    /* 1: the winner's inliers remain; 0: the list is unchanged, T is the identity */
  int no_sample;                    /* 1: the loop ended at a trial whose 1,000 attempts found no good sample */
  uint32_t n;                       /* length of the list */
  uint32_t reserved;
  double sample_dist_thresh;
} pclhip_rejector_sac_stats;
typedef struct {                    /* one entry per consumed trial (pclhip_rejector_sac_last_trace) */
  int samples[3];                   /* ascending list positions (the last attempt's) */
  int attempts;                     /* draws of three made: 1 .. 1000 */
  int no_sample;                    /* 1: none of them was good (the transformation is zero, the count 0) */
  float transformation[16];
  uint32_t count;
} pclhip_rejector_sac_trace;
PCLHIP_API void pclhip_rejector_sac_params_default(pclhip_rejector_sac_params* p);
/* Clouds (records of stride bytes, xyz first) and lists (int32) may be host or device memory.  out_positions (optional,
 * host or device, `capacity` entries): the list positions that remain, ascending (getInliersIndices); *out_n (host) is
 * always written, a capacity that is too small gives PCLHIP_ERR_OVERFLOW after it.  out_T (optional, host): the best
 * transformation, row-major.  out_stats optional. */
PCLHIP_API pclhip_status pclhip_correspondence_rejector_sample_consensus(
    pclhip_ctx* ctx, const void* source, uint64_t n_source, size_t source_stride_bytes, const void* target,
    uint64_t n_target, size_t target_stride_bytes, const int32_t* index_query, const int32_t* index_match, uint64_t n,
    const pclhip_rejector_sac_params* params, int32_t* out_positions, uint64_t capacity, uint64_t* out_n, float out_T[16],
    pclhip_rejector_sac_stats* out_stats);
/* countWithinDistance of n_models row-major 4x4 transforms (host; rows 0..2 are used): out_counts[m] (host) pairs of the
 * list with double(d2) < threshold * threshold (exposed for tests). */
PCLHIP_API pclhip_status pclhip_rejector_sac_evaluate(pclhip_ctx* ctx, const void* source, uint64_t n_source,
                                                      size_t source_stride_bytes, const void* target, uint64_t n_target,
                                                      size_t target_stride_bytes, const int32_t* index_query,
                                                      const int32_t* index_match, uint64_t n, double threshold,
                                                      const float* transforms, int n_models, uint32_t* out_counts);
/* The trials the last pclhip_correspondence_rejector_sample_consensus of this context consumed (the first 65,536 at
 * most): *count always, the first min(capacity, *count) records to buf (host). */
PCLHIP_API pclhip_status pclhip_rejector_sac_last_trace(pclhip_ctx* ctx, pclhip_rejector_sac_trace* buf, uint64_t capacity,
                                                        uint64_t* count);
/* The last PCLHIP_REJ_SAMPLE_CONSENSUS rejector this registration applied: its best transformation (row-major; the
 * identity without a model) and its statistics.  They synchronise on their own, like pclhip_icp_last_median_distance;
 * PCLHIP_ERR_STATE when no such rejector has run. */
PCLHIP_API pclhip_status pclhip_icp_last_sac_transformation(const pclhip_icp* icp, float T[16]);
PCLHIP_API pclhip_status pclhip_icp_last_sac_stats(const pclhip_icp* icp, pclhip_rejector_sac_stats* out);

/* One iteration on the device-resident working source cloud (a search kernel and a streaming
 * accumulation kernel):
 *   cur <- T_prev * cur   (transformCloud, impl/icp.hpp:49-111 / transforms.hpp:109-123)
 *   1-NN of every cur point in the target, drop d2 > max_dist^2
 *        (CorrespondenceEstimation::determineCorrespondences, impl/correspondence_estimation.hpp:145-218)
 *   accumulate the normal system (TransformationEstimationPointToPlaneLLS::estimateRigidTransformation,
 *        impl/transformation_estimation_point_to_plane_lls.hpp:165-245) or the umeyama sums.
 * T_prev: row-major 4x4 float (identity on the first iteration, or the guess).
 * sums: PCLHIP_ICP_NSUMS doubles on the host. */
PCLHIP_API pclhip_status pclhip_icp_iterate(pclhip_icp* icp, const float T_prev[16], double max_dist,
                                            int mode, double sums[PCLHIP_ICP_NSUMS]);

/* GPU time (ms, HIP events on the context stream) of the search + accumulate kernels of the
 * last pclhip_icp_iterate call. */
PCLHIP_API double pclhip_icp_last_kernel_ms(const pclhip_icp* icp);
/* GPU time (ms) the last pclhip_icp_set_source spent ordering the source spatially (the same ordering the
 * index build applies to the target; paid once per source cloud, not per iteration). */
PCLHIP_API double pclhip_icp_source_order_ms(const pclhip_icp* icp);
/* Duration (ms) of the search kernel alone in the last pclhip_icp_iterate (the default iteration is
 * two kernels: search, then the streaming accumulation of the 6x6 / umeyama sums). */
PCLHIP_API double pclhip_icp_last_search_ms(const pclhip_icp* icp);

/* Host-side closed forms on a reduction record (exposed for the adapters and for tests):
 * 6x6 solve + constructTransformationMatrix (…point_to_plane_lls.hpp:132-163,264-268) or umeyama
 * (common/include/pcl/common/impl/eigen.hpp:675-738). */
PCLHIP_API pclhip_status pclhip_solve_transformation(const double sums[PCLHIP_ICP_NSUMS], int mode,
                                                     float T[16]);

/* The whole loop of IterativeClosestPoint::computeTransformation (impl/icp.hpp:113-268) with
 * DefaultConvergenceCriteria (impl/default_convergence_criteria.hpp:49-140).  The criteria's
 * previous-MSE memory persists across calls on the same object, as in the reference.
 * guess: row-major 4x4 or NULL. */
PCLHIP_API pclhip_status pclhip_icp_align(pclhip_icp* icp, const pclhip_icp_params* params,
                                          const float guess[16], pclhip_icp_result* result);

/* DefaultConvergenceCriteria::hasConverged (impl/default_convergence_criteria.hpp:49-140) as a host function, for
 * callers that run the loop themselves (a Registration with a foreign CorrespondenceEstimation /
 * TransformationEstimation plugged in): the same code the device loop runs.  `params` supplies the thresholds as
 * ICP sets them (impl/icp.hpp:157-161); `st` is the criteria's memory, which persists across alignments.
 * Returns 1 when the alignment ends with converged_ = true; the loop also ends whenever
 * st->convergence_state != 0 (NOT_CONVERGED). */
typedef struct {
  double prev_mse;                    /* correspondences_prev_mse_, DBL_MAX initially */
  int iterations_similar_transforms;
  int convergence_state;              /* ConvergenceState values of default_convergence_criteria.h:71-80 */
} pclhip_convergence_state;
PCLHIP_API void pclhip_convergence_init(pclhip_convergence_state* st);
PCLHIP_API int pclhip_convergence_has_converged(const pclhip_icp_params* params, pclhip_convergence_state* st,
                                                int nr_iterations, const float T[16], double mse);

/* The same loop as a stream of exactly n_steps iterations for measurements and for back-to-back registration
 * of the same clouds: Registration::align() called again and again -- when an alignment ends (converged or
 * not) the next step starts the next one from the input cloud and `guess`, on the device, without host
 * involvement.  All steps are queued on the context's stream before the first result is read; the solve,
 * final = T * final and the convergence test of every iteration run in a device kernel.  out_steps[i]
 * describes step i.  No rejectors / reciprocal correspondences (they need host decisions). */
typedef struct {
  int iteration;              /* nr_iterations_ of the running alignment after this step (0: no correspondences) */
  int convergence_state;      /* DefaultConvergenceCriteria state after this step */
  int converged;              /* the alignment ended here with converged_ = true */
  int alignment_ended;        /* this step was the last of its alignment */
  uint64_t num_correspondences;
  double mse;
  /* Three intervals from one start: the moment the previous step's closing kernel was done (the first step of a call: the
   * upload of the control block).  The chain-free loop (no rejectors, no reciprocal test, no served groups, no per-lane
   * search) takes them from stamps of the device's constant-rate counter that the step's own kernels leave: the start is
   * the exit stamp of the previous closing kernel, and each end is the entry of the NEXT kernel, so each interval includes
   * one launch latency.  Every other loop, and the chain-free one under option "step_events", brackets the kernels with
   * HIP events on the context's stream: the same bounds, plus the events' own cost. */
  float search_ms;            /* start .. the search launch is done (the accumulation kernel starts) */
  float kernels_ms;           /* start .. search + accumulation are done (the reduction kernel starts) */
  float step_ms;              /* start .. the whole step incl. reduction, (all-reduce,) solve (the closing kernel's exit) */
  float final_transformation[16];
} pclhip_icp_step;
PCLHIP_API pclhip_status pclhip_icp_run_steps(pclhip_icp* icp, const pclhip_icp_params* params,
                                              const float guess[16], int n_steps, pclhip_icp_step* out_steps);

/* ---- multi-GPU: one process per GPU, the 32-double record summed over the ranks per iteration --------
 * PCL has no multi-GPU path (gpu/containers/src/initialization.cpp:109 picks one device); the contract is
 * SURVEY.md 8(e).  A communicator wraps an RCCL (ncclComm_t) group over xGMI: rank 0 obtains an id, the
 * application distributes its 128 bytes to the other ranks by whatever means it has (MPI, a file, a socket,
 * torch.distributed's store), every rank calls pclhip_comm_create.  With a communicator attached the
 * all-reduce is issued from C on the context's stream between the reduction and the solve kernel of every
 * iteration; RCCL is bound with dlopen at first use (no link-time dependency). */
#define PCLHIP_COMM_ID_BYTES 128
typedef struct pclhip_comm pclhip_comm;
PCLHIP_API pclhip_status pclhip_comm_get_unique_id(unsigned char id[PCLHIP_COMM_ID_BYTES]);
PCLHIP_API pclhip_status pclhip_comm_create(pclhip_ctx* ctx, int rank, int nranks,
                                            const unsigned char id[PCLHIP_COMM_ID_BYTES], pclhip_comm** out);
PCLHIP_API void pclhip_comm_destroy(pclhip_comm* comm);
PCLHIP_API int pclhip_comm_rank(const pclhip_comm* comm);
PCLHIP_API int pclhip_comm_size(const pclhip_comm* comm);
/* in-place sum of `count` doubles in device memory over the ranks, on the context's stream (asynchronous) */
PCLHIP_API pclhip_status pclhip_comm_allreduce_sum_f64(pclhip_comm* comm, double* device_buf, int count);
/* attach (or detach with NULL) a communicator; replaces the pclhip_icp_set_allreduce hook when both are set */
PCLHIP_API pclhip_status pclhip_icp_set_comm(pclhip_icp* icp, pclhip_comm* comm);

/* ---- target sharding: a target cloud spread over the GPUs of a node ------------------------
 * The target is cut into n_slabs cells of a kd partition of space (recursive bisection at order statistics along
 * the widest axis: equal point counts, half-open boxes [lo, hi) that tile R^3, unbounded on the outside).  Rank g
 *   1. selects the target points of its region dilated by a margin >= max_correspondence_distance (the halo) and
 *      builds its index on them -- pclhip_index_build with that index list, so results keep ORIGINAL indices;
 *   2. holds the whole source, but serves only the points whose CURRENT position lies in its region
 *      (pclhip_icp_set_region): such a point finds its true nearest neighbour in the rank's index whenever that
 *      neighbour is within the margin, and correctly finds none within max_correspondence_distance otherwise;
 *   3. takes part in the per-iteration all-reduce of the record (pclhip_icp_set_comm); all ranks then apply the
 *      same transformation, so routing stays consistent without any other exchange.
 * Correspondences over all ranks are exactly those of a single index over the whole target.
 * Partitioning and selection are host code (no GPU needed); clouds may be host or device memory.  A cloud in DEVICE
 * memory is cut on the device (same regions and lists, bit for bit; up to 254 slabs, more fall back to the host code):
 * these two calls take no context, run on the null stream and first wait for everything queued on the device, so a
 * cloud another stream is still producing is complete when they read it.
 * regions: n_slabs x 6 floats (lo.xyz, hi.xyz), +-inf on unbounded sides. */
PCLHIP_API pclhip_status pclhip_partition_slabs(const void* points, size_t stride_bytes, uint64_t n, int n_slabs,
                                                float* regions);
/* ascending indices of the finite points inside `region` dilated by `margin` per axis (rounded outwards);
 * *out_count is always set; PCLHIP_ERR_OVERFLOW if it exceeds `capacity` */
PCLHIP_API pclhip_status pclhip_select_region(const void* points, size_t stride_bytes, uint64_t n,
                                              const float region[6], double margin, int32_t* out_indices,
                                              uint64_t capacity, uint64_t* out_count);
/* the slab whose region holds the point (x >= lo && x < hi per axis), -1 for non-finite points */
PCLHIP_API int pclhip_region_owner(const float* regions, int n_slabs, const float xyz[3]);
/* restrict the registration to the source points whose current position lies in `region`; NULL: all points.  Inside
 * pclhip_icp_align / pclhip_icp_run_steps the rank can WALK only the 64-point groups of its (kd-ordered) source copy
 * whose box touches the region -- about n / n_slabs points per iteration, not n; groups that come into reach later are
 * brought up to date from the transforms they missed, bit for bit (measured in round 4: one rank of eight of a 30M-point
 * job iterates in 0.59 ms against 1.82 ms for the full pass).  pclhip_ctx_set_option(ctx, "served_groups", 0) walks the
 * whole source copy and masks per point -- the reference the tests compare with */
PCLHIP_API pclhip_status pclhip_icp_set_region(pclhip_icp* icp, const float region[6]);
/* Largest squared distance to the k-th nearest neighbour (the point itself counts as the first, as in
 * pclhip_normals) over the indexed points inside `box` (lo.xyz, hi.xyz; NULL: all).  With a halo index this
 * tells whether the normals of the points a rank can be matched to are exact: they are when
 * sqrt(*out_max_d2) <= margin - max_correspondence_distance (every neighbour then lies inside the halo). */
PCLHIP_API pclhip_status pclhip_index_kth_distance_max(pclhip_index* index, int k, const float box[6],
                                                       double* out_max_d2);

/* Registration::getFitnessScore(max_range) (registration/include/pcl/registration/impl/registration.hpp:132-168):
 * the source is transformed by T (row-major 4x4, Transformer::se3 operation order like
 * transformPointCloud), every finite point looks up its nearest target point, and the SQUARED
 * distances that are <= max_range (compared as given, like the reference) are averaged in double.
 * *score = DBL_MAX when nothing qualifies; *nr (may be NULL) = number of points that counted.
 * Does not disturb the state of the alignment (seeds, correspondences of the last iteration). */
PCLHIP_API pclhip_status pclhip_icp_fitness_score(pclhip_icp* icp, const float T[16], double max_range,
                                                  double* score, uint64_t* nr);

/* Correspondences of the LAST iteration, materialised lazily as pcl::Correspondences
 * (common/include/pcl/correspondence.h:60-89): sorted by index_query, entries beyond max_dist
 * omitted.  With rejectors the list is the chain's output in the reference's order (ONE_TO_ONE:
 * by match index, TRIMMED: by distance).  Buffers (host or device) must hold n_source entries;
 * *out_n receives the count. */
PCLHIP_API pclhip_status pclhip_icp_fetch_correspondences(pclhip_icp* icp, int32_t* index_query,
                                                          int32_t* index_match, float* distance,
                                                          uint64_t* out_n);
/* The same list as an array of pcl::Correspondence records -- { int32 index_query; int32 index_match; float distance },
 * 12 bytes (correspondence.h:60-71) --, compacted on the device and handed over in ONE copy: what
 * CorrespondenceEstimation::determineCorrespondences leaves in its std::vector (impl/correspondence_estimation.hpp
 * :160-216: resized to the number of queries, filled, shrunk to the valid ones).  Query order only: refused (ERR_STATE)
 * when a ONE_TO_ONE or TRIMMED rejector re-orders the list.  `capacity` records at `out` (host or device); *out_n receives
 * the count, PCLHIP_ERR_OVERFLOW if it exceeds the capacity.  10M pairs through the binding
 * (CorrespondenceEstimationHIP::determineCorrespondences on host clouds): 102 -> 13.6 ms repeated, 138 -> 66 ms the first
 * time (scratch/boundary_probe.cpp). */
PCLHIP_API pclhip_status pclhip_icp_fetch_correspondence_records(pclhip_icp* icp, void* out, uint64_t capacity,
                                                                 uint64_t* out_n);

/* TransformationEstimation::estimateRigidTransformation(cloud_src, cloud_tgt, T)
 * (registration/include/pcl/registration/transformation_estimation.h:71-115) for n explicit pairs
 * (src[i], tgt[i]); `mode` selects TransformationEstimationSVD / PointToPlaneLLS (target normals) /
 * SymmetricPointToPlaneLLS (both normals).  Buffers host or device; normals may be NULL when the mode
 * does not use them.  T: row-major 4x4; sums (may be NULL): the PCLHIP_ICP_NSUMS reduction record. */
PCLHIP_API pclhip_status pclhip_estimate_rigid_transformation(
    pclhip_ctx* ctx, int mode, const void* src, size_t src_stride, const void* src_normals,
    size_t src_normals_stride, const void* tgt, size_t tgt_stride, const void* tgt_normals,
    size_t tgt_normals_stride, uint64_t n, int enforce_same_direction_normals, float T[16], double* sums);

/* TransformationEstimationPointToPlaneLLSWeighted::estimateRigidTransformation
 * (impl/transformation_estimation_point_to_plane_lls_weighted.hpp:195-290): the point-to-plane system
 * with every target normal scaled by its pair's weight (n floats, host or device). */
PCLHIP_API pclhip_status pclhip_estimate_rigid_transformation_weighted(
    pclhip_ctx* ctx, const void* src, size_t src_stride, const void* tgt, size_t tgt_stride,
    const void* tgt_normals, size_t tgt_normals_stride, const float* weights, uint64_t n, float T[16],
    double* sums);

/* out = T * in for n records (x,y,z at byte 0; other bytes of the record untouched);
 * order 0: Eigen Matrix4f*Vector4f order (icp.hpp:49-111); order 1: Transformer::se3 order
 * (transforms.hpp:117-123).  If normals_offset_bytes != 0 the 3 floats there are rotated too. */
PCLHIP_API pclhip_status pclhip_transform_cloud(pclhip_ctx* ctx, const float T[16], int order,
                                                const void* in, void* out, size_t stride_bytes,
                                                uint64_t n, size_t normals_offset_bytes);
/* The same for the SOURCE cloud of a registration: when `in` is the host buffer pclhip_icp_set_source[_indexed] was
 * given (same address, stride and count), the records staged on the device then are used and nothing is uploaded
 * again -- the moved cloud IterativeClosestPoint::computeTransformation hands back (impl/icp.hpp:264-267:
 * output = *input_, then transformCloud) costs one download.  Any other `in` behaves like pclhip_transform_cloud.
 * CONTRACT: the staged records are the cloud as it was when pclhip_icp_set_source[_indexed] was called -- like the
 * registration's own copy of the points.  A caller that edits the buffer in place (or reuses the address for another
 * cloud) must call pclhip_icp_set_source[_indexed] again before aligning or transforming, exactly as it must for the
 * alignment itself to see the change; the copy is dropped there and is never kept beyond 1/8 of the device's memory. */
PCLHIP_API pclhip_status pclhip_icp_transform_source(pclhip_icp* icp, const float T[16], int order,
                                                     const void* in, void* out, size_t stride_bytes,
                                                     uint64_t n, size_t normals_offset_bytes);

/* ---- GeneralizedIterativeClosestPoint -------------------------------------------------------------
 * Replaces pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ> with the Newton solver
 * (registration/include/pcl/registration/gicp.h, impl/gicp.hpp:370-477,480-766,768-933).  Bound to a target index;
 * the covariances (computeCovariances, impl/gicp.hpp:70-147) are computed by the first align() and cached until the
 * source is set again (source) or the object is recreated on a new index (target), or replaced by the caller's.
 * Not supported (refused by the bindings): useBFGS, source subsets (setIndices), multi-GPU. */
typedef struct pclhip_gicp pclhip_gicp;
typedef struct {
  int max_iterations;                     /* gicp.h:146, default 200 */
  double transformation_epsilon;          /* gicp.h:147, default 5e-4 */
  double rotation_epsilon;                /* gicp.h:419 rotation_epsilon_, default 2e-3 */
  double max_correspondence_distance;     /* gicp.h:148 corr_dist_threshold_, default 5 */
  int min_number_correspondences;         /* gicp.h:149, default 4 */
  int k_correspondences;                  /* gicp.h:409, default 20 (<= 32 here) */
  double gicp_epsilon;                    /* gicp.h:413, default 1e-3 */
  int max_inner_iterations;               /* gicp.h:429, default 20 */
  double translation_gradient_tolerance;  /* gicp.h:425, default 1e-2 */
  double rotation_gradient_tolerance;     /* gicp.h:427, default 1e-2 */
} pclhip_gicp_params;
typedef struct {
  float final_transformation[16];   /* row-major: previous_transformation_ * guess (impl/gicp.hpp:905) */
  float last_transformation[16];    /* transformation_ of the last outer iteration */
  int nr_iterations;                /* outer iterations */
  int converged;
  uint64_t num_correspondences;     /* pairs of the last outer iteration */
  int newton_iterations;            /* inner iterations, summed over the outer ones */
  int newton_steps;                 /* line searches run (one multi-candidate pass each) */
  int newton_steps_alpha_one;       /* ... of which accepted the full step (no gradient pass needed) */
  int eval_passes;                  /* streaming passes over the pairs (candidate + gradient passes) */
  int trace_count;                  /* entries written to the trace buffer */
  int reserved;
  double covariance_ms;             /* wall time of the covariances this call computed (0 when cached) */
  double search_ms;                 /* GPU time of the 1-NN searches (HIP events) */
  double pack_ms;                   /* ... of the pack passes (Mahalanobis matrices, cached sums) incl. their reductions */
  double eval_ms;                   /* ... of the evaluation passes incl. their reductions */
  double total_ms;                  /* wall time of the call (the rest: copies, launches, the host's serial step) */
} pclhip_gicp_result;
typedef struct {                    /* one entry per outer iteration (pclhip_gicp_set_trace) */
  uint64_t correspondences;
  int inner_iterations;
  int reserved;
  double f;                         /* the functor's value at the accepted x */
  float transformation[16];         /* transformation_ after this iteration */
} pclhip_gicp_trace;
PCLHIP_API void pclhip_gicp_params_default(pclhip_gicp_params* p);
PCLHIP_API pclhip_status pclhip_gicp_create(pclhip_index* target, pclhip_gicp** out);
PCLHIP_API void pclhip_gicp_destroy(pclhip_gicp* gicp);
/* setInputSource (gicp.h:160-166): stages the source and drops its covariances. */
PCLHIP_API pclhip_status pclhip_gicp_set_source(pclhip_gicp* gicp, const void* points, size_t stride_bytes, uint64_t n);
/* setSourceCovariances / setTargetCovariances (gicp.h:184-215): 9 doubles (row-major 3x3) per point in the cloud's
 * order, host or device; used as given. */
PCLHIP_API pclhip_status pclhip_gicp_set_source_covariances(pclhip_gicp* gicp, const double* cov, uint64_t n);
PCLHIP_API pclhip_status pclhip_gicp_set_target_covariances(pclhip_gicp* gicp, const double* cov, uint64_t n);
/* Optional per-outer-iteration record of the next alignments (NULL / 0: none); the buffer must outlive them. */
PCLHIP_API pclhip_status pclhip_gicp_set_trace(pclhip_gicp* gicp, pclhip_gicp_trace* buf, int capacity);
/* computeTransformation (impl/gicp.hpp:768-930).  guess: row-major 4x4 or NULL. */
PCLHIP_API pclhip_status pclhip_gicp_align(pclhip_gicp* gicp, const pclhip_gicp_params* params, const float guess[16],
                                          pclhip_gicp_result* result);
/* OptimizationFunctorWithIndices::dfddf (impl/gicp.hpp:612-750) on the pairs of the last outer iteration: f (the
 * functor's value), gradient g[6], Hessian H[36] row-major (exposed for tests). */
PCLHIP_API pclhip_status pclhip_gicp_evaluate(pclhip_gicp* gicp, const double x[6], double* f, double g[6], double H[36]);
/* mahalanobis_ (impl/gicp.hpp:863-865): 9 doubles per source point, original order (NaN for non-finite points). */
PCLHIP_API pclhip_status pclhip_gicp_mahalanobis(pclhip_gicp* gicp, double* out);
/* Registration::getFitnessScore (impl/registration.hpp:132-168) through pclhip_icp_fitness_score; T NULL: the final
 * transformation of the last alignment. */
PCLHIP_API pclhip_status pclhip_gicp_fitness_score(pclhip_gicp* gicp, const float T[16], double max_range, double* score,
                                                  uint64_t* nr);

/* ---- NormalDistributionsTransform -----------------------------------------------------------------
 * Replaces pcl::NormalDistributionsTransform<PointXYZ, PointXYZ> with the RADIUS neighbourhood
 * (registration/include/pcl/registration/ndt.h, impl/ndt.hpp:79-934) on the voxel Gaussians of
 * pcl::VoxelGridCovariance (filters/include/pcl/filters/impl/voxel_grid_covariance.hpp:47-367).  The voxel Gaussians and the
 * index over their centroids are built by the first call that needs them and cached until the target, the resolution,
 * min_points_per_voxel or min_covar_eigvalue_mult changes (ndt.h:121-141, 351-364).
 * Not built (PCLHIP_ERR_STATE / refused by the bindings): the DIRECT27 / 26 / 7 / 1 neighbourhoods, source subsets
 * (setIndices), multi-GPU, NormalDistributionsTransform2D. */
typedef struct pclhip_ndt pclhip_ndt;
enum { PCLHIP_NDT_RADIUS = 0, PCLHIP_NDT_DIRECT27 = 1, PCLHIP_NDT_DIRECT26 = 2, PCLHIP_NDT_DIRECT7 = 3, PCLHIP_NDT_DIRECT1 = 4 };
typedef struct {
  float resolution;                        /* ndt.h:680 resolution_, default 1.0f */
  int max_iterations;                      /* impl/ndt.hpp:76, default 35 */
  double step_size;                        /* ndt.h:683 step_size_, default 0.1 */
  double outlier_ratio;                    /* ndt.h:687 outlier_ratio_, default 0.55 */
  double transformation_epsilon;           /* impl/ndt.hpp:75, default 0.1; compared with a SQUARED translation (:190-200) */
  double transformation_rotation_epsilon;  /* registration.h, default 0 */
  double min_covar_eigvalue_mult;          /* voxel_grid_covariance.h:572, default 0.01 */
  int min_points_per_voxel;                /* voxel_grid_covariance.h:571, default 6; values below 3 count as 3 (:214-225) */
  int neighborhood_search_method;          /* PCLHIP_NDT_RADIUS (the reference's default); the others are refused */
} pclhip_ndt_params;
typedef struct {
  float final_transformation[16];   /* row-major; identity when the voxel grid holds no cell (impl/ndt.hpp:86-90) */
  float last_transformation[16];    /* transformation_: the last outer iteration's step as a matrix */
  int nr_iterations;                /* outer iterations */
  int converged;
  double score;                     /* the score at the final transformation */
  double transformation_likelihood; /* trans_likelihood_ = score / source size */
  uint64_t num_cells;               /* voxel Gaussians of the target */
  uint64_t num_pairs;               /* (point, cell) pairs of the last evaluation */
  int evaluations_full;             /* passes: score + gradient + Hessian, */
  int evaluations_gradient;         /* ... score + gradient (line-search trials), */
  int evaluations_hessian;          /* ... Hessian only (after a line search that iterated) */
  int trace_count;                  /* entries written to the trace buffer */
  double cells_ms;                  /* wall time of the voxel Gaussians + their index built by this call (0 when cached) */
  double eval_ms_full;              /* GPU time of the passes by variant, incl. their reductions (HIP events) */
  double eval_ms_gradient;
  double eval_ms_hessian;
  double total_ms;                  /* wall time of the call */
} pclhip_ndt_result;
typedef struct {                    /* one entry per outer iteration (pclhip_ndt_set_trace) */
  double step_length;               /* what computeStepLengthMT returned */
  int line_search_trials;           /* iterations of its More-Thuente loop */
  int reserved;
  double score;                     /* at the accepted step */
  float transformation[16];         /* final_transformation_ after this iteration */
} pclhip_ndt_trace;
PCLHIP_API void pclhip_ndt_params_default(pclhip_ndt_params* p);
PCLHIP_API pclhip_status pclhip_ndt_create(pclhip_ctx* ctx, pclhip_ndt** out);
PCLHIP_API void pclhip_ndt_destroy(pclhip_ndt* ndt);
/* setInputTarget / setInputSource: strided records (x y z first), host or device; the registration keeps its own copy. */
PCLHIP_API pclhip_status pclhip_ndt_set_target(pclhip_ndt* ndt, const void* points, size_t stride_bytes, uint64_t n);
PCLHIP_API pclhip_status pclhip_ndt_set_source(pclhip_ndt* ndt, const void* points, size_t stride_bytes, uint64_t n);
/* Optional per-outer-iteration record of the next alignments (NULL / 0: none); the buffer must outlive them. */
PCLHIP_API pclhip_status pclhip_ndt_set_trace(pclhip_ndt* ndt, pclhip_ndt_trace* buf, int capacity);
/* Registration::align -> computeTransformation (impl/ndt.hpp:79-207).  guess: row-major 4x4 or NULL. */
PCLHIP_API pclhip_status pclhip_ndt_align(pclhip_ndt* ndt, const pclhip_ndt_params* params, const float guess[16],
                                         pclhip_ndt_result* result);
/* One derivative pass at the transformation vector x = (tx ty tz roll pitch yaw) (computeDerivatives, impl/ndt.hpp:209-304;
 * exposed for tests).  variant 0: score, g[6] and H[36] (row-major); 1: score and gradient (H = 0); 2: computeHessian
 * (score = 0, g = 0).  pairs (optional): the (point, cell) pairs within the resolution. */
PCLHIP_API pclhip_status pclhip_ndt_evaluate(pclhip_ndt* ndt, const pclhip_ndt_params* params, const double x[6], int variant,
                                            double* score, double g[6], double H[36], uint64_t* pairs);
/* The voxel Gaussians in ascending voxel id (exposed for tests): *count always; each non-NULL host array receives one row
 * per cell when capacity >= *count (PCLHIP_ERR_OVERFLOW otherwise): centroids 3 floats, means 3 doubles, cov (the raw
 * covariance of voxel_grid_covariance.hpp:326) and icov 9 doubles row-major, point counts, voxel ids, validity (0: the
 * cell failed the eigenvalue test; it stays in the centroid cloud with a zero icov, as in the reference). */
PCLHIP_API pclhip_status pclhip_ndt_cells(pclhip_ndt* ndt, const pclhip_ndt_params* params, uint64_t* count, float* centroids,
                                         double* means, double* cov, double* icov, int32_t* npoints, int32_t* voxel_ids,
                                         uint8_t* valid, uint64_t capacity);
/* Registration::getFitnessScore (impl/registration.hpp:132-168) through pclhip_icp_fitness_score (an index over the
 * target's points is built on first use); T NULL: the final transformation of the last alignment. */
PCLHIP_API pclhip_status pclhip_ndt_fitness_score(pclhip_ndt* ndt, const float T[16], double max_range, double* score,
                                                 uint64_t* nr);

/* ---- SampleConsensusPrerejective ------------------------------------------------------------------
 * Replaces pcl::SampleConsensusPrerejective<PointXYZ, PointXYZ, FeatureT> (registration/include/pcl/registration/
 * sample_consensus_prerejective.h, impl/sample_consensus_prerejective.hpp:78-348) with its polygonal pre-rejection
 * (correspondence_rejection_poly.h:208-338) and TransformationEstimationSVD.  Bound to a target index built over the
 * whole unscaled target cloud.  Per iteration: selectSamples (:96-117), one of the k nearest target features of each
 * sample (:123-153), thresholdPolygon, umeyama on the pairs (double, demeaned), getFitness (:310-348), acceptance
 * (:284-293): float(inliers) / float(source size) >= inlier_fraction && error < lowest error -- strict, the earliest
 * iteration wins a tie; a guess that is not isApprox(Identity, 0.01f) is scored first (:233-243).
 * Deviations:
 *   - random numbers: a draw is a pure function of (seed, iteration, slot) -- splitmix64's finalizer over
 *     seed + 0x9E3779B97F4A7C15 * ((iteration << 8 | slot) + 1), u = (x >> 11) * 2^-53, index = int(n * u), which mirrors
 *     n * (rand() / (RAND_MAX + 1.0)).  Slots 0 .. nr_samples-1 are the sample draws, nr_samples .. 2 nr_samples-1 the
 *     picks among the k neighbours.  The reference's rand() sequence cannot be reproduced across libcs; with this one the
 *     result does not depend on how iterations are batched (batch_size changes nothing) and a test can replay the draws.
 *     The reference's feature-neighbour cache is an optimisation, not a semantic: it is kept as one (a source row is
 *     searched once per source / target feature set).
 *   - the error is float(sum / count) with the float d2 values summed in double in a fixed order (per 64-point group of
 *     the source's kd order a wave tree, then the groups in the order of block_sums_finalize_kernel), where the reference
 *     adds floats sequentially: they differ by at most (count + 4) * 2^-24 relative.  Two runs give the same bits.
 *   - nr_samples <= 8 (the trace record and the per-thread state hold that many); k_correspondences <= 32.
 *   - k is clamped to the number of finite target feature rows (the pick is drawn among that many); a sampled source row
 *     that is not finite has no neighbour and its hypothesis counts as rejected (the reference asserts inside FLANN); so
 *     does one whose chosen target record is not finite.
 * Not built: SampleConsensusInitialAlignment, a user-supplied transformation estimator, setIndices, multi-GPU, early
 * abandonment of a hypothesis that can no longer win, CorrespondenceRejectorPoly as a rejector of the ICP chain. */
typedef struct pclhip_scp pclhip_scp;
typedef struct {
  int max_iterations;                  /* sample_consensus_prerejective.h:128, default 5000 */
  int nr_samples;                      /* nr_samples_, default 3 (1 .. 8 here) */
  int k_correspondences;               /* k_correspondences_ ("correspondence randomness"), default 2 (<= 32 here) */
  float similarity_threshold;          /* :127, default 0.6f, in [0, 1[ */
  float inlier_fraction;               /* inlier_fraction_, default 0, in [0, 1] */
  double max_correspondence_distance;  /* registration.h corr_dist_threshold_, default sqrt(DBL_MAX) */
  uint64_t seed;                       /* of the draws (above), default 0 */
  int batch_size;                      /* iterations per batch of launches, default 2048; never changes a result */
} pclhip_scp_params;
typedef struct {
  float final_transformation[16];   /* row-major; the guess when nothing was accepted */
  int converged;
  int iterations;                   /* max_iterations */
  int rejected;                     /* iterations that did not reach getFitness (num_rejections) */
  int best_iteration;               /* the accepted iteration; -1: the guess; -2: none */
  float best_error;                 /* lowest_error (FLT_MAX when nothing was accepted) */
  uint32_t best_count;              /* inliers of the accepted hypothesis */
  int trace_count;                  /* entries written to the trace buffer */
  uint32_t knn_rows;                /* source feature rows searched by this call */
  double knn_ms, hypothesis_ms, fitness_ms;  /* GPU time of the launches by kind (HIP events) */
  double total_ms;                  /* wall time of the call */
} pclhip_scp_result;
typedef struct {                    /* one entry per iteration (pclhip_scp_set_trace) */
  int iteration;
  int rejected;                     /* 0: scored; 1: thresholdPolygon; 2: a sample without a usable match */
  int samples[8];                   /* selectSamples, ascending */
  int matches[8];                   /* the chosen target indices (-1: none) */
  float transformation[16];         /* the hypothesis (not rejected only) */
  uint32_t inliers;                 /* getFitness of it */
  float error;
} pclhip_scp_trace;
/* KdTreeFLANN<FeatureT>::nearestKSearch, exact, by brute force: the k target rows nearest to every query row under
 * FLANN's L2_Simple<float> -- in float, dimension 0 .. D-1 in order, acc = acc + diff * diff, no contraction -- in
 * ascending (d2, target index): ties go to the lower index.  Rows are D floats at the start of strided records, host or
 * device; D <= 64, 1 <= k <= 32.  A target row that holds a non-finite value is never a candidate (convertCloudToArray
 * drops it); counts[q] = min(k, finite target rows), PCLHIP_ERR_STATE when there is none; a query row that is not
 * finite gets count 0.  out_indices / out_d2: k entries per query (-1 / +inf behind the count). */
PCLHIP_API pclhip_status pclhip_feature_knn(pclhip_ctx* ctx, const void* target_rows, size_t target_stride_bytes,
                                            uint64_t n_target, const void* query_rows, size_t query_stride_bytes,
                                            uint64_t n_query, int D, int k, int32_t* out_indices, float* out_d2,
                                            uint32_t* out_counts);
PCLHIP_API void pclhip_scp_params_default(pclhip_scp_params* p);
PCLHIP_API pclhip_status pclhip_scp_create(pclhip_index* target, pclhip_scp** out);
PCLHIP_API void pclhip_scp_destroy(pclhip_scp* scp);
/* setInputSource: strided records (x y z first), host or device; the registration keeps its own copy. */
PCLHIP_API pclhip_status pclhip_scp_set_source(pclhip_scp* scp, const void* points, size_t stride_bytes, uint64_t n);
/* setSourceFeatures / setTargetFeatures (:140-160): D floats at the start of each record, one per record of the cloud,
 * in the cloud's order; copied. */
PCLHIP_API pclhip_status pclhip_scp_set_source_features(pclhip_scp* scp, const void* rows, size_t stride_bytes, uint64_t n,
                                                        int D);
PCLHIP_API pclhip_status pclhip_scp_set_target_features(pclhip_scp* scp, const void* rows, size_t stride_bytes, uint64_t n,
                                                        int D);
/* Optional per-iteration record of the next alignments (NULL / 0: none); the buffer must outlive them.  With a trace the
 * records of every batch are read back (one more synchronisation per batch). */
PCLHIP_API pclhip_status pclhip_scp_set_trace(pclhip_scp* scp, pclhip_scp_trace* buf, int capacity);
/* getFitness (:310-348) of n_transforms row-major 4x4 matrices (host) in batched launches: the source moved by T
 * (Transformer::se3 order, as pclhip_transform_cloud order 1), the 1-NN in the target per point, inlier when float
 * d2 < float(corr_dist * corr_dist); counts[h] inliers, errors[h] = float(sum / count) or FLT_MAX (exposed for tests). */
PCLHIP_API pclhip_status pclhip_scp_evaluate(pclhip_scp* scp, const pclhip_scp_params* params, const float* transforms,
                                            int n_transforms, uint32_t* counts, float* errors);
/* Registration::align -> computeTransformation (:157-306).  guess: row-major 4x4 or NULL.  PCLHIP_ERR_STATE: features
 * missing or not one per point (:161-190); PCLHIP_ERR_INVALID: inlier fraction outside [0, 1], similarity outside [0, 1[,
 * k <= 0 (:192-212), nr_samples greater than the source size (:83-90). */
PCLHIP_API pclhip_status pclhip_scp_align(pclhip_scp* scp, const pclhip_scp_params* params, const float guess[16],
                                         pclhip_scp_result* result);
/* getInliers (:240): the accepted hypothesis' inlier indices into the source, ascending; *count always, the indices when
 * capacity >= *count (PCLHIP_ERR_OVERFLOW otherwise).  out: host. */
PCLHIP_API pclhip_status pclhip_scp_inliers(pclhip_scp* scp, int32_t* out, uint64_t capacity, uint64_t* count);
/* Registration::getFitnessScore through pclhip_icp_fitness_score; T NULL: the final transformation of the last alignment. */
PCLHIP_API pclhip_status pclhip_scp_fitness_score(pclhip_scp* scp, const float T[16], double max_range, double* score,
                                                 uint64_t* nr);
/* GPU time (ms) of the feature k-NN, hypothesis and fitness launches of the last pclhip_scp_align. */
PCLHIP_API void pclhip_scp_last_ms(const pclhip_scp* scp, double* knn_ms, double* hypothesis_ms, double* fitness_ms);

/* ---- SACSegmentation: SACMODEL_PLANE with SAC_RANSAC --------------------------------------------------
 * Replaces pcl::SACSegmentation<PointT>::segment (segmentation/include/pcl/segmentation/impl/sac_segmentation.hpp:79-133)
 * for SampleConsensusModelPlane (sample_consensus/.../impl/sac_model_plane.hpp:80-118,153-230,311-360) under
 * RandomSampleConsensus (impl/ransac.hpp:56-217).  The point set is `indices` (positions into the cloud, any order,
 * repeats allowed) or every record; n = its length; samples are positions in that list.
 * Trial t = 0, 1, 2, ...: the sample is scp::select_samples(seed, t, 3, n) (the draws of SampleConsensusPrerejective
 * above); with p0, p1, p2 the points at s[0] < s[1] < s[2], in float without contraction: c = (p1 - p0) x (p2 - p0),
 * norm = sqrtf((cx cx + cy cy) + cz cz); norm < 1e-5f skips the trial; (a, b, c) = c / norm,
 * d = -((a p0x + b p0y) + c p0z).  A point is an inlier when fabsf((a x + b y) + (c z + d)) < float(threshold): strict,
 * float, the order of dist4 / dist8 (sac_model_plane.h:299-320), the one expression of counting, selecting and the
 * refined selection.  A non-finite point is never an inlier; a sample that holds one is not a skip: its trial counts 0.
 * The trials are replayed on the host in order (sac_replay.hpp): a skipped trial adds to `skipped` and ends the call at
 * 10 * max_iterations; a count > best (strict: the earliest wins) becomes the model and sets
 * k = log(1 - probability) / log(clamp(1 - (best / n)^3, DBL_EPSILON, 1 - DBL_EPSILON)); ++iterations; the call ends when
 * iterations > k or iterations > max_iterations.  No trial with a count above 0: no model (out_coeff zeroed, no inliers,
 * best_trial -1 in the stats); the outlier list is then the whole point set.
 * With optimize_coefficients and more than 3 inliers the plane is refitted to the inliers: the nine sums of
 * computeMeanAndCovarianceMatrix (shifted by the first inlier) in double in a fixed order, the covariance formed in double
 * and rounded once to float, pcl::eigen33's smallest eigenvector in the reference's float order, d = -(n . centroid) in
 * float; a non-finite result keeps the unrefined coefficients; the inliers are selected again with the result.
 * Lists hold cloud indices in the order of the point set (ascending when no indices are given); the outlier list is its
 * complement (ExtractIndices::setNegative(true)).  Outputs are host or device memory, each optional; the counts are always
 * written, a capacity that is too small gives PCLHIP_ERR_OVERFLOW after them.  Two calls give the same bytes, and
 * batch_size never changes a result.
 * Deviations: the draws; a degenerate sample counts towards the skip limit (the reference redraws it up to 1,000 times
 * inside getSamples first); the norm is a plain sqrtf (Eigen's stableNorm guards an underflow the 1e-5 test makes moot);
 * one distance expression and float(threshold) everywhere (selectWithinDistance uses Eigen's dot and compares a float with
 * a double); the refit's double tree sums replace a sequential float sum.
 * Not built: models that are not planes (the constrained and the normal plane models follow below), other methods,
 * setSamplesMaxDist, multi-GPU. */
typedef struct {
  double distance_threshold;        /* sac_segmentation.h:90, default 0.0 */
  int max_iterations;               /* default 50 */
  double probability;               /* default 0.99 */
  int optimize_coefficients;        /* default 1 */
  uint64_t seed;                    /* of the draws, default 0 */
  int batch_size;                   /* trials per scoring pass (<= 1024); 0 (default): 64 first, then doubling */
} pclhip_sac_plane_params;
typedef struct {
  uint64_t trials;                  /* trials the replay consumed (the draw counter at the end) */
  int iterations;                   /* iterations_ */
  uint32_t skipped;                 /* degenerate samples */
  int batches;                      /* scoring passes */
  int best_trial;                   /* the winner; -1: no model */
  uint32_t best_count;              /* its count (the unrefined inliers) */
  int refined;                      /* the refit replaced the coefficients */
  double count_ms;                  /* GPU time of the scoring launches (HIP events) */
  double total_ms;                  /* GPU time of the whole call */
} pclhip_sac_plane_stats;
typedef struct {                    /* one entry per consumed trial (pclhip_sac_last_trace) */
  int samples[3];                   /* ascending positions in the point set */
  int skipped;
  float coefficients[4];            /* as computed (not finite for a sample that holds a non-finite point) */
  uint32_t count;                   /* 0 for a skipped trial */
} pclhip_sac_plane_trace;
PCLHIP_API void pclhip_sac_plane_params_default(pclhip_sac_plane_params* p);
PCLHIP_API pclhip_status pclhip_sac_segment_plane(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                  const int32_t* indices, uint64_t n_indices,
                                                  const pclhip_sac_plane_params* params, float out_coeff[4],
                                                  int32_t* out_inliers, uint64_t inliers_capacity, uint64_t* out_n_inliers,
                                                  int32_t* out_outliers, uint64_t outliers_capacity,
                                                  uint64_t* out_n_outliers, pclhip_sac_plane_stats* out_stats);
/* SampleConsensusModelPlane::countWithinDistance for n_models coefficient quadruples (host) in batched passes over the
 * point set: out_counts[m] (host) points with fabsf((a x + b y) + (c z + d)) < float(threshold) (exposed for tests). */
PCLHIP_API pclhip_status pclhip_sac_plane_evaluate(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                   const int32_t* indices, uint64_t n_indices, double threshold,
                                                   const float* coeffs, int n_models, uint32_t* out_counts);
/* The trials the last pclhip_sac_segment_plane of this context consumed (the first 65,536 at most): *count always, the
 * first min(capacity, *count) records to buf (host). */
PCLHIP_API pclhip_status pclhip_sac_last_trace(pclhip_ctx* ctx, pclhip_sac_plane_trace* buf, uint64_t capacity,
                                               uint64_t* count);

/* ---- SACSegmentation: the constrained planes and SACSegmentationFromNormals ----------------------------
 * The plane models with a gate per hypothesis (sample_consensus/.../impl/sac_model_perpendicular_plane.hpp:93-119,
 * sac_model_parallel_plane.hpp:92-115, sac_model_normal_parallel_plane.hpp:48-78) and the plane scored with the points'
 * normals (impl/sac_model_normal_plane.hpp:48-101,128-162: the standard path), as pcl::SACSegmentation and
 * pcl::SACSegmentationFromNormals reach them (segmentation/.../impl/sac_segmentation.hpp:230-262,374-531).  Samples,
 * coefficients, the replay, the refit and the lists are those of the plane above; model 0 gives the bytes of
 * pclhip_sac_segment_plane.
 * Float sums of three terms have ONE order here: dot3(u, v) = (u.x v.x + u.z v.z) + u.y v.y, what a 4-lane packet
 * reduction of a Vector4f with w = 0 produces; no contraction.  normalized(v) = v / sqrtf(dot3(v, v)) when that squared
 * norm is > 0, else v itself (Eigen's normalized()).  angle(u, v) = acos(clamp(double(dot3(normalized(u), normalized(v))),
 * -1, 1)) in double, folded: a = min(a, M_PI - a) as std::min does (M_PI - a when that is smaller).
 * The gate of a hypothesis (a, b, c, d), n = (a, b, c); with eps_angle > 0 only:
 *   PERPENDICULAR_PLANE (9)         invalid when angle(axis, n) > eps_angle
 *   PARALLEL_PLANE (15)             invalid when double(fabsf(dot3(axis, normalized(n)))) > |sin(eps_angle)|
 *   NORMAL_PARALLEL_PLANE (16)      invalid when double(fabsf(dot3(axis, normalized(n)))) < |cos(eps_angle)|; and with
 *                                   eps_dist > 0: invalid when fabs(double(-d) - distance_from_origin) > eps_dist
 * (sin and cos are the host's).  A comparison with a NaN is false: such a hypothesis passes the gate and counts 0.
 * An invalid hypothesis is not a skipped trial: it is an iteration whose count is 0 (trace: skipped 0, valid 0).
 * Models 9 and 15 score with the plane's expression.  Models 11 and 16 score a point p with normal record (nx, ny, nz,
 * curvature) as
 *   d_euclid = double(fabsf(dot3(n, p) + d)),  d_normal = angle((nx, ny, nz), n),
 *   weight = normal_distance_weight * (1.0 - double(curvature)),
 *   inlier iff fabs(weight * d_normal + (1.0 - weight) * d_euclid) < distance_threshold        (all in double)
 * in counting and in both selections.  A NaN in the normal or the curvature gives a NaN distance: never an inlier.  The
 * scoring pass decides most pairs without the angle (bounds that rounding cannot cross, sac_models.hpp); its flags are
 * those of this expression with the device's double acos.  After the refit the refined coefficients pass the gate again:
 * when they fail it the inlier list is EMPTY and the coefficients stay the refined ones (sac_segmentation.hpp:117-125).
 * Refused (PCLHIP_ERR_INVALID with a message): a model type other than 0, 9, 11, 15, 16; models 11 and 16 without
 * normals; a zero axis with eps_angle > 0 for models 9, 15, 16.
 * Deviations, beyond the plane's: the double acos is the device's (the host's differs from it by ulps); the class never
 * sets an eps_dist (sac_segmentation.hpp:440-468), this interface does. */
enum {
  PCLHIP_SACMODEL_PLANE = 0,                   /* sample_consensus/model_types.h:47-65 */
  PCLHIP_SACMODEL_PERPENDICULAR_PLANE = 9,
  PCLHIP_SACMODEL_NORMAL_PLANE = 11,
  PCLHIP_SACMODEL_PARALLEL_PLANE = 15,
  PCLHIP_SACMODEL_NORMAL_PARALLEL_PLANE = 16
};
typedef struct {
  int model_type;                   /* default 0 */
  float axis[3];                    /* default 0, 0, 0 */
  double eps_angle;                 /* radians; <= 0 (default 0): no angle gate */
  double normal_distance_weight;    /* setNormalDistanceWeight, default 0.1 */
  double distance_from_origin;      /* model 16, default 0 */
  double eps_dist;                  /* model 16; <= 0 (default 0): no distance gate */
} pclhip_sac_model_params;
typedef struct {                    /* pclhip_sac_plane_trace and the gate's bit */
  int samples[3];
  int skipped;
  float coefficients[4];
  uint32_t count;                   /* 0 for a skipped and for an invalid trial */
  int valid;                        /* 0: skipped, or the hypothesis failed its gate */
} pclhip_sac_model_trace;
PCLHIP_API void pclhip_sac_model_params_default(pclhip_sac_model_params* p);
/* pclhip_sac_segment_plane for any of the five models.  normals: n records (nx, ny, nz, curvature) of
 * normals_stride_bytes (>= 16, a multiple of 4), host or device, read at the cloud's indices; null for models 0, 9, 15. */
PCLHIP_API pclhip_status pclhip_sac_segment_model(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                  const void* normals, size_t normals_stride_bytes,
                                                  const int32_t* indices, uint64_t n_indices,
                                                  const pclhip_sac_plane_params* params,
                                                  const pclhip_sac_model_params* model, float out_coeff[4],
                                                  int32_t* out_inliers, uint64_t inliers_capacity, uint64_t* out_n_inliers,
                                                  int32_t* out_outliers, uint64_t outliers_capacity,
                                                  uint64_t* out_n_outliers, pclhip_sac_plane_stats* out_stats);
/* countWithinDistance of the model for n_models coefficient quadruples (host): out_counts[m] (host; 0 for an invalid
 * hypothesis), out_valid[m] (host, optional) the gate's bit (exposed for tests). */
PCLHIP_API pclhip_status pclhip_sac_model_evaluate(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                   const void* normals, size_t normals_stride_bytes,
                                                   const int32_t* indices, uint64_t n_indices, double threshold,
                                                   const pclhip_sac_model_params* model, const float* coeffs,
                                                   int n_models, uint32_t* out_counts, uint8_t* out_valid);
/* pclhip_sac_last_trace with the gate's bit, for the last segment call of either kind of this context. */
PCLHIP_API pclhip_status pclhip_sac_last_model_trace(pclhip_ctx* ctx, pclhip_sac_model_trace* buf, uint64_t capacity,
                                                     uint64_t* count);

/* ---- SampleConsensusModelCylinder under RandomSampleConsensus --------------------------------------------
 * pcl::SampleConsensusModelCylinder<PointT, PointNT> (sample_consensus/.../impl/sac_model_cylinder.hpp:49-140,182-265,
 * 268-309,453-489, sample_consensus/src/sac_model_cylinder.cpp:42-143, common/.../distances.h:75-80, common/impl/common.hpp:
 * 58-68) run by pcl::RandomSampleConsensus (impl/ransac.hpp:56-217), and one call, pclhip_sac_cylinder_segment, that does
 * with them what SACSegmentation::segment does (segmentation/.../impl/sac_segmentation.hpp:79-133).  The segmentation
 * classes themselves still refuse model type 5 (SACMODEL_CYLINDER): the cylinder lives at the level of the model and the
 * RANSAC objects.  Coefficients: (line_pt x y z, line_dir x y z, radius).  The point set, the draws, the replay, the lists
 * and the outputs are those of pclhip_sac_segment_plane, with a sample of TWO: trial t draws scp::select_samples(seed, t,
 * 2, n), s0 < s1, and the stopping rule's exponent is 2.  Normals: one record (nx, ny, nz, curvature) per record of the
 * cloud, as for the normal plane; the curvature is not read.
 * Two orders of a float sum of three products, no contraction anywhere:
 *   dot3(u, v)  = (u.x v.x + u.z v.z) + u.y v.y     a Vector4f with w = 0 (the plane models' order, above)
 *   dot3v(u, v) = u.x v.x + (u.y v.y + u.z v.z)     an Eigen::Vector3f: Eigen's unrolled scalar reduction of size 3 splits
 *                                                   1 + 2 (stated from Eigen's redux_novec_unroller)
 * normalized3v(v) = v / sqrtf(dot3v(v, v)) when that is > 0, else v.  angle(rad) = acos(clamp(double(rad), -1, 1)) folded
 * with min(a, M_PI - a), as above.
 * The model of a sample (computeModelCoefficients, :75-140), p1, p2 the points at s0, s1 and n1, n2 their RAW normal
 * records, all as Vector4f with w = 0:
 *   w = (n1 + p1) - p2, line_dir = n1 x n2, b = dot3(n1, n2), c = dot3(n2, n2), d = dot3(n1, w), e = dot3(n2, w),
 *   denominator = dot3(line_dir, line_dir), sc = double(denominator) < 1e-8 ? 0 : (b e - c d) / denominator,
 *   line_pt = (p1 + n1) + sc n1, line_dir /= sqrtf(denominator) when denominator > 0,
 *   radius = float(0.5 * (sqrt(double(q1)) + sqrt(double(q2)))), q = dot3(x, x) / dot3(line_dir, line_dir) in float with
 *   x = line_dir x (line_pt - p).
 * The trial is SKIPPED (no iteration; the call ends at 10 * max_iterations skips) when fabsf(p1 - p2) <= FLT_EPSILON in
 * every coordinate or when double(radius) > radius_max or < radius_min (the defaults -+DBL_MAX never fire).  A non-finite
 * point or normal in the sample is not a skip: its trial counts 0.
 * The gate (isModelValid, :453-489): with eps_angle > 0 invalid when angle(dot3v(normalized3v(axis),
 * normalized3v(line_dir))) > eps_angle; invalid when radius_min is set (!= -DBL_MAX) and double(radius) < radius_min, or
 * radius_max is set and double(radius) > radius_max.  An invalid hypothesis is an iteration that counts 0, not a skip.
 * The distance of a point p with unit normal n (the normal plane's: normalized((nx, ny, nz)) in dot3's order), against
 * (line_pt, l = normalized3v(line_dir), radius), :206-221:
 *   diff = p - line_pt, dir = diff - dot3v(diff, l) l, e = fabsf(sqrtf(dot3v(dir, dir)) - radius)        (float)
 *   wed = (1.0 - normal_distance_weight) * double(e);  wed > threshold: not an inlier
 *   d_normal = angle(dot3v(n, normalized3v(dir)))
 *   inlier iff fabs(normal_distance_weight * d_normal + wed) < threshold                                  (double)
 * in counting and both selections: one function.  The weight is the plain normal_distance_weight (no curvature, :170).  A
 * zero dir or normal stays zero (dot 0, angle pi/2); a NaN anywhere is never an inlier.  The scoring pass replaces the
 * test on wed, for 0 <= normal_distance_weight <= 1, by e >= e_out with e_out the least float that fails it (the product
 * is monotone in e, so the two agree on every float); its flags are those of the function above.
 * getDistancesToModel: fabs(normal_distance_weight * d_normal + wed) for every point, without the exit; none for an
 * invalid model.
 * The refit (optimizeModelCoefficients, :268-309; src/sac_model_cylinder.cpp:42-143) runs when the coefficients pass the
 * gate and there are more than 2 inliers.  The frame: ref_dir the unit axis, ref_pt the axis point nearest the inliers'
 * centroid, u the unit vector among x / z / y picked by |ref_dir.x| < |ref_dir.y| ? (|ref_dir.x| < |ref_dir.z| ? x : z) : y
 * made orthogonal to ref_dir, v = ref_dir x u.  Unknowns (a, b, c, d, r) from (0, 0, 0, 0, radius); residual of inlier i:
 *   f_i = |(ref_pt + a u + b v - p_i) x normalized(ref_dir + c u + d v)| - |r|
 * minimised by Levenberg-Marquardt on the device in double: the sums of f^2, J^T f and J^T J over the inliers in a fixed
 * order, then a damped (H + lambda diag H) 5x5 Cholesky step, accepted when the sum of squares falls.  It stops when every
 * |g_a| <= 1e-12 sqrt(H_aa sum f^2), when a step is below 1e-12 of the unknowns' scales (|r| for a, b, r; 1 for c, d), or
 * after 100 steps.  Outputs: line_pt, the direction rounded to float and then normalized3v, |r|.  A non-finite value, a
 * Cholesky that fails at the largest damping, or no accepted step keep the unrefined coefficients (refined 0).  After the
 * refit the gate runs again: a refined cylinder that fails it gives an EMPTY inlier list and keeps the refined
 * coefficients.  Two calls give the same bytes.
 * Refused (PCLHIP_ERR_INVALID with a message): no normals, or a normals stride below 16 bytes; a zero axis with eps_angle
 * > 0; radius_min > radius_max; what pclhip_sac_segment_plane refuses.
 * Deviations, beyond the plane's: the reference minimises with Eigen's MINPACK port in float (ftol = xtol =
 * sqrt(FLT_EPSILON)), this converges past float resolution; the frame and the centroid are double; at most 100 steps
 * against 400 function evaluations; the point normals are normalised in dot3's order (the normal plane's staging); the
 * double acos and sqrt are the device's.  Not built: refineModel, setNumberOfThreads, projectPoints, doSamplesVerifyModel,
 * setSamplesMaxDist. */
typedef struct {
  double normal_distance_weight;    /* default 0.1 */
  double radius_min;                /* default -DBL_MAX: not set */
  double radius_max;                /* default DBL_MAX: not set */
  float axis[3];                    /* default 0, 0, 0 */
  double eps_angle;                 /* radians; <= 0 (default 0): no angle gate */
} pclhip_sac_cylinder_params;
typedef struct {                    /* one entry per consumed trial (pclhip_sac_last_cylinder_trace) */
  int samples[2];                   /* ascending positions in the point set */
  int skipped;
  float coefficients[7];            /* as computed */
  uint32_t count;                   /* 0 for a skipped and for an invalid trial */
  int valid;                        /* 0: skipped, or the hypothesis failed the gate */
} pclhip_sac_cylinder_trace;
PCLHIP_API void pclhip_sac_cylinder_params_default(pclhip_sac_cylinder_params* p);
/* RandomSampleConsensus::computeModel, then with params->optimize_coefficients the refit and the second selection. */
PCLHIP_API pclhip_status pclhip_sac_cylinder_segment(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                     const void* normals, size_t normals_stride_bytes,
                                                     const int32_t* indices, uint64_t n_indices,
                                                     const pclhip_sac_plane_params* params,
                                                     const pclhip_sac_cylinder_params* model, float out_coeff[7],
                                                     int32_t* out_inliers, uint64_t inliers_capacity, uint64_t* out_n_inliers,
                                                     int32_t* out_outliers, uint64_t outliers_capacity,
                                                     uint64_t* out_n_outliers, pclhip_sac_plane_stats* out_stats);
/* computeModelCoefficients of samples[0], samples[1] (cloud indices, in this order): *out_found 0 where the reference
 * returns false (out_coeff then holds what was computed). */
PCLHIP_API pclhip_status pclhip_sac_cylinder_model(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                   const void* normals, size_t normals_stride_bytes,
                                                   const int32_t samples[2], const pclhip_sac_cylinder_params* model,
                                                   float out_coeff[7], int* out_found);
/* countWithinDistance and isModelValid of n_models septuples (host): out_counts[m] (host; 0 for an invalid one),
 * out_valid[m] (host, optional). */
PCLHIP_API pclhip_status pclhip_sac_cylinder_evaluate(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                      const void* normals, size_t normals_stride_bytes,
                                                      const int32_t* indices, uint64_t n_indices, double threshold,
                                                      const pclhip_sac_cylinder_params* model, const float* coeffs,
                                                      int n_models, uint32_t* out_counts, uint8_t* out_valid);
/* selectWithinDistance: cloud indices in the order of the point set (host or device; null: the count alone). */
PCLHIP_API pclhip_status pclhip_sac_cylinder_select(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                    const void* normals, size_t normals_stride_bytes,
                                                    const int32_t* indices, uint64_t n_indices, double threshold,
                                                    const pclhip_sac_cylinder_params* model, const float coeff[7],
                                                    int32_t* out_inliers, uint64_t inliers_capacity, uint64_t* out_n_inliers);
/* getDistancesToModel: one double per entry of the point set (host or device); *out_n 0 for an invalid model. */
PCLHIP_API pclhip_status pclhip_sac_cylinder_distances(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                       const void* normals, size_t normals_stride_bytes,
                                                       const int32_t* indices, uint64_t n_indices,
                                                       const pclhip_sac_cylinder_params* model, const float coeff[7],
                                                       double* out_distances, uint64_t capacity, uint64_t* out_n);
/* optimizeModelCoefficients over `inliers` (cloud indices): out_coeff = coeff where nothing was refined; *out_refined,
 * *out_iterations (the Levenberg-Marquardt steps tried), both optional. */
PCLHIP_API pclhip_status pclhip_sac_cylinder_optimize(pclhip_ctx* ctx, const void* cloud, uint64_t n, size_t stride_bytes,
                                                      const int32_t* inliers, uint64_t n_inliers,
                                                      const pclhip_sac_cylinder_params* model, const float coeff[7],
                                                      float out_coeff[7], int* out_refined, int* out_iterations);
/* The trials the last pclhip_sac_cylinder_segment of this context consumed (the first 65,536 at most). */
PCLHIP_API pclhip_status pclhip_sac_last_cylinder_trace(pclhip_ctx* ctx, pclhip_sac_cylinder_trace* buf, uint64_t capacity,
                                                        uint64_t* count);

/* ---- VoxelGrid ----------------------------------------------------------------------------------
 * Replaces pcl::VoxelGrid<pcl::PointXYZ>::applyFilter (filters/include/pcl/filters/impl/
 * voxel_grid.hpp:597-814) with downsample_all_data and the optional pass-through filter in front of
 * the grid (setFilterFieldName + setFilterLimits + setFilterLimitsNegative, voxel_grid.h:440-476;
 * impl/voxel_grid.hpp:513-590,684-695).  `has_z_limits`: 0 = no filter; 1 = keep z inside [z_min, z_max];
 * generally bit 0 = on, bit 1 = negative (cut the points INSIDE the interval instead), bits 8..15 = 1 + position
 * of the filter field inside the record, counted in floats (0 = the z coordinate; PCLHIP_VOXELGRID_LIMITS
 * composes it).  Output: ascending voxel id, records x,y,z,1
 * (16 B).  out must hold n records; *out_n receives the count.  Returns PCLHIP_ERR_OVERFLOW when
 * the reference would refuse (:620-629). */
#define PCLHIP_VOXELGRID_LIMITS(float_index_of_field, negative) (1 | ((negative) ? 2 : 0) | (((float_index_of_field) + 1) << 8))
PCLHIP_API pclhip_status pclhip_voxelgrid(pclhip_ctx* ctx, const void* points, size_t stride_bytes,
                                          uint64_t n, const float leaf[3], uint32_t min_points_per_voxel,
                                          int has_z_limits, double z_min, double z_max,
                                          void* out_xyzw, uint64_t* out_n);

/* The same for records that carry normals and for setDownsampleAllData (filters/include/pcl/filters/voxel_grid.h
 * :293-302, impl/voxel_grid.hpp:790-809).  Input and output records share a layout: x y z at +0 and, when
 * normals_offset != 0 (pcl::PointNormal: 16, strides 48), normal[3], 0, curvature, 0 0 0 at +normals_offset.
 *   downsample_all_data != 0: the CentroidPoint accumulators of common/include/pcl/common/impl/accumulators.hpp
 *        :68-127 -- coordinates averaged, normal = normalised sum of the voxel's normals, curvature averaged;
 *   downsample_all_data == 0: only the coordinates are averaged, every other field of the output keeps its
 *        default (0).
 * Sums run in ascending input index inside a voxel.  out must hold n records of out_stride bytes. */
PCLHIP_API pclhip_status pclhip_voxelgrid_ex(pclhip_ctx* ctx, const void* points, size_t stride_bytes, uint64_t n,
                                             const float leaf[3], uint32_t min_points_per_voxel, int has_z_limits,
                                             double z_min, double z_max, int downsample_all_data,
                                             size_t normals_offset, void* out, size_t out_stride_bytes,
                                             uint64_t* out_n);

/* The grid of a filter run: getMinBoxCoordinates / getMaxBoxCoordinates / getNrDivisions / getDivisionMultiplier
 * (filters/include/pcl/filters/voxel_grid.h:326-344).  Cell (i, j, k) has the id
 * (i - min_b[0]) * divb_mul[0] + (j - min_b[1]) * divb_mul[1] + (k - min_b[2]) * divb_mul[2]. */
typedef struct pclhip_voxelgrid_dims {
  int32_t min_b[3];
  int32_t max_b[3];
  int32_t div_b[3];
  int32_t divb_mul[3];
} pclhip_voxelgrid_dims;

/* pclhip_voxelgrid_ex plus setSaveLeafLayout (voxel_grid.h:316, impl/voxel_grid.hpp:752-787): leaf_layout (host
 * or device, may be NULL) receives, for every cell id, the position of that voxel's centroid in the output or -1
 * for a cell that is empty or was dropped by min_points_per_voxel; it must hold div_b[0]*div_b[1]*div_b[2] ints
 * (leaf_layout_capacity is checked).  dims (may be NULL) receives the grid.  Call pclhip_voxelgrid_grid first to
 * learn how many cells the layout has. */
PCLHIP_API pclhip_status pclhip_voxelgrid_ex2(pclhip_ctx* ctx, const void* points, size_t stride_bytes, uint64_t n,
                                              const float leaf[3], uint32_t min_points_per_voxel, int has_z_limits,
                                              double z_min, double z_max, int downsample_all_data,
                                              size_t normals_offset, void* out, size_t out_stride_bytes,
                                              uint64_t* out_n, int32_t* leaf_layout, uint64_t leaf_layout_capacity,
                                              pclhip_voxelgrid_dims* dims);

/* Only the grid the filter would use for this cloud (bounding box pass, impl/voxel_grid.hpp:613-645). */
PCLHIP_API pclhip_status pclhip_voxelgrid_grid(pclhip_ctx* ctx, const void* points, size_t stride_bytes, uint64_t n,
                                               const float leaf[3], int has_z_limits, double z_min, double z_max,
                                               pclhip_voxelgrid_dims* dims);

/* ---- PCD files (io/src/pcd_io.cpp: PCDReader :115-675, PCDWriter :848-1500) ----------------------
 * The on-disk format either side of the path.  ascii, binary and binary_compressed (LZF, fields stored
 * as struct of arrays) are read straight into the strided records the calls above consume.  Errors are
 * reported through pclhip_last_error(NULL). */
typedef struct {
  uint64_t points;       /* POINTS */
  uint32_t width, height;
  int data_type;         /* 0 ascii, 1 binary, 2 binary_compressed */
  int version;           /* 7 when a VIEWPOINT line is present, else 6 */
  uint32_t point_step;   /* bytes per point in the file */
  uint32_t num_fields;
  int has_xyz, has_normals, has_curvature, has_intensity, has_rgb;
  float viewpoint[7];    /* tx ty tz qw qx qy qz */
  uint64_t data_offset;  /* byte offset of the body */
} pclhip_pcd_info;

/* PCDReader::readHeader */
PCLHIP_API pclhip_status pclhip_pcd_read_header(const char* path, pclhip_pcd_info* info);
/* pcl::io::loadPCDFile into records of stride_bytes: x,y,z at +0 (and 1.0f at +12 when the record has
 * room, like PointXYZ); if normals_offset != 0 and the file has normal_x/y/z they go to +normals_offset
 * (3 floats, then 0.0f, then curvature at +normals_offset+16 when the file has it and the record has
 * room -- the PointNormal layout with normals_offset = 16, stride 48).  float64 / integer fields are
 * converted.  points: host or device memory holding `capacity` records; *n_out = POINTS (also when the
 * buffer is too small: PCLHIP_ERR_OVERFLOW); *is_dense as the reference computes it. */
PCLHIP_API pclhip_status pclhip_pcd_read(const char* path, void* points, size_t stride_bytes,
                                         size_t normals_offset, uint64_t capacity, uint64_t* n_out,
                                         int* is_dense);
/* pcl::io::savePCDFile{ASCII,Binary,BinaryCompressed}: unorganized cloud of n records (x y z, plus
 * normal_x normal_y normal_z [curvature] when normals_offset != 0); precision: significant digits of the
 * ascii writer (<= 0: the reference's default 8). */
PCLHIP_API pclhip_status pclhip_pcd_write(const char* path, const void* points, size_t stride_bytes,
                                          size_t normals_offset, uint64_t n, int data_type, int precision);
/* The same for an organized cloud (width x height records, row-major) with an acquisition pose
 * (VIEWPOINT tx ty tz qw qx qy qz; NULL = 0 0 0 1 0 0 0). */
PCLHIP_API pclhip_status pclhip_pcd_write_organized(const char* path, const void* points, size_t stride_bytes,
                                                    size_t normals_offset, uint32_t width, uint32_t height,
                                                    const float viewpoint[7], int data_type, int precision);
/* One component of any field of the file (e.g. "intensity", "curvature", "normal_x") as float32, one value
 * per point, into HOST memory.  float64 / integer fields are converted; 4-byte "rgb" / "rgba" keep their
 * 32 bits (PCL packs colours into a float). */
PCLHIP_API pclhip_status pclhip_pcd_read_field(const char* path, const char* field, uint32_t component,
                                               float* out, uint64_t capacity, uint64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* PCLHIP_H_ */
