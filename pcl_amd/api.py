"""Python mirror of the PCL plugin surface for the ICP hot path, over the C ABI (include/pclhip.h).

Class and method names follow the reference so parity tests read like PCL's own tests:
  pcl::search::KdTree<PointT>                         search/include/pcl/search/kdtree.h:61-168
  pcl::registration::CorrespondenceEstimation          registration/include/pcl/registration/correspondence_estimation.h
  pcl::IterativeClosestPoint / ...WithNormals          registration/include/pcl/registration/icp.h:98-347,360-440
  pcl::NormalEstimation                                features/include/pcl/features/normal_3d.h:243-420
  pcl::FPFHEstimation                                  features/include/pcl/features/fpfh.h:79-222
  pcl::ISSKeypoint3D                                   keypoints/include/pcl/keypoints/iss_3d.h
  pcl::MovingLeastSquares (no upsampling)              surface/include/pcl/surface/mls.h
  pcl::BoundaryEstimation                              features/include/pcl/features/boundary.h
  pcl::VoxelGrid                                       filters/include/pcl/filters/voxel_grid.h:221-533
  pcl::EuclideanClusterExtraction                      segmentation/include/pcl/segmentation/extract_clusters.h:330-435
  pcl::registration::CorrespondenceRejectorSampleConsensus  registration/.../correspondence_rejection_sample_consensus.h
  pcl::SACSegmentation (planes, RANSAC)                segmentation/include/pcl/segmentation/sac_segmentation.h:77-330
Clouds are (n, c>=3) float32 arrays: numpy (host) or torch CUDA tensors (device-resident; only the
pointer crosses the boundary).  All compute happens in libpclhip.so; there is no CPU fallback.
"""
import ctypes as C
import os
import math

import numpy as np

from . import _lib
from ._lib import POINT_TO_PLANE, POINT_TO_POINT, IcpParams, IcpResult, check

_SQRT_DBL_MAX = math.sqrt(np.finfo(np.float64).max)


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _cloud(a):
    """-> (pointer, stride_bytes, n, keepalive)."""
    if _is_torch(a):
        assert a.dtype.is_floating_point and a.element_size() == 4 and a.dim() == 2 and a.shape[1] >= 3
        a = a.contiguous()
        return C.c_void_p(a.data_ptr()), a.shape[1] * 4, a.shape[0], a
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] >= 3
    return C.c_void_p(a.ctypes.data), a.shape[1] * 4, a.shape[0], a


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Context:
    """One device + one HIP stream (pclhip_ctx)."""

    def __init__(self, device=0, stream=None):
        """stream=None: the context creates its own non-blocking stream.  Any integer -- including 0,
        the legacy default stream torch reports as current_stream().cuda_stream -- is ADOPTED as given,
        so work the caller orders on that stream (collectives, copies) stays ordered with the kernels."""
        self.lib = _lib.load()
        h = C.c_void_p()
        if stream is None:
            check(self.lib.pclhip_ctx_create(int(device), None, C.byref(h)))
        else:
            check(self.lib.pclhip_ctx_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(h)))
        self.h = h
        self.device = device
        self.stream = int(self.lib.pclhip_ctx_stream(h) or 0)
        self._children = []  # weakrefs to objects holding handles that point into this context

    def _adopt(self, obj):
        import weakref
        self._children.append(weakref.ref(obj))

    def synchronize(self):
        check(self.lib.pclhip_ctx_synchronize(self.h), self.h)

    def reserve(self, nbytes):
        """Reserve the context's device arena up front (pclhip_ctx_reserve); automatic for the first large cloud otherwise."""
        check(self.lib.pclhip_ctx_reserve(self.h, int(nbytes)), self.h)

    def setOption(self, name, value):
        """pclhip_ctx_set_option: "served_groups", "icp_lookahead", "step_events", "cache_mb", "arena_mb", "lane_search", "lane_max_up",
        "lane_far" (none changes a result)."""
        check(self.lib.pclhip_ctx_set_option(self.h, name.encode(), float(value)), self.h)

    def stats(self, enable=True):
        """Read (then re-arm or disable) the traversal work counters."""
        out = (C.c_uint64 * 8)()
        check(self.lib.pclhip_ctx_stats(self.h, int(enable), out), self.h)
        names = ("nodes", "leaves_group", "leaves_allpairs", "pushes", "groups", "so_done", "so_list", "so_union")
        return {n: int(out[i]) for i, n in enumerate(names)}

    def counters(self, enable=True):
        """The same eight counters as a plain list (the per-lane search kernels of lane.hip count in them too: 0 queries,
        1 done with their own leaf, 2 done in the first pass, 3 greedy descents, 4 finished by the second pass)."""
        out = (C.c_uint64 * 8)()
        check(self.lib.pclhip_ctx_stats(self.h, int(enable), out), self.h)
        return [int(v) for v in out]

    def close(self):
        if getattr(self, "h", None):
            # handles hold a raw pointer to the context: release them first, whatever order the
            # interpreter finalises objects in
            for ref in self._children:
                obj = ref()
                if obj is not None:
                    obj._release()
            self._children = []
            self.lib.pclhip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Communicator:
    """pclhip_comm: an RCCL group (one rank per GPU/process) for the per-iteration all-reduce of the record.
    `unique_id()` on rank 0, distribute the 128 bytes (e.g. torch.distributed.broadcast_object_list over gloo,
    MPI, a file), then Communicator(ctx, rank, nranks, id) on every rank."""

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
        check(_lib.load().pclhip_comm_get_unique_id(buf))
        return bytes(buf)

    def __init__(self, ctx, rank, nranks, uid):
        self.ctx = ctx
        self.lib = ctx.lib
        assert len(uid) == _lib.COMM_ID_BYTES
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        check(self.lib.pclhip_comm_create(ctx.h, int(rank), int(nranks), buf, C.byref(h)), ctx.h)
        self.h = h
        self.rank, self.size = int(rank), int(nranks)
        ctx._adopt(self)

    def allreduce_sum_f64(self, device_ptr, count):
        check(self.lib.pclhip_comm_allreduce_sum_f64(self.h, C.c_void_p(int(device_ptr)), int(count)), self.ctx.h)

    def _release(self):
        if getattr(self, "h", None):
            if self.ctx.h is not None:
                self.lib.pclhip_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class KdTree:
    """pcl::search::KdTree<PointT> backed by the GPU kd-ordered wide BVH (pclhip_index)."""

    def __init__(self, ctx=None, sorted_results=True):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.h = None
        self._cloud_id = None
        self._cloud = None
        self._indices = None
        self.n_cloud = 0
        self._sorted = bool(sorted_results)
        self._epsilon = 0.0
        self.ctx._adopt(self)

    def _release(self):
        self._free()

    # search/include/pcl/search/search.h:96-142, search/kdtree.h:110-143
    def getName(self):
        return "KdTree"

    def getInputCloud(self):
        return self._cloud

    def getIndices(self):
        return self._indices

    def setSortedResults(self, sorted_results):
        """search.h:104-110: results always come back ascending by distance here, which satisfies either setting."""
        self._sorted = bool(sorted_results)

    def getSortedResults(self):
        return self._sorted

    def setEpsilon(self, eps):
        """search/kdtree.h:130-143: FLANN's (1 + eps) approximate search; this index always answers exactly."""
        self._epsilon = float(eps)

    def getEpsilon(self):
        return self._epsilon

    def setInputCloud(self, cloud, indices=None):
        # search/include/pcl/search/impl/kdtree.hpp:87-97 -> kdtree_flann.hpp:99-136: ALWAYS rebuilds, like
        # the reference (the array may have been modified in place since the last call).  Callers that know
        # the cloud is unchanged keep the tree and pass it with setSearchMethodTarget(tree, True).
        self._cloud, self._indices = cloud, indices
        key = (id(cloud), None if indices is None else id(indices))
        self._free()
        ptr, stride, n, keep = _cloud(cloud)
        h = C.c_void_p()
        ind = None if indices is None else np.ascontiguousarray(indices, np.int32)
        scale = getattr(self, "_scale", None)
        check(self.lib.pclhip_index_build_scaled(self.ctx.h, ptr, stride, n,
                                                 None if ind is None else C.c_void_p(ind.ctypes.data),
                                                 0 if ind is None else len(ind),
                                                 None if scale is None else _fp(scale), C.byref(h)), self.ctx.h)
        self.h = h
        self._cloud_id = key
        self._keep = (cloud, indices)
        self.n_cloud = n
        return True

    def setPointRepresentation(self, rescale_values=None, dimensions=3):
        """pcl::search::KdTree::setPointRepresentation (search/include/pcl/search/kdtree.h:110) for the
        representations the 3-D index can honour: the first `dimensions` of (x, y, z), each times its rescale
        value (CustomPointRepresentation(dimensions) + setRescaleValues, common/include/pcl/point_representation.h
        :150-190,546-579).  None / 3 = the default representation.  Takes effect at the next setInputCloud."""
        if rescale_values is None and dimensions == 3:
            self._scale = None
            return
        assert 1 <= dimensions <= 3, "the index is three-dimensional: only prefixes of (x, y, z)"
        sc = np.zeros(3, np.float32)
        rv = np.ones(dimensions, np.float32) if rescale_values is None else np.asarray(rescale_values, np.float32)
        assert rv.shape == (dimensions,)
        sc[:dimensions] = rv
        self._scale = sc

    def kthDistanceMax(self, k, box=None):
        """pclhip_index_kth_distance_max: the largest k-th-neighbour distance (not squared) over the indexed
        points inside `box` (lo.xyz, hi.xyz; None: all)."""
        out = C.c_double(0.0)
        b = None if box is None else np.ascontiguousarray(box, np.float32).reshape(6)
        check(self.lib.pclhip_index_kth_distance_max(self.h, int(k), _fp(b) if b is not None else None, C.byref(out)),
              self.ctx.h)
        return math.sqrt(out.value)

    def size(self):
        return int(self.lib.pclhip_index_size(self.h))

    def build_ms(self):
        return float(self.lib.pclhip_index_build_ms(self.h))

    def order(self):
        """pclhip_index_order: original index of the point at every position of the index's kd order (int32 array)."""
        out = np.empty(self.size(), np.int32)
        if len(out):
            check(self.lib.pclhip_index_order(self.h, C.c_void_p(out.ctypes.data)), self.ctx.h)
        return out

    def cells(self, level):
        """pclhip_index_cells: (boxes [n,6], cells [n,6], top level) of one quad level of the per-lane search structure."""
        cnt, top = C.c_uint64(0), C.c_int(0)
        check(self.lib.pclhip_index_cells(self.h, int(level), None, None, 0, C.byref(cnt), C.byref(top)), self.ctx.h)
        boxes = np.empty((cnt.value, 6), np.float32)
        cells = np.empty((cnt.value, 6), np.float32)
        check(self.lib.pclhip_index_cells(self.h, int(level), C.c_void_p(boxes.ctypes.data), C.c_void_p(cells.ctypes.data),
                                          cnt.value, C.byref(cnt), C.byref(top)), self.ctx.h)
        return boxes, cells, top.value

    def lastKernelMs(self):
        return float(self.lib.pclhip_index_last_kernel_ms(self.h))

    def nearestKSearch(self, queries, k, out=None):
        """Batch overload (search.h:216-219).  Returns (indices int32 [nq,k], sqr_distances [nq,k])."""
        ptr, stride, nq, keep = _cloud(queries)
        if _is_torch(queries):
            import torch
            idx = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
            d2 = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
            check(self.lib.pclhip_knn(self.h, ptr, stride, nq, int(k), C.c_void_p(idx.data_ptr()),
                                      C.c_void_p(d2.data_ptr())), self.ctx.h)
            return idx, d2
        idx = np.empty((nq, k), np.int32)
        d2 = np.empty((nq, k), np.float32)
        check(self.lib.pclhip_knn(self.h, ptr, stride, nq, int(k), C.c_void_p(idx.ctypes.data),
                                  C.c_void_p(d2.ctypes.data)), self.ctx.h)
        return idx, d2

    def gicpCovariances(self, k=20, epsilon=0.001):
        """GeneralizedIterativeClosestPoint::computeCovariances (impl/gicp.hpp:70-147) for the indexed cloud:
        (n, 3, 3) float64, NaN for points that are not in the index."""
        out = np.empty((self.n_cloud, 9), np.float64)
        check(self.lib.pclhip_gicp_covariances(self.h, int(k), float(epsilon), C.c_void_p(out.ctypes.data)), self.ctx.h)
        return out.reshape(self.n_cloud, 3, 3)

    def radiusSearch(self, queries, radius, max_nn=0):
        """Batch radiusSearch (search.h:271-273 / search.hpp:164-190).  Returns (offsets uint64 [nq+1],
        indices int32 [total], sqr_distances float32 [total]) -- neighbours of query i are
        indices[offsets[i]:offsets[i+1]], ascending by distance."""
        ptr, stride, nq, keep = _cloud(queries)
        offsets = np.zeros(nq + 1, np.uint64)
        total = C.c_uint64(0)
        optr = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
        st = self.lib.pclhip_radius_search(self.h, ptr, stride, nq, float(radius), int(max_nn), optr, None, None, 0,
                                           C.byref(total))
        if st not in (0, -5):
            check(st, self.ctx.h)
        n = int(total.value)
        idx = np.empty(n, np.int32)
        d2 = np.empty(n, np.float32)
        if n:
            check(self.lib.pclhip_radius_search(self.h, ptr, stride, nq, float(radius), int(max_nn), optr,
                                                C.c_void_p(idx.ctypes.data), C.c_void_p(d2.ctypes.data), n,
                                                C.byref(total)), self.ctx.h)
        return offsets, idx, d2

    def setNormals(self, normals):
        ptr, stride, n, keep = _cloud(normals)
        assert n == self.n_cloud
        check(self.lib.pclhip_index_set_normals(self.h, ptr, stride), self.ctx.h)

    def _free(self):
        if getattr(self, "h", None):
            if self.ctx.h is not None:
                self.lib.pclhip_index_destroy(self.h)
            self.h = None
            self._cloud_id = None

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


class NormalEstimation:
    """pcl::NormalEstimation<PointInT, pcl::Normal> with setKSearch (k-NN mode) or setRadiusSearch."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.tree = None
        self.k = 0
        self.radius = 0.0
        self.vp = np.zeros(3, np.float32)  # sensor_origin_ default (normal_3d.h:328-351)
        self.cloud = None
        self.surface = None
        self.indices = None
        self.nan_count = 0

    def setInputCloud(self, cloud):
        self.cloud = cloud

    def setSearchSurface(self, cloud):
        """Feature::setSearchSurface (features/include/pcl/features/feature.h:139-153): neighbours are taken from this
        cloud, normals are computed at the input cloud's points (None: surface == input)."""
        self.surface = cloud

    def getSearchSurface(self):
        return self.surface

    def setIndices(self, indices):
        """PCLBase::setIndices (common/include/pcl/pcl_base.h:102-125): one normal per input[indices[j]]."""
        self.indices = None if indices is None else np.ascontiguousarray(indices, np.int32)

    def setSearchMethod(self, tree):
        self.tree = tree

    def getSearchMethod(self):
        return self.tree

    def getKSearch(self):
        return self.k

    def getRadiusSearch(self):
        return self.radius

    def getViewPoint(self):
        return tuple(float(v) for v in self.vp)

    def setKSearch(self, k):
        self.k = int(k)

    def setRadiusSearch(self, radius):
        self.radius = float(radius)

    def setViewPoint(self, x, y, z):
        self.vp = np.asarray([x, y, z], np.float32)

    def compute(self, want_output=True):
        """-> (n,4) float32 [nx,ny,nz,curvature]; also retains the normals inside the tree."""
        # Feature::initCompute (impl/feature.hpp:131-155): exactly one of k and radius must be set
        if self.radius != 0.0 and self.k != 0:
            raise ValueError("Both radius (%f) and K (%d) defined! Set one of them to zero first" % (self.radius, self.k))
        if self.radius == 0.0 and self.k == 0:
            raise ValueError("Neither radius nor K defined! Set one of them to a positive number first")
        if self.tree is None:
            self.tree = KdTree(self.ctx)
        if self.surface is not None or self.indices is not None:
            return self._compute_at(want_output)
        # feature.hpp:125-130 sets the search surface on the tree.  A tree the caller has already built
        # on this very cloud object is reused (setSearchMethod(tree) after tree.setInputCloud(cloud), the
        # common PCL idiom, would otherwise build twice).
        if self.tree.h is None or self.tree._cloud_id != (id(self.cloud), None):
            self.tree.setInputCloud(self.cloud)
        n = self.tree.n_cloud
        nan = C.c_uint64(0)
        out = None
        optr, stride = None, 0
        if want_output:
            stride = 16
            if _is_torch(self.cloud):
                import torch
                out = torch.empty((n, 4), dtype=torch.float32, device=self.cloud.device)
                optr = C.c_void_p(out.data_ptr())
            else:
                out = np.empty((n, 4), np.float32)
                optr = C.c_void_p(out.ctypes.data)
        if self.k > 0:
            check(self.lib.pclhip_normals(self.tree.h, self.k, _fp(self.vp), optr, stride, C.byref(nan)), self.ctx.h)
        else:
            check(self.lib.pclhip_normals_radius(self.tree.h, self.radius, _fp(self.vp), optr, stride, C.byref(nan)),
                  self.ctx.h)
        self.nan_count = int(nan.value)
        return out


    def _compute_at(self, want_output):
        """search surface != input and / or an index subset of the input (impl/feature.hpp:104-130,
        impl/normal_3d.hpp:48-95): the tree indexes the surface, every (selected) input point is a query."""
        surface = self.surface if self.surface is not None else self.cloud
        if self.tree.h is None or self.tree._cloud_id != (id(surface), None):
            self.tree.setInputCloud(surface)
        base, stride, nq, _keep = _cloud(self.cloud)
        m = nq if self.indices is None else len(self.indices)
        if _is_torch(self.cloud):
            import torch
            out = torch.empty((m, 4), dtype=torch.float32, device=self.cloud.device)
            optr = C.c_void_p(out.data_ptr())
        else:
            out = np.empty((m, 4), np.float32)
            optr = C.c_void_p(out.ctypes.data)
        nan = C.c_uint64(0)
        ind = None if self.indices is None else C.c_void_p(self.indices.ctypes.data)
        check(self.lib.pclhip_normals_at(self.tree.h, base, stride, nq, ind, 0 if self.indices is None else m, self.k,
                                         self.radius, _fp(self.vp), optr, 16, C.byref(nan)), self.ctx.h)
        self.nan_count = int(nan.value)
        return out if want_output else None


class CorrespondenceRejectorDistance:
    """pcl::registration::CorrespondenceRejectorDistance (correspondence_rejection_distance.h)."""
    kind = _lib.REJ_DISTANCE

    def __init__(self):
        self.param, self.min_corr = 0.0, 0

    def setMaximumDistance(self, d):
        self.param = float(d)

    def getMaximumDistance(self):
        return self.param


class CorrespondenceRejectorMedianDistance:
    """pcl::registration::CorrespondenceRejectorMedianDistance."""
    kind = _lib.REJ_MEDIAN_DISTANCE

    def __init__(self):
        self.param, self.min_corr = 1.0, 0
        self.median_distance_ = None

    def setMedianFactor(self, f):
        self.param = float(f)

    def getMedianFactor(self):
        return self.param

    def getMedianDistance(self):
        return self.median_distance_


class CorrespondenceRejectorOneToOne:
    """pcl::registration::CorrespondenceRejectorOneToOne."""
    kind = _lib.REJ_ONE_TO_ONE

    def __init__(self):
        self.param, self.min_corr = 0.0, 0


class CorrespondenceRejectorTrimmed:
    """pcl::registration::CorrespondenceRejectorTrimmed."""
    kind = _lib.REJ_TRIMMED

    def __init__(self):
        self.param, self.min_corr = 0.5, 0

    def setOverlapRatio(self, r):
        self.param = float(r)

    def getOverlapRatio(self):
        return self.param

    def setMinCorrespondences(self, n):
        self.min_corr = int(n)

    def getMinCorrespondences(self):
        return self.min_corr


class CorrespondenceRejectorSampleConsensus:
    """pcl::registration::CorrespondenceRejectorSampleConsensus<PointT> (correspondence_rejection_sample_consensus.h,
    impl/correspondence_rejection_sample_consensus.hpp:55-142): RANSAC over the rigid transform of three pairs, the
    semantics of include/pclhip.h.  Standalone through getRemainingCorrespondences(index_query, index_match), or as a
    member of a rejector chain (IterativeClosestPoint.addCorrespondenceRejector, CorrespondenceEstimation.
    determineCorrespondences(rejectors=...)): there param / min_corr / seed travel in the chain's record, and
    getBestTransformation() / lastStats() are filled from the registration afterwards."""
    kind = _lib.REJ_SAMPLE_CONSENSUS

    def __init__(self, ctx=None):
        self._ctx = ctx
        self.param, self.min_corr, self.seed = 0.05, 1000, 0   # inlier threshold, max_iterations, seed of the draws
        self._batch = 0
        self._save_inliers = False
        self._src = self._tgt = None
        self._best = np.eye(4, dtype=np.float32)
        self._inliers = np.zeros(0, np.int32)
        self._stats = None
        self._list = (np.zeros(0, np.int32), np.zeros(0, np.int32))

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def getClassName(self):
        return "CorrespondenceRejectorSampleConsensus"

    def setInputSource(self, cloud):
        self._src = cloud

    def getInputSource(self):
        return self._src

    def setInputTarget(self, cloud):
        self._tgt = cloud

    def getInputTarget(self):
        return self._tgt

    def setInlierThreshold(self, threshold):
        self.param = float(threshold)

    def getInlierThreshold(self):
        return self.param

    def setMaximumIterations(self, max_iterations):
        """correspondence_rejection_sample_consensus.h:177: negative values clamp to 0"""
        self.min_corr = max(int(max_iterations), 0)

    def getMaximumIterations(self):
        return self.min_corr

    def setRefineModel(self, refine):
        if refine:
            raise NotImplementedError("CorrespondenceRejectorSampleConsensus.setRefineModel(True) is not built: refineModel "
                                      "is a host loop of up to 1,000 data-dependent rounds with a median per round")

    def getRefineModel(self):
        return False

    def setSaveInliers(self, save):
        self._save_inliers = bool(save)

    def getSaveInliers(self):
        return self._save_inliers

    def setSeed(self, seed):
        """the seed of the draws (32 bits: it travels in pclhip_rejector.reserved when the object sits in a chain)"""
        self.seed = int(seed) & 0xFFFFFFFF

    def setBatchSize(self, batch):
        """trials per scoring pass of the standalone call (0: 16 first, then doubling); never changes a result"""
        self._batch = int(batch)

    def setInputCorrespondences(self, index_query, index_match):
        """CorrespondenceRejector::setInputCorrespondences: the list evaluate() and getCorrespondences() work on"""
        self._list = (np.ascontiguousarray(index_query, np.int32).reshape(-1).copy(),
                      np.ascontiguousarray(index_match, np.int32).reshape(-1).copy())

    def getCorrespondences(self):
        """CorrespondenceRejector::getCorrespondences: the input list through getRemainingCorrespondences"""
        return self.getRemainingCorrespondences(*self._list)

    def _lists(self, index_query, index_match):
        if index_query is None:
            index_query, index_match = self._list
        else:
            self.setInputCorrespondences(index_query, index_match)
        q = np.ascontiguousarray(index_query, np.int32).reshape(-1)
        m = np.ascontiguousarray(index_match, np.int32).reshape(-1)
        if len(q) != len(m):
            raise ValueError("CorrespondenceRejectorSampleConsensus: index_query and index_match differ in length")
        assert self._src is not None and self._tgt is not None, "setInputSource / setInputTarget first"
        return q, m, _cloud(self._src), _cloud(self._tgt)

    def getRemainingCorrespondences(self, index_query, index_match):
        """-> (index_query, index_match) of the correspondences that remain, in the list's order."""
        q, m, (sp, ss, sn, sk), (tp, ts, tn, tk) = self._lists(index_query, index_match)
        lib = self.ctx.lib
        p = _lib.RejectorSacParams()
        lib.pclhip_rejector_sac_params_default(C.byref(p))
        p.inlier_threshold, p.max_iterations, p.seed, p.batch_size = self.param, self.min_corr, self.seed, self._batch
        pos = np.empty(max(len(q), 1), np.int32)
        T = np.zeros(16, np.float32)
        n_out = C.c_uint64(0)
        st = _lib.RejectorSacStats()
        check(lib.pclhip_correspondence_rejector_sample_consensus(
            self.ctx.h, sp, sn, ss, tp, tn, ts, C.c_void_p(q.ctypes.data), C.c_void_p(m.ctypes.data), len(q), C.byref(p),
            C.c_void_p(pos.ctypes.data), len(q), C.byref(n_out), _fp(T), C.byref(st)), self.ctx.h)
        pos = pos[:int(n_out.value)].copy()
        self._fill(T, st)
        self._inliers = pos if (self._save_inliers and st.has_model) else np.zeros(0, np.int32)
        return q[pos], m[pos]

    def _fill(self, T, st):
        self._best = np.array(T, np.float32).reshape(4, 4)
        self._stats = dict(trials=int(st.trials), iterations=int(st.iterations), best_trial=int(st.best_trial),
                           best_count=int(st.best_count), remaining=int(st.remaining), has_model=bool(st.has_model),
                           no_sample=bool(st.no_sample), n=int(st.n), sample_dist_thresh=float(st.sample_dist_thresh))

    def _fill_from_chain(self, lib, ctx, h):
        T = np.zeros(16, np.float32)
        st = _lib.RejectorSacStats()
        if lib.pclhip_icp_last_sac_transformation(h, _fp(T)) == -4:  # PCLHIP_ERR_STATE: the chain has not run (no source point)
            return
        check(lib.pclhip_icp_last_sac_transformation(h, _fp(T)), ctx.h)
        check(lib.pclhip_icp_last_sac_stats(h, C.byref(st)), ctx.h)
        self._fill(T, st)

    def getBestTransformation(self):
        """(4, 4) float32: the winner's transformation; the identity when no model was found."""
        return self._best.copy()

    def getInliersIndices(self):
        """positions in the input list of the correspondences that remain (setSaveInliers(True); empty without a model)"""
        return self._inliers.copy()

    def lastStats(self):
        """dict of the last run: trials, iterations, best_trial, best_count, remaining, has_model, no_sample, n,
        sample_dist_thresh."""
        return self._stats

    def evaluate(self, transforms, index_query=None, index_match=None):
        """countWithinDistance of (H, 4, 4) transforms over the list (given, or the last one this object saw) ->
        (H,) uint32."""
        q, m, (sp, ss, sn, sk), (tp, ts, tn, tk) = self._lists(index_query, index_match)
        M = np.ascontiguousarray(transforms, np.float32).reshape(-1, 16)
        cnt = np.zeros(len(M), np.uint32)
        check(self.ctx.lib.pclhip_rejector_sac_evaluate(
            self.ctx.h, sp, sn, ss, tp, tn, ts, C.c_void_p(q.ctypes.data), C.c_void_p(m.ctypes.data), len(q),
            float(self.param), _fp(M), len(M), C.c_void_p(cnt.ctypes.data)), self.ctx.h)
        return cnt

    def trace(self, capacity=65536):
        """One dict per trial the last getRemainingCorrespondences() consumed: samples, attempts, no_sample,
        transformation (4, 4), count."""
        lib = self.ctx.lib
        n = C.c_uint64(0)
        check(lib.pclhip_rejector_sac_last_trace(self.ctx.h, None, 0, C.byref(n)), self.ctx.h)
        k = min(int(n.value), int(capacity))
        buf = (_lib.RejectorSacTrace * max(1, k))()
        check(lib.pclhip_rejector_sac_last_trace(self.ctx.h, buf, k, C.byref(n)), self.ctx.h)
        return [dict(samples=list(t.samples), attempts=int(t.attempts), no_sample=bool(t.no_sample),
                     transformation=np.array(t.transformation, np.float32).reshape(4, 4), count=int(t.count))
                for t in buf[:k]]


def _set_filters(lib, ctx, h, rejectors, reciprocal):
    arr = (_lib.Rejector * max(len(rejectors), 1))()
    for i, r in enumerate(rejectors):
        arr[i].kind, arr[i].param, arr[i].min_correspondences = r.kind, r.param, r.min_corr
        arr[i].reserved = getattr(r, "seed", 0)   # SampleConsensus: the seed of its draws
    check(lib.pclhip_icp_set_rejectors(h, arr, len(rejectors)), ctx.h)
    check(lib.pclhip_icp_set_reciprocal(h, int(bool(reciprocal))), ctx.h)


def _read_filters(lib, ctx, h, rejectors):
    """what the chain's last application left for the rejector objects' getters (each reader synchronises)"""
    for r in rejectors:
        if r.kind == _lib.REJ_MEDIAN_DISTANCE:
            r.median_distance_ = float(lib.pclhip_icp_last_median_distance(h))
        elif r.kind == _lib.REJ_SAMPLE_CONSENSUS:
            r._fill_from_chain(lib, ctx, h)


class CorrespondenceEstimation:
    """pcl::registration::CorrespondenceEstimation (determineCorrespondences only)."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.tree = KdTree(self.ctx)
        self.icp = None
        self.src = None

    def setInputTarget(self, cloud):
        self._target = cloud
        self.tree.setInputCloud(cloud, getattr(self, "_tgt_indices", None))

    def setSearchMethodTarget(self, tree, force_no_recompute=False):
        self.tree = tree

    def setInputSource(self, cloud):
        self.src = cloud

    def setIndicesSource(self, indices):
        """correspondence_estimation.h:194: the source points to find correspondences for"""
        self._src_indices = None if indices is None else np.ascontiguousarray(indices, np.int32)

    def setIndicesTarget(self, indices):
        """correspondence_estimation.h:210: the target points correspondences may go to (the tree is rebuilt on
        them, impl/correspondence_estimation.hpp:82-91)"""
        self._tgt_indices = None if indices is None else np.ascontiguousarray(indices, np.int32)
        if getattr(self, "_target", None) is not None:
            self.tree.setInputCloud(self._target, self._tgt_indices)

    def determineReciprocalCorrespondences(self, max_distance=_SQRT_DBL_MAX):
        """impl/correspondence_estimation.hpp:220-311."""
        return self.determineCorrespondences(max_distance, reciprocal=True)

    def determineCorrespondences(self, max_distance=_SQRT_DBL_MAX, rejectors=(), reciprocal=False):
        """-> (index_query, index_match, distance) sorted by index_query (after `rejectors`: in the
        order the reference's chain leaves them)."""
        ptr, stride, n, keep = _cloud(self.src)
        h = C.c_void_p()
        check(self.lib.pclhip_icp_create(self.tree.h, C.byref(h)), self.ctx.h)
        try:
            ind = getattr(self, "_src_indices", None)
            if ind is None:
                check(self.lib.pclhip_icp_set_source(h, ptr, stride, n), self.ctx.h)
            else:
                check(self.lib.pclhip_icp_set_source_indexed(h, ptr, stride, n, C.c_void_p(ind.ctypes.data), len(ind)),
                      self.ctx.h)
            _set_filters(self.lib, self.ctx, h, list(rejectors), reciprocal)
            I = np.eye(4, dtype=np.float32).reshape(16)
            sums = np.zeros(_lib.NSUMS, np.float64)
            check(self.lib.pclhip_icp_iterate(h, _fp(I), float(max_distance), POINT_TO_POINT,
                                              sums.ctypes.data_as(C.POINTER(C.c_double))), self.ctx.h)
            q = np.empty(n, np.int32)
            m = np.empty(n, np.int32)
            d = np.empty(n, np.float32)
            cnt = C.c_uint64(0)
            check(self.lib.pclhip_icp_fetch_correspondences(
                h, C.c_void_p(q.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(d.ctypes.data),
                C.byref(cnt)), self.ctx.h)
            c = int(cnt.value)
            assert c == int(sums[28])
            _read_filters(self.lib, self.ctx, h, rejectors)
            return q[:c].copy(), m[:c].copy(), d[:c].copy()
        finally:
            self.lib.pclhip_icp_destroy(h)


class DefaultConvergenceCriteria:
    """pcl::registration::DefaultConvergenceCriteria (default_convergence_criteria.h:61-286) as a view of a
    registration's parameter block: hasConverged() itself runs on the device (closed_forms.hpp)."""

    def __init__(self, reg):
        self._reg = reg

    def setMaximumIterationsSimilarTransforms(self, n):
        self._reg.p.max_iterations_similar_transforms = int(n)

    def getMaximumIterationsSimilarTransforms(self):
        return int(self._reg.p.max_iterations_similar_transforms)

    def setFailureAfterMaximumIterations(self, f):
        self._reg.p.failure_after_max_iterations = int(bool(f))

    def getFailureAfterMaximumIterations(self):
        return bool(self._reg.p.failure_after_max_iterations)

    def setAbsoluteMSE(self, mse):
        self._reg.p.mse_threshold_absolute = float(mse)

    def getAbsoluteMSE(self):
        return float(self._reg.p.mse_threshold_absolute)

    # the remaining thresholds are overwritten from the registration's own setters at every align()
    # (impl/icp.hpp:157-161): the getters show what the loop will use
    def getMaximumIterations(self):
        return int(self._reg.p.max_iterations)

    def getRelativeMSE(self):
        return float(self._reg.p.euclidean_fitness_epsilon)

    def getTranslationThreshold(self):
        return float(self._reg.p.transformation_epsilon)

    def getRotationThreshold(self):
        e = float(self._reg.p.transformation_rotation_epsilon)
        return e if e > 0 else 0.99999

    def getConvergenceState(self):
        return self._reg.getConvergenceState()


class IterativeClosestPoint:
    """pcl::IterativeClosestPoint<PointXYZ, PointXYZ> (TransformationEstimationSVD)."""
    MODE = POINT_TO_POINT
    ORDER = 0

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.p = IcpParams()
        self.lib.pclhip_icp_params_default(C.byref(self.p))
        self.p.mode = self.MODE
        self.tree = KdTree(self.ctx)
        self.h = None
        self.src = None
        self.src_normals = None
        self.target = None
        self._target_updated = False
        self._force_no_recompute = False
        self._src_dirty = True
        self._src_nrm_dirty = True
        self.result = None
        self._allreduce = None
        self.rejectors = []
        self.use_reciprocal = False
        self.ctx._adopt(self)

    def _release(self):
        self._drop_icp()

    # --- setters named after registration.h:276-415 ---
    def setInputTarget(self, cloud):
        """Registration::setInputTarget (impl/registration.hpp:53-66): remembers the cloud and flags it as
        updated; the tree is (re)built by the next align()/iterate() -- always, even for the same array
        object (it may have been modified in place), unless setSearchMethodTarget(tree, True) said not to."""
        self.target = cloud
        self._target_updated = True
        self._drop_icp()

    def setSearchMethodTarget(self, tree, force_no_recompute=False):
        """registration.h:214-221: with force_no_recompute the caller vouches that `tree` already indexes the
        target, and it is never rebuilt here."""
        self.tree = tree
        self._force_no_recompute = bool(force_no_recompute)
        if force_no_recompute:
            self._target_updated = False
        self._drop_icp()

    def setInputSource(self, cloud):
        """Registration::setInputSource (registration.h:195-196): every call marks the source as new (the
        device copy is refreshed by the next align()/iterate())."""
        self.src = cloud
        self._src_dirty = True
        self.src_normals = None   # a cloud without normals must not inherit the previous cloud's

    def setIndices(self, indices):
        """PCLBase::setIndices (common/include/pcl/pcl_base.h:102-125): only these source points take part in
        the correspondence search and the estimation; None = all points."""
        self._src_indices = None if indices is None else np.ascontiguousarray(indices, np.int32)
        self._src_dirty = True

    def setMaximumIterations(self, n):
        self.p.max_iterations = int(n)

    def setMaxCorrespondenceDistance(self, d):
        self.p.max_correspondence_distance = float(d)

    def setTransformationEpsilon(self, e):
        self.p.transformation_epsilon = float(e)

    def setTransformationRotationEpsilon(self, e):
        self.p.transformation_rotation_epsilon = float(e)

    def setEuclideanFitnessEpsilon(self, e):
        self.p.euclidean_fitness_epsilon = float(e)

    # --- getters of registration.h:190-330 ---
    def getClassName(self):
        return type(self).__name__

    def getInputSource(self):
        return self.src

    def getInputTarget(self):
        return self.target

    def getSearchMethodTarget(self):
        return self.tree

    def setSearchMethodSource(self, tree, force_no_recompute=False):
        """registration.h:230-250: the reciprocal search's tree over the source.  The device indexes the moving
        source itself every iteration; the object is kept for the getter."""
        self._tree_source = tree

    def getSearchMethodSource(self):
        return getattr(self, "_tree_source", None)

    def getMaximumIterations(self):
        return int(self.p.max_iterations)

    def getMaxCorrespondenceDistance(self):
        return float(self.p.max_correspondence_distance)

    def getTransformationEpsilon(self):
        return float(self.p.transformation_epsilon)

    def getTransformationRotationEpsilon(self):
        return float(self.p.transformation_rotation_epsilon)

    def getEuclideanFitnessEpsilon(self):
        return float(self.p.euclidean_fitness_epsilon)

    def setRANSACIterations(self, n):
        """registration.h:300-322: stored; IterativeClosestPoint does not use them (nor does the reference's)."""
        self._ransac_iterations = int(n)

    def getRANSACIterations(self):
        return getattr(self, "_ransac_iterations", 0)

    def setRANSACOutlierRejectionThreshold(self, t):
        self._inlier_threshold = float(t)

    def getRANSACOutlierRejectionThreshold(self):
        return getattr(self, "_inlier_threshold", 0.05)

    def getConvergeCriteria(self):
        """icp.h:180-184: the DefaultConvergenceCriteria options a caller reaches through the criteria object."""
        return DefaultConvergenceCriteria(self)

    def addCorrespondenceRejector(self, rejector):
        """Registration::addCorrespondenceRejector (registration.h:430-434)."""
        self.rejectors.append(rejector)
        self._filters_dirty = True

    def getCorrespondenceRejectors(self):
        return list(self.rejectors)

    def removeCorrespondenceRejector(self, i):
        """registration.h:536-544: False when there is no i-th rejector."""
        if i < 0 or i >= len(self.rejectors):
            return False
        del self.rejectors[i]
        self._filters_dirty = True
        return True

    def clearCorrespondenceRejectors(self):
        self.rejectors = []
        self._filters_dirty = True

    def getUseReciprocalCorrespondences(self):
        return self.use_reciprocal

    def setUseReciprocalCorrespondences(self, on):
        """icp.h:251-256."""
        self.use_reciprocal = bool(on)
        self._filters_dirty = True

    def setAllReduce(self, fn):
        """fn(device_ptr:int, count:int, stream:int) -> 0 ; sums the 32 doubles across ranks."""
        def tramp(user, ptr, count, stream):
            try:
                return int(fn(ptr, count, stream) or 0)
            except Exception:  # never raise through the C frame
                import traceback
                traceback.print_exc()
                return 1
        self._allreduce = _lib.ALLREDUCE_FN(tramp)
        if self.h:
            check(self.lib.pclhip_icp_set_allreduce(self.h, self._allreduce, None), self.ctx.h)

    def setCommunicator(self, comm):
        """Multi-GPU: sum the per-iteration record over the ranks of `comm` (a Communicator: RCCL over xGMI,
        issued from C on the context's stream).  None detaches."""
        self._comm = comm
        if self.h:
            check(self.lib.pclhip_icp_set_comm(self.h, comm.h if comm is not None else None), self.ctx.h)

    def setRegion(self, region):
        """Target sharding (pclhip_icp_set_region): only the source points whose CURRENT position lies in
        `region` = (lo.xyz, hi.xyz), half-open, take part on this rank.  None: all points."""
        self._region = None if region is None else np.ascontiguousarray(region, np.float32).reshape(6)
        if self.h:
            check(self.lib.pclhip_icp_set_region(self.h, _fp(self._region) if self._region is not None else None), self.ctx.h)

    def runSteps(self, n_steps, guess=None):
        """pclhip_icp_run_steps: exactly n_steps iterations queued back to back on the device, alignments
        restarting on convergence.  Returns the list of per-step dicts."""
        self._ensure()
        arr = (_lib.IcpStep * max(int(n_steps), 1))()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(16)
        check(self.lib.pclhip_icp_run_steps(self.h, C.byref(self.p), _fp(g) if g is not None else None, int(n_steps),
                                            arr), self.ctx.h)
        out = []
        for i in range(int(n_steps)):
            s = arr[i]
            out.append({"iteration": s.iteration, "state": _lib.CONVERGENCE_STATES[s.convergence_state],
                        "converged": bool(s.converged), "alignment_ended": bool(s.alignment_ended),
                        "num_correspondences": int(s.num_correspondences), "mse": float(s.mse),
                        "search_ms": float(s.search_ms), "kernels_ms": float(s.kernels_ms),
                        "step_ms": float(s.step_ms),
                        "final_transformation": np.array(s.final_transformation, np.float32).reshape(4, 4)})
        return out

    def _drop_icp(self):
        if getattr(self, "h", None):
            if self.ctx.h is not None:
                self.lib.pclhip_icp_destroy(self.h)
            self.h = None
        self._src_dirty = True
        self._src_nrm_dirty = True
        self._filters_dirty = True

    def _init_target(self):
        # Registration::initCompute (impl/registration.hpp:84-87)
        if self._target_updated and not self._force_no_recompute:
            self.tree.setInputCloud(self.target)
            self._after_target_build()
            self._target_updated = False
            self._drop_icp()
        if self.tree.h is None:
            raise ValueError("No input target dataset was given!")

    def _after_target_build(self):
        pass

    def _ensure(self):
        self._init_target()
        if self.src is None:
            raise ValueError("No input source dataset was given!")
        if self.h is None:
            h = C.c_void_p()
            check(self.lib.pclhip_icp_create(self.tree.h, C.byref(h)), self.ctx.h)
            self.h = h
            if self._allreduce is not None:
                check(self.lib.pclhip_icp_set_allreduce(self.h, self._allreduce, None), self.ctx.h)
            if getattr(self, "_comm", None) is not None:
                check(self.lib.pclhip_icp_set_comm(self.h, self._comm.h), self.ctx.h)
            if getattr(self, "_region", None) is not None:
                check(self.lib.pclhip_icp_set_region(self.h, _fp(self._region)), self.ctx.h)
        if self._src_dirty:
            ptr, stride, n, keep = _cloud(self.src)
            ind = getattr(self, "_src_indices", None)
            if ind is None:
                check(self.lib.pclhip_icp_set_source(self.h, ptr, stride, n), self.ctx.h)
            else:
                check(self.lib.pclhip_icp_set_source_indexed(self.h, ptr, stride, n, C.c_void_p(ind.ctypes.data), len(ind)),
                      self.ctx.h)
            self._src_dirty = False
            self._src_nrm_dirty = True
        if self.src_normals is not None and self._src_nrm_dirty:
            nptr, nstride, nn, _keep = _cloud(self.src_normals)
            assert nn == _cloud(self.src)[2], "one normal per source point"
            check(self.lib.pclhip_icp_set_source_normals(self.h, nptr, nstride), self.ctx.h)
        self._src_nrm_dirty = False
        self._apply_options()
        if getattr(self, "_filters_dirty", True):
            _set_filters(self.lib, self.ctx, self.h, self.rejectors, self.use_reciprocal)
            self._filters_dirty = False

    def _apply_options(self):
        pass

    def iterate(self, T_prev=None, max_dist=None):
        """One device iteration (search + accumulate kernels); returns the 32-double reduction record."""
        self._ensure()
        T = np.eye(4, dtype=np.float32) if T_prev is None else np.ascontiguousarray(T_prev, np.float32)
        sums = np.zeros(_lib.NSUMS, np.float64)
        md = self.p.max_correspondence_distance if max_dist is None else float(max_dist)
        check(self.lib.pclhip_icp_iterate(self.h, _fp(T.reshape(16)), md, self.MODE,
                                          sums.ctypes.data_as(C.POINTER(C.c_double))), self.ctx.h)
        self._read_sac_rejectors()
        return sums

    def _read_sac_rejectors(self):
        sac = [r for r in self.rejectors if r.kind == _lib.REJ_SAMPLE_CONSENSUS]
        if sac:
            _read_filters(self.lib, self.ctx, self.h, sac)

    def reset(self):
        self._ensure()
        check(self.lib.pclhip_icp_reset(self.h), self.ctx.h)

    def lastKernelMs(self):
        """search + (filters) + accumulate kernels of the last iterate(), HIP events"""
        return float(self.lib.pclhip_icp_last_kernel_ms(self.h))

    def sourceOrderMs(self):
        """GPU time the last source upload spent on the spatial ordering (once per source cloud)"""
        self._ensure()
        return float(self.lib.pclhip_icp_source_order_ms(self.h))

    def lastSearchMs(self):
        """the search kernel alone"""
        return float(self.lib.pclhip_icp_last_search_ms(self.h))

    def solve(self, sums):
        T = np.zeros(16, np.float32)
        s = np.ascontiguousarray(sums, np.float64)
        check(self.lib.pclhip_solve_transformation(s.ctypes.data_as(C.POINTER(C.c_double)), self.MODE,
                                                   _fp(T)))
        return T.reshape(4, 4)

    def fetchCorrespondences(self):
        n = _cloud(self.src)[2]
        q = np.empty(n, np.int32)
        m = np.empty(n, np.int32)
        d = np.empty(n, np.float32)
        cnt = C.c_uint64(0)
        check(self.lib.pclhip_icp_fetch_correspondences(
            self.h, C.c_void_p(q.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(d.ctypes.data),
            C.byref(cnt)), self.ctx.h)
        c = int(cnt.value)
        return q[:c].copy(), m[:c].copy(), d[:c].copy()

    def align(self, guess=None, want_output=False):
        """Registration::align (registration.hpp:170-221).  Returns the registered source when
        want_output, else None; results via getFinalTransformation()/hasConverged()."""
        self._ensure()
        r = IcpResult()
        g = None
        if guess is not None:
            g = np.ascontiguousarray(guess, np.float32).reshape(16)
        check(self.lib.pclhip_icp_align(self.h, C.byref(self.p), _fp(g) if g is not None else None,
                                        C.byref(r)), self.ctx.h)
        self.result = r
        if r.nr_iterations > 0 or r.num_correspondences > 0:
            self._read_sac_rejectors()
        if want_output:
            return self.transformCloud(self.src, self.getFinalTransformation())
        return None

    def transformCloud(self, cloud, T):
        ptr, stride, n, keep = _cloud(cloud)
        Tm = np.ascontiguousarray(T, np.float32).reshape(16)
        if _is_torch(cloud):
            out = keep.clone()
            optr = C.c_void_p(out.data_ptr())
        else:
            out = keep.copy()
            optr = C.c_void_p(out.ctypes.data)
        check(self.lib.pclhip_transform_cloud(self.ctx.h, _fp(Tm), self.ORDER, ptr, optr, stride, n, 0),
              self.ctx.h)
        return out

    def getFinalTransformation(self):
        return np.array(self.result.final_transformation, np.float32).reshape(4, 4)

    def getFitnessScore(self, max_range=float(np.finfo(np.float64).max), transform=None):
        """Registration::getFitnessScore (impl/registration.hpp:132-168): mean squared 1-NN distance
        of the source moved by the final transformation (or `transform`), over the points whose
        squared distance is <= max_range; DBL_MAX when none qualifies."""
        self._ensure()
        T = self.getFinalTransformation() if transform is None else transform
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        score = C.c_double(0.0)
        nr = C.c_uint64(0)
        check(self.lib.pclhip_icp_fitness_score(self.h, _fp(T), C.c_double(max_range), C.byref(score),
                                                C.byref(nr)), self.ctx.h)
        self.fitness_points = int(nr.value)
        return float(score.value)

    def getLastIncrementalTransformation(self):
        return np.array(self.result.last_transformation, np.float32).reshape(4, 4)

    def hasConverged(self):
        return bool(self.result.converged)

    def getConvergenceState(self):
        return _lib.CONVERGENCE_STATES[self.result.convergence_state]

    @property
    def nr_iterations_(self):
        return int(self.result.nr_iterations)

    def __del__(self):
        try:
            self._drop_icp()
        except Exception:
            pass


class IterativeClosestPointWithNormals(IterativeClosestPoint):
    """pcl::IterativeClosestPointWithNormals<PointNormal, PointNormal>
    (TransformationEstimationPointToPlaneLLS, icp.h:395-398).  Target normals come either from
    setInputTarget(cloud with >= 7 columns: x,y,z,_,nx,ny,nz) or from setTargetNormals()/a
    NormalEstimation run on the same KdTree."""
    MODE = POINT_TO_PLANE
    ORDER = 1

    def setInputTarget(self, cloud):
        super().setInputTarget(cloud)
        self._target_normals = None

    def _after_target_build(self):
        # pcl::PointNormal layout: normal at floats 4..6 (point_types.hpp:843-853)
        if self.target is not None and self.target.shape[1] >= 7:
            self.tree.setNormals(self.target[:, 4:7])
        if getattr(self, "_target_normals", None) is not None:
            self.tree.setNormals(self._target_normals)

    def setTargetNormals(self, normals):
        """Normals for the target given separately (one row per target point)."""
        self._target_normals = normals
        if self.tree.h is not None and not self._target_updated:
            self.tree.setNormals(normals)

    def setInputSource(self, cloud):
        super().setInputSource(cloud)
        if cloud.shape[1] >= 7:  # pcl::PointNormal source: its normals feed the symmetric objective
            self.src_normals = cloud[:, 4:7]
            self._src_nrm_dirty = True

    def setSourceNormals(self, normals):
        self.src_normals = normals
        self._src_nrm_dirty = True

    def setUseSymmetricObjective(self, on):
        """icp.h:380-400: TransformationEstimationSymmetricPointToPlaneLLS instead of PointToPlaneLLS."""
        self.MODE = _lib.SYMMETRIC if on else POINT_TO_PLANE
        self.p.mode = self.MODE

    def getUseSymmetricObjective(self):
        return self.MODE == _lib.SYMMETRIC

    def setEnforceSameDirectionNormals(self, on):
        """icp.h:416-428.  Only stored here (this is usually called before the clouds are set); applied
        whenever the device-side registration object is (re)created."""
        self._enforce = bool(on)

    def _apply_options(self):
        check(self.lib.pclhip_icp_set_enforce_same_direction_normals(
            self.h, 1 if getattr(self, "_enforce", True) else 0), self.ctx.h)

    def getEnforceSameDirectionNormals(self):
        return getattr(self, "_enforce", True)


def estimateRigidTransformation(ctx, mode, src, tgt, src_normals=None, tgt_normals=None,
                                enforce_same_direction_normals=True, weights=None):
    """TransformationEstimation{SVD, PointToPlaneLLS, SymmetricPointToPlaneLLS}::estimateRigidTransformation
    (cloud_src, cloud_tgt) for equally sized clouds (pair i = (src[i], tgt[i])).  Returns (T 4x4, sums)."""
    sp, ss, n, _k1 = _cloud(src)
    tp, ts, nt, _k2 = _cloud(tgt)
    assert n == nt, "Number or points in source differs than target"
    snp, sns = None, 0
    tnp, tns = None, 0
    if src_normals is not None:
        snp, sns, _, _k3 = _cloud(src_normals)
    if tgt_normals is not None:
        tnp, tns, _, _k4 = _cloud(tgt_normals)
    T = np.zeros(16, np.float32)
    sums = np.zeros(_lib.NSUMS, np.float64)
    if weights is not None:  # TransformationEstimationPointToPlaneLLSWeighted::setWeights
        assert int(mode) == POINT_TO_PLANE, "weights belong to the point-to-plane estimator"
        w = np.ascontiguousarray(weights, np.float32)
        assert w.shape == (n,), "Number or weights from the number of correspondences"
        check(ctx.lib.pclhip_estimate_rigid_transformation_weighted(
            ctx.h, sp, ss, tp, ts, tnp, tns, C.c_void_p(w.ctypes.data), n, _fp(T),
            sums.ctypes.data_as(C.POINTER(C.c_double))), ctx.h)
        return T.reshape(4, 4), sums
    check(ctx.lib.pclhip_estimate_rigid_transformation(
        ctx.h, int(mode), sp, ss, snp, sns, tp, ts, tnp, tns, n, 1 if enforce_same_direction_normals else 0,
        _fp(T), sums.ctypes.data_as(C.POINTER(C.c_double))), ctx.h)
    return T.reshape(4, 4), sums


def getPCDHeader(path):
    """PCDReader::readHeader (io/src/pcd_io.cpp:115-392) -> _lib.PcdInfo"""
    info = _lib.PcdInfo()
    check(_lib.load().pclhip_pcd_read_header(os.fsencode(path), C.byref(info)))
    return info


def loadPCDFile(path, with_normals=False, device=None):
    """pcl::io::loadPCDFile into PointXYZ records [n,4] (x,y,z,1) or PointNormal records [n,12]
    (x,y,z,1, nx,ny,nz,0, curvature,0,0,0).  device=None -> numpy array, else a torch tensor on that
    device (the library writes straight into its memory).  Returns (cloud, is_dense)."""
    lib = _lib.load()
    info = getPCDHeader(path)
    n = int(info.points)
    cols = 12 if with_normals else 4
    dense = C.c_int(1)
    cnt = C.c_uint64(0)
    if device is None:
        out = np.zeros((n, cols), np.float32)
        ptr = C.c_void_p(out.ctypes.data)
    else:
        import torch
        out = torch.zeros((n, cols), dtype=torch.float32, device=device)
        ptr = C.c_void_p(out.data_ptr())
    check(lib.pclhip_pcd_read(os.fsencode(path), ptr, cols * 4, 16 if with_normals else 0, n, C.byref(cnt),
                              C.byref(dense)))
    return out, bool(dense.value)


def loadPCDField(path, field, component=0):
    """One component of any field of a PCD file as float32 [n] (packed rgb/rgba: view the result as uint32)."""
    info = getPCDHeader(path)
    out = np.zeros(int(info.points), np.float32)
    cnt = C.c_uint64(0)
    check(_lib.load().pclhip_pcd_read_field(os.fsencode(path), field.encode(), int(component),
                                            C.c_void_p(out.ctypes.data), len(out), C.byref(cnt)))
    return out


def savePCDFile(path, cloud, mode="binary", precision=8, width=None, height=None, viewpoint=None):
    """pcl::io::savePCDFile{ASCII,Binary,BinaryCompressed}; clouds with >= 7 columns (PointNormal layout:
    normals at floats 4..6, curvature at float 8 when present) are written with their normals."""
    data_type = {"ascii": 0, "binary": 1, "binary_compressed": 2}[mode]
    ptr, stride, n, keep = _cloud(cloud)
    ncol = stride // 4
    if width is None and height is None and viewpoint is None:
        check(_lib.load().pclhip_pcd_write(os.fsencode(path), ptr, stride, 16 if ncol >= 7 else 0, n, data_type,
                                           int(precision)))
        return
    width = n if width is None else int(width)
    height = 1 if height is None else int(height)
    assert width * height == n, "width x height must equal the number of points"
    vp = None
    if viewpoint is not None:
        vp = np.ascontiguousarray(viewpoint, np.float32)
        assert vp.shape == (7,)
    check(_lib.load().pclhip_pcd_write_organized(os.fsencode(path), ptr, stride, 16 if ncol >= 7 else 0, width, height,
                                                 _fp(vp) if vp is not None else None, data_type, int(precision)))


class GeneralizedIterativeClosestPoint:
    """pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ> with the Newton solver (registration/include/pcl/
    registration/gicp.h, impl/gicp.hpp:370-477, 768-933).  Covariances are computed by the first align() and cached:
    setInputSource drops the source's, setInputTarget the target's; set{Source,Target}Covariances replace them."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.p = _lib.GicpParams()
        self.lib.pclhip_gicp_params_default(C.byref(self.p))
        self.tree = KdTree(self.ctx)
        self.src_tree = None
        self.h = None
        self.src = None
        self.target = None
        self._target_updated = False
        self._force_no_recompute = False
        self._src_dirty = True
        self._src_cov = None
        self._tgt_cov = None
        self._tgt_cov_dirty = False
        self.result = None
        self.trace = []
        self.ctx._adopt(self)

    def _release(self):
        self._drop()

    def _drop(self):
        if getattr(self, "h", None):
            if self.ctx.h is not None:
                self.lib.pclhip_gicp_destroy(self.h)
            self.h = None
        self._src_dirty = True
        self._tgt_cov_dirty = self._tgt_cov is not None

    def getClassName(self):
        return "GeneralizedIterativeClosestPoint"

    # --- inputs (gicp.h:160-215, registration.h:195-240) ---
    def setInputTarget(self, cloud):
        """GeneralizedIterativeClosestPoint::setInputTarget (gicp.h:174-180): drops the target covariances."""
        self.target = cloud
        self._target_updated = True
        self._tgt_cov = None
        self._drop()

    def setSearchMethodTarget(self, tree, force_no_recompute=False):
        """registration.h:214-221: a new tree counts as an update of the target; with force_no_recompute the caller
        vouches that `tree` already indexes it and it is used as given."""
        self.tree = tree
        self._force_no_recompute = bool(force_no_recompute)
        self._target_updated = self.target is not None
        self._drop()

    def setSearchMethodSource(self, tree, force_no_recompute=False):
        """registration.h:228-240: the source tree only serves the source covariances, which are computed over the
        source cloud itself here (the same k nearest neighbours whichever tree finds them)."""
        self.src_tree = tree

    def setInputSource(self, cloud):
        """GeneralizedIterativeClosestPoint::setInputSource (gicp.h:160-166): drops the source covariances."""
        self.src = cloud
        self._src_cov = None
        self._src_dirty = True

    def setSourceCovariances(self, cov):
        self._src_cov = np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
        self._src_dirty = True

    def setTargetCovariances(self, cov):
        self._tgt_cov = np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
        self._tgt_cov_dirty = True

    def setIndices(self, indices):
        if indices is not None:
            raise NotImplementedError("GeneralizedIterativeClosestPoint: source subsets (setIndices) are not supported")

    def useBFGS(self):
        raise NotImplementedError("GeneralizedIterativeClosestPoint: the BFGS solver is not supported (Newton only)")

    def setCommunicator(self, comm):
        raise NotImplementedError("GeneralizedIterativeClosestPoint: multi-GPU registration is not supported")

    # --- parameters (gicp.h:136-152, 386-431) ---
    def setMaximumIterations(self, n):
        self.p.max_iterations = int(n)

    def setTransformationEpsilon(self, e):
        self.p.transformation_epsilon = float(e)

    def setRotationEpsilon(self, e):
        self.p.rotation_epsilon = float(e)

    def setMaxCorrespondenceDistance(self, d):
        self.p.max_correspondence_distance = float(d)

    def setCorrespondenceRandomness(self, k):
        self.p.k_correspondences = int(k)

    def setMaximumOptimizerIterations(self, n):
        self.p.max_inner_iterations = int(n)

    def setTranslationGradientTolerance(self, t):
        self.p.translation_gradient_tolerance = float(t)

    def setRotationGradientTolerance(self, t):
        self.p.rotation_gradient_tolerance = float(t)

    def getMaximumIterations(self):
        return int(self.p.max_iterations)

    def getTransformationEpsilon(self):
        return float(self.p.transformation_epsilon)

    def getRotationEpsilon(self):
        return float(self.p.rotation_epsilon)

    def getMaxCorrespondenceDistance(self):
        return float(self.p.max_correspondence_distance)

    def getCorrespondenceRandomness(self):
        return int(self.p.k_correspondences)

    def getMaximumOptimizerIterations(self):
        return int(self.p.max_inner_iterations)

    def _ensure(self):
        if self._target_updated and not self._force_no_recompute:
            self.tree.setInputCloud(self.target)
            self._target_updated = False
            self._drop()
        if self.tree.h is None:
            raise ValueError("No input target dataset was given!")
        if self.src is None:
            raise ValueError("No input source dataset was given!")
        if self.h is None:
            h = C.c_void_p()
            check(self.lib.pclhip_gicp_create(self.tree.h, C.byref(h)), self.ctx.h)
            self.h = h
        if self._src_dirty:
            ptr, stride, n, keep = _cloud(self.src)
            check(self.lib.pclhip_gicp_set_source(self.h, ptr, stride, n), self.ctx.h)
            if self._src_cov is not None:
                check(self.lib.pclhip_gicp_set_source_covariances(self.h, C.c_void_p(self._src_cov.ctypes.data),
                                                                  len(self._src_cov)), self.ctx.h)
            self._src_dirty = False
        if self._tgt_cov_dirty:
            check(self.lib.pclhip_gicp_set_target_covariances(self.h, C.c_void_p(self._tgt_cov.ctypes.data),
                                                              len(self._tgt_cov)), self.ctx.h)
            self._tgt_cov_dirty = False

    def align(self, guess=None, trace_capacity=256):
        """Registration::align -> computeTransformation (impl/gicp.hpp:768-930).  Results via getFinalTransformation()
        / hasConverged(); the per-outer-iteration record in self.trace."""
        self._ensure()
        buf = (_lib.GicpTrace * max(1, int(trace_capacity)))()
        check(self.lib.pclhip_gicp_set_trace(self.h, buf, int(trace_capacity)), self.ctx.h)
        r = _lib.GicpResult()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(16)
        try:
            check(self.lib.pclhip_gicp_align(self.h, C.byref(self.p), _fp(g) if g is not None else None, C.byref(r)),
                  self.ctx.h)
        finally:
            self.lib.pclhip_gicp_set_trace(self.h, None, 0)
        self.result = r
        self.trace = [dict(correspondences=int(t.correspondences), inner_iterations=int(t.inner_iterations), f=float(t.f),
                           transformation=np.array(t.transformation, np.float32).reshape(4, 4))
                      for t in buf[:r.trace_count]]

    def getFinalTransformation(self):
        return np.array(self.result.final_transformation, np.float32).reshape(4, 4)

    def getLastIncrementalTransformation(self):
        return np.array(self.result.last_transformation, np.float32).reshape(4, 4)

    def hasConverged(self):
        return bool(self.result.converged)

    @property
    def nr_iterations_(self):
        return int(self.result.nr_iterations)

    def getFitnessScore(self, max_range=float(np.finfo(np.float64).max)):
        """Registration::getFitnessScore (impl/registration.hpp:132-168) with the final transformation."""
        self._ensure()
        T = np.ascontiguousarray(self.getFinalTransformation(), np.float32).reshape(16)
        score = C.c_double(0.0)
        nr = C.c_uint64(0)
        check(self.lib.pclhip_gicp_fitness_score(self.h, _fp(T), C.c_double(max_range), C.byref(score), C.byref(nr)),
              self.ctx.h)
        return float(score.value)

    def evaluate(self, x):
        """OptimizationFunctorWithIndices::dfddf (impl/gicp.hpp:612-750) on the pairs of the last outer iteration:
        (f, g[6], H[6x6])."""
        xv = np.ascontiguousarray(x, np.float64).reshape(6)
        f = C.c_double(0.0)
        g = np.zeros(6, np.float64)
        H = np.zeros(36, np.float64)
        dp = C.POINTER(C.c_double)
        check(self.lib.pclhip_gicp_evaluate(self.h, xv.ctypes.data_as(dp), C.byref(f), g.ctypes.data_as(dp),
                                            H.ctypes.data_as(dp)), self.ctx.h)
        return float(f.value), g, H.reshape(6, 6)

    def mahalanobis(self):
        """mahalanobis_: one 3x3 per source point (NaN for non-finite points)."""
        n = _cloud(self.src)[2]
        out = np.zeros((n, 9), np.float64)
        check(self.lib.pclhip_gicp_mahalanobis(self.h, C.c_void_p(out.ctypes.data)), self.ctx.h)
        return out.reshape(n, 3, 3)

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass


class NormalDistributionsTransform:
    """pcl::NormalDistributionsTransform<PointXYZ, PointXYZ> (registration/include/pcl/registration/ndt.h, impl/ndt.hpp)
    with the RADIUS neighbourhood.  The voxel Gaussians of the target (VoxelGridCovariance) are built by the first call
    that needs them and cached until the target, the resolution or min_points_per_voxel changes."""

    RADIUS, DIRECT27, DIRECT26, DIRECT7, DIRECT1 = (_lib.NDT_RADIUS, _lib.NDT_DIRECT27, _lib.NDT_DIRECT26, _lib.NDT_DIRECT7,
                                                    _lib.NDT_DIRECT1)

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.p = _lib.NdtParams()
        self.lib.pclhip_ndt_params_default(C.byref(self.p))
        self.h = None
        self.src = None
        self.target = None
        self._tgt_dirty = True
        self._src_dirty = True
        self.result = None
        self.trace = []
        self.ctx._adopt(self)

    def _release(self):
        self._drop()

    def _drop(self):
        if getattr(self, "h", None):
            if self.ctx.h is not None:
                self.lib.pclhip_ndt_destroy(self.h)
            self.h = None
        self._tgt_dirty = self._src_dirty = True

    def getClassName(self):
        return "NormalDistributionsTransform"

    # --- inputs (ndt.h:121-141, registration.h:195-240) ---
    def setInputTarget(self, cloud):
        """ndt.h:121-127: a new target rebuilds the voxel grid."""
        self.target = cloud
        self._tgt_dirty = True

    def setInputSource(self, cloud):
        self.src = cloud
        self._src_dirty = True

    def setSearchMethodTarget(self, tree, force_no_recompute=False):
        """Accepted: NormalDistributionsTransform searches its voxel grid, not the target's tree."""

    def setSearchMethodSource(self, tree, force_no_recompute=False):
        """Accepted: see setSearchMethodTarget."""

    def setNumberOfThreads(self, n):
        """Accepted, no effect (impl/ndt.hpp:49-66: the OpenMP thread count of the derivative loop)."""

    def setIndices(self, indices):
        if indices is not None:
            raise NotImplementedError("NormalDistributionsTransform: source subsets (setIndices) are not supported")

    def setCommunicator(self, comm):
        raise NotImplementedError("NormalDistributionsTransform: multi-GPU registration is not supported")

    # --- parameters (ndt.h:130-260) ---
    def setResolution(self, r):
        """ndt.h:133-141: a new resolution rebuilds the voxel grid (on the next call that needs it)."""
        self.p.resolution = float(r)

    def getResolution(self):
        return float(self.p.resolution)

    def setStepSize(self, s):
        self.p.step_size = float(s)

    def getStepSize(self):
        return float(self.p.step_size)

    def setOutlierRatio(self, r):
        self.p.outlier_ratio = float(r)

    def getOutlierRatio(self):
        return float(self.p.outlier_ratio)

    def setMinPointPerVoxel(self, n):
        self.p.min_points_per_voxel = int(n)

    def setMaximumIterations(self, n):
        self.p.max_iterations = int(n)

    def getMaximumIterations(self):
        return int(self.p.max_iterations)

    def setTransformationEpsilon(self, e):
        self.p.transformation_epsilon = float(e)

    def getTransformationEpsilon(self):
        return float(self.p.transformation_epsilon)

    def setTransformationRotationEpsilon(self, e):
        self.p.transformation_rotation_epsilon = float(e)

    def setNeighborhoodSearchMethod(self, method):
        """ndt.h:243-254.  Only NeighborSearchMethod::RADIUS (the reference's default) is built."""
        if int(method) != _lib.NDT_RADIUS:
            raise NotImplementedError("NormalDistributionsTransform: the DIRECT27 / DIRECT26 / DIRECT7 / DIRECT1 "
                                      "neighbourhoods are not supported (RADIUS only)")
        self.p.neighborhood_search_method = int(method)

    def _ensure(self):
        if self.target is None:
            raise ValueError("No input target dataset was given!")
        if self.src is None:
            raise ValueError("No input source dataset was given!")
        if self.h is None:
            h = C.c_void_p()
            check(self.lib.pclhip_ndt_create(self.ctx.h, C.byref(h)), self.ctx.h)
            self.h = h
        if self._tgt_dirty:
            ptr, stride, n, keep = _cloud(self.target)
            check(self.lib.pclhip_ndt_set_target(self.h, ptr, stride, n), self.ctx.h)
            self._tgt_dirty = False
        if self._src_dirty:
            ptr, stride, n, keep = _cloud(self.src)
            check(self.lib.pclhip_ndt_set_source(self.h, ptr, stride, n), self.ctx.h)
            self._src_dirty = False

    def align(self, guess=None, trace_capacity=256, want_output=False):
        """Registration::align -> computeTransformation (impl/ndt.hpp:79-207).  Returns the registered source (the input
        moved by the final transformation, transformPointCloud's order) when want_output, else None; results via
        getFinalTransformation() / hasConverged(); per outer iteration the step length, the line search's trials, the
        score and the transformation in self.trace."""
        self._ensure()
        buf = (_lib.NdtTrace * max(1, int(trace_capacity)))()
        check(self.lib.pclhip_ndt_set_trace(self.h, buf, int(trace_capacity)), self.ctx.h)
        r = _lib.NdtResult()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(16)
        try:
            check(self.lib.pclhip_ndt_align(self.h, C.byref(self.p), _fp(g) if g is not None else None, C.byref(r)),
                  self.ctx.h)
        finally:
            self.lib.pclhip_ndt_set_trace(self.h, None, 0)
        self.result = r
        self.trace = [dict(step_length=float(t.step_length), line_search_trials=int(t.line_search_trials),
                           score=float(t.score), transformation=np.array(t.transformation, np.float32).reshape(4, 4))
                      for t in buf[:r.trace_count]]
        if not want_output:
            return None
        ptr, stride, n, keep = _cloud(self.src)
        out = keep.clone() if _is_torch(self.src) else keep.copy()
        optr = C.c_void_p(out.data_ptr() if _is_torch(self.src) else out.ctypes.data)
        check(self.lib.pclhip_transform_cloud(self.ctx.h, _fp(np.ascontiguousarray(self.getFinalTransformation()).reshape(16)),
                                              1, ptr, optr, stride, n, 0), self.ctx.h)
        return out

    def getFinalTransformation(self):
        return np.array(self.result.final_transformation, np.float32).reshape(4, 4)

    def getLastIncrementalTransformation(self):
        return np.array(self.result.last_transformation, np.float32).reshape(4, 4)

    def hasConverged(self):
        return bool(self.result.converged)

    def getFinalNumIteration(self):
        return int(self.result.nr_iterations)

    @property
    def nr_iterations_(self):
        return int(self.result.nr_iterations)

    def getTransformationLikelihood(self):
        return float(self.result.transformation_likelihood)

    def getTransformationProbability(self):
        return self.getTransformationLikelihood()

    def getFitnessScore(self, max_range=float(np.finfo(np.float64).max)):
        """Registration::getFitnessScore (impl/registration.hpp:132-168) with the final transformation."""
        self._ensure()
        T = np.ascontiguousarray(self.getFinalTransformation(), np.float32).reshape(16)
        score = C.c_double(0.0)
        nr = C.c_uint64(0)
        check(self.lib.pclhip_ndt_fitness_score(self.h, _fp(T), C.c_double(max_range), C.byref(score), C.byref(nr)),
              self.ctx.h)
        return float(score.value)

    def evaluate(self, x, variant=0):
        """One derivative pass at x = (tx ty tz roll pitch yaw): (score, g[6], H[6x6], pairs).  variant 0: all three
        (computeDerivatives), 1: score and gradient (the line search's trials), 2: Hessian only (computeHessian)."""
        self._ensure()
        xv = np.ascontiguousarray(x, np.float64).reshape(6)
        f = C.c_double(0.0)
        pairs = C.c_uint64(0)
        g = np.zeros(6, np.float64)
        H = np.zeros(36, np.float64)
        dp = C.POINTER(C.c_double)
        check(self.lib.pclhip_ndt_evaluate(self.h, C.byref(self.p), xv.ctypes.data_as(dp), int(variant), C.byref(f),
                                           g.ctypes.data_as(dp), H.ctypes.data_as(dp), C.byref(pairs)), self.ctx.h)
        return float(f.value), g, H.reshape(6, 6), int(pairs.value)

    def cells(self):
        """The voxel Gaussians of the target in ascending voxel id: dict(centroids (n, 3) float32, means (n, 3), cov and
        icov (n, 3, 3) float64, npoints, voxel_ids (n,) int32, valid (n,) bool)."""
        self._ensure()
        count = C.c_uint64(0)
        none = C.c_void_p(None)
        check(self.lib.pclhip_ndt_cells(self.h, C.byref(self.p), C.byref(count), none, none, none, none, none, none, none, 0),
              self.ctx.h)
        n = int(count.value)
        out = dict(centroids=np.zeros((n, 3), np.float32), means=np.zeros((n, 3), np.float64), cov=np.zeros((n, 3, 3), np.float64),
                   icov=np.zeros((n, 3, 3), np.float64), npoints=np.zeros(n, np.int32), voxel_ids=np.zeros(n, np.int32),
                   valid=np.zeros(n, np.uint8))
        if n:
            ptr = [C.c_void_p(out[k].ctypes.data) for k in ("centroids", "means", "cov", "icov", "npoints", "voxel_ids", "valid")]
            check(self.lib.pclhip_ndt_cells(self.h, C.byref(self.p), C.byref(count), *ptr, n), self.ctx.h)
        out["valid"] = out["valid"].astype(bool)
        return out

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass


class VoxelGrid:
    """pcl::VoxelGrid<PointT> for pcl::PointXYZ ((n, 4) clouds) and pcl::PointNormal ((n, 12) clouds): leaf size,
    minimum points per voxel, downsample_all_data, the pass-through filter on one field, the leaf layout."""

    _FLT_MAX = float(np.finfo(np.float32).max)
    # position of a field inside the record, in floats (point_types.hpp:315-321, 843-853)
    _FIELDS = {"x": 0, "y": 1, "z": 2, "normal_x": 4, "normal_y": 5, "normal_z": 6, "curvature": 8}

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.leaf = np.zeros(3, np.float32)
        self.min_pts = 0
        self.field = ""                                  # voxel_grid.h:503-512: no filter until a field is named
        self.limits = (-self._FLT_MAX, self._FLT_MAX)
        self.negative = False
        self.cloud = None

    def setInputCloud(self, cloud):
        self.cloud = cloud

    def setLeafSize(self, lx, ly=None, lz=None):
        self.leaf = np.asarray([lx, lx if ly is None else ly, lx if lz is None else lz], np.float32)

    def setMinimumPointsNumberPerVoxel(self, n):
        self.min_pts = int(n)

    def getLeafSize(self):
        return tuple(float(v) for v in self.leaf)

    def getMinimumPointsNumberPerVoxel(self):
        return self.min_pts

    def setFilterFieldName(self, name):
        """voxel_grid.h:440-444: points are filtered on this field before the grid is laid out ("" = no filter)"""
        self.field = str(name)

    def getFilterFieldName(self):
        return self.field

    def setFilterLimits(self, lo, hi):
        self.limits = (float(lo), float(hi))

    def getFilterLimits(self):
        return self.limits

    def setFilterLimitsNegative(self, negative):
        """voxel_grid.h:468-476: True keeps the points OUTSIDE (limit_min, limit_max) instead of those inside"""
        self.negative = bool(negative)

    def getFilterLimitsNegative(self):
        return self.negative

    def _limit_flags(self, stride):
        if not self.field:
            return 0
        idx = self._FIELDS.get(self.field)
        if idx is None or (idx + 1) * 4 > stride or (idx > 2 and stride < 48):
            raise ValueError("[pcl::VoxelGrid] could not find field '%s' in this point type" % self.field)
        return 1 | (2 if self.negative else 0) | ((idx + 1) << 8)

    def setDownsampleAllData(self, downsample):
        """voxel_grid.h:293-302: False averages only x, y, z and leaves the other fields of the output at 0"""
        self.all_data = bool(downsample)

    def getDownsampleAllData(self):
        return getattr(self, "all_data", True)

    def filter(self):
        """-> [m, 4] (x, y, z, 1) for PointXYZ clouds; clouds with >= 12 columns are pcl::PointNormal records
        (x y z 1 | nx ny nz 0 | curvature 0 0 0) and come back in the same layout."""
        ptr, stride, n, keep = _cloud(self.cloud)
        cnt = C.c_uint64(0)
        has = self._limit_flags(stride)
        lo, hi = self.limits
        with_normals = stride >= 48
        cols = 12 if with_normals else 4
        if _is_torch(self.cloud):
            import torch
            out = torch.empty((max(n, 1), cols), dtype=torch.float32, device=self.cloud.device)
            optr = C.c_void_p(out.data_ptr())
        else:
            out = np.empty((max(n, 1), cols), np.float32)
            optr = C.c_void_p(out.ctypes.data)
        from ._lib import VoxelGridDims
        dims = VoxelGridDims()
        layout = None
        if getattr(self, "save_leaf_layout", False) and n > 0:
            # the layout has one int per cell of the grid: ask for the grid first (a bounding-box pass)
            check(self.lib.pclhip_voxelgrid_grid(self.ctx.h, ptr, stride, n, _fp(self.leaf), int(has), lo, hi,
                                                 C.byref(dims)), self.ctx.h)
            layout = np.empty(int(dims.div_b[0]) * int(dims.div_b[1]) * int(dims.div_b[2]), np.int32)
        check(self.lib.pclhip_voxelgrid_ex2(self.ctx.h, ptr, stride, n, _fp(self.leaf), self.min_pts, int(has), lo, hi,
                                            int(self.getDownsampleAllData()), 16 if with_normals else 0, optr, cols * 4,
                                            C.byref(cnt), None if layout is None else C.c_void_p(layout.ctypes.data),
                                            0 if layout is None else len(layout), C.byref(dims)), self.ctx.h)
        self._dims = dims
        self._layout = layout
        return out[:int(cnt.value)]

    # ---- the grid of the last filter() call and the leaf layout (voxel_grid.h:316-420) ----
    def setSaveLeafLayout(self, save):
        self.save_leaf_layout = bool(save)

    def getSaveLeafLayout(self):
        return getattr(self, "save_leaf_layout", False)

    def getMinBoxCoordinates(self):
        return np.asarray(self._dims.min_b, np.int32)

    def getMaxBoxCoordinates(self):
        return np.asarray(self._dims.max_b, np.int32)

    def getNrDivisions(self):
        return np.asarray(self._dims.div_b, np.int32)

    def getDivisionMultiplier(self):
        return np.asarray(self._dims.divb_mul, np.int32)

    def getLeafLayout(self):
        """position (i-min_x) + (j-min_y)*div_x + (k-min_z)*div_x*div_y -> index of that voxel's centroid, -1 if empty"""
        return np.empty(0, np.int32) if self._layout is None else self._layout

    def getGridCoordinates(self, x, y, z):
        inv = np.float32(1.0) / self.leaf
        return np.floor(np.asarray([x, y, z], np.float32) * inv).astype(np.int32)      # voxel_grid.h:402-407

    def getCentroidIndexAt(self, ijk):
        idx = int(np.dot(np.asarray(ijk, np.int64) - self.getMinBoxCoordinates(), self.getDivisionMultiplier()))
        if self._layout is None or idx < 0 or idx >= len(self._layout):
            return -1                                                                   # voxel_grid.h:412-421
        return int(self._layout[idx])

    def getCentroidIndex(self, p):
        return self.getCentroidIndexAt(self.getGridCoordinates(p[0], p[1], p[2]))


class _OutlierRemoval:
    """FilterIndices<PointT> surface shared by StatisticalOutlierRemoval and RadiusOutlierRemoval
    (filters/include/pcl/filters/filter_indices.h, impl/filter_indices.hpp:77-107).  The input is an (n, c >= 3) float32
    cloud, numpy or a torch CUDA tensor; results come back in the same kind of array."""

    def __init__(self, ctx=None, extract_removed_indices=False):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.extract_removed_indices = bool(extract_removed_indices)
        self._cloud = None
        self._is_dense = None
        self._indices = None
        self._negative = False
        self._keep_organized = False
        self._user_value = float("nan")
        self._tree = None      # setSearchMethod
        self._own = None       # the index this filter built, cached for the same cloud object
        self._own_key = None
        self._removed = np.empty(0, np.int32)
        self._ms = 0.0
        self._threads = 0

    def getClassName(self):
        return type(self).__name__

    def setInputCloud(self, cloud, is_dense=None):
        """is_dense: the PointCloud's flag; None = every point is finite (computed)."""
        self._cloud = cloud
        self._is_dense = None if is_dense is None else bool(is_dense)

    def getInputCloud(self):
        return self._cloud

    def setIndices(self, indices):
        self._indices = indices

    def getIndices(self):
        return self._indices

    def setNegative(self, negative):
        self._negative = bool(negative)

    def getNegative(self):
        return self._negative

    def setKeepOrganized(self, keep):
        self._keep_organized = bool(keep)

    def getKeepOrganized(self):
        return self._keep_organized

    def setUserFilterValue(self, value):
        self._user_value = float(value)

    def setNumberOfThreads(self, n):
        """Accepted for PCL compatibility; the GPU decides its own parallelism."""
        self._threads = int(n)

    def setSearchMethod(self, tree):
        """A KdTree already built over this filter's (unscaled, whole) input cloud is reused; any other tree is ignored and
        the filter builds its own index."""
        self._tree = tree

    def getSearchMethod(self):
        return self._tree

    def getRemovedIndices(self):
        return self._removed

    def lastKernelMs(self):
        """GPU time of the last filter call (all of its kernels)."""
        return self._ms

    def _dense(self):
        if self._is_dense is not None:
            return self._is_dense
        c = self._cloud
        if _is_torch(c):
            import torch
            return bool(torch.isfinite(c[:, :3]).all().item())
        return bool(np.isfinite(np.asarray(c, np.float32)[:, :3]).all())

    def _index(self):
        t = self._tree
        if (t is not None and getattr(t, "h", None) and t.getInputCloud() is self._cloud and t.getIndices() is None
                and getattr(t, "_scale", None) is None):
            return t.h
        key = id(self._cloud)
        if self._own is None or self._own_key != key or self._own._cloud is not self._cloud:
            self._own = KdTree(self.ctx)
            self._own.setInputCloud(self._cloud)
            self._own_key = key
        return self._own.h

    def _run(self, call):
        """call(index, idx_ptr, n_idx, kept_ptr, n_kept, removed_ptr, n_removed) -> (kept, removed) as arrays."""
        assert self._cloud is not None, "setInputCloud first"
        ptr, stride, n, keep = _cloud(self._cloud)
        dev = _is_torch(self._cloud)
        ind = self._indices
        if ind is None:
            m = n
            iptr = None
        elif _is_torch(ind):
            ind = ind.to(dtype=__import__("torch").int32).contiguous()
            m = int(ind.numel())
            iptr = C.c_void_p(ind.data_ptr())
        else:
            ind = np.ascontiguousarray(ind, np.int32)
            m = len(ind)
            iptr = C.c_void_p(ind.ctypes.data)
        want_removed = self.extract_removed_indices or self._keep_organized
        if dev:
            import torch
            kept = torch.empty(max(m, 1), dtype=torch.int32, device=self._cloud.device)
            rem = torch.empty(max(m, 1), dtype=torch.int32, device=self._cloud.device) if want_removed else None
            kp, rp = C.c_void_p(kept.data_ptr()), (C.c_void_p(rem.data_ptr()) if rem is not None else None)
        else:
            kept = np.empty(max(m, 1), np.int32)
            rem = np.empty(max(m, 1), np.int32) if want_removed else None
            kp, rp = C.c_void_p(kept.ctypes.data), (C.c_void_p(rem.ctypes.data) if rem is not None else None)
        nk, nr = C.c_uint64(0), C.c_uint64(0)
        h = self._index()
        check(call(h, iptr, m, kp, C.byref(nk), rp, C.byref(nr)), self.ctx.h)
        self._ms = float(self.lib.pclhip_index_last_kernel_ms(h))
        kept = kept[:nk.value]
        if rem is not None:
            rem = rem[:nr.value]
        else:
            rem = kept[:0]
        self._removed = rem if self.extract_removed_indices or self._keep_organized else kept[:0]
        return kept, rem

    def filterIndices(self):
        """filter(Indices&): the ids of the kept points, in input (or setIndices) order."""
        kept, _ = self._run(self._call)
        return kept

    def filter(self):
        """filter(PointCloud&): the kept records in the input's layout; with setKeepOrganized the whole input with the xyz of
        removed records set to the user filter value."""
        if self._keep_organized:
            self.extract_removed_indices = True  # filter_indices.hpp:82-86
        kept, rem = self._run(self._call)
        c = self._cloud
        if self._keep_organized:
            if _is_torch(c):
                out = c.clone()
                out[rem.long(), :3] = self._user_value
            else:
                out = np.array(c, np.float32, copy=True)
                out[rem, :3] = np.float32(self._user_value)
            return out
        if _is_torch(c):
            return c.index_select(0, kept.long())
        return np.asarray(c, np.float32)[kept]


class StatisticalOutlierRemoval(_OutlierRemoval):
    """pcl::StatisticalOutlierRemoval<PointT> (filters/include/pcl/filters/statistical_outlier_removal.h,
    impl/statistical_outlier_removal.hpp:47-132) over pclhip_statistical_outlier_removal."""

    def __init__(self, ctx=None, extract_removed_indices=False):
        super().__init__(ctx, extract_removed_indices)
        self._mean_k = 1
        self._std_mul = 0.0
        self._dist = None
        self._stats = None

    def setMeanK(self, k):
        self._mean_k = int(k)

    def getMeanK(self):
        return self._mean_k

    def setStddevMulThresh(self, m):
        self._std_mul = float(m)

    def getStddevMulThresh(self):
        return self._std_mul

    def lastMeanDistances(self):
        """Per query (input or setIndices order) the mean distance to its mean_k neighbours (0 for non-finite points)."""
        return self._dist

    def lastStatistics(self):
        """dict(mean, stddev, threshold, sum, sq_sum, valid) of the last call."""
        return self._stats

    def _call(self, h, iptr, m, kp, nk, rp, nr):
        if _is_torch(self._cloud):
            import torch
            self._dist = torch.empty(max(m, 1), dtype=torch.float32, device=self._cloud.device)
            dptr = C.c_void_p(self._dist.data_ptr())
        else:
            self._dist = np.empty(max(m, 1), np.float32)
            dptr = C.c_void_p(self._dist.ctypes.data)
        st = _lib.SorStats()
        r = self.lib.pclhip_statistical_outlier_removal(h, iptr, m, self._mean_k, self._std_mul, int(self._negative), kp, nk,
                                                        rp, nr, dptr, C.byref(st))
        self._dist = self._dist[:m]
        self._stats = dict(mean=st.mean, stddev=st.stddev, threshold=st.threshold, sum=st.sum, sq_sum=st.sq_sum,
                           valid=int(st.valid))
        return r


class RadiusOutlierRemoval(_OutlierRemoval):
    """pcl::RadiusOutlierRemoval<PointT> (filters/include/pcl/filters/radius_outlier_removal.h,
    impl/radius_outlier_removal.hpp:48-172) over pclhip_radius_outlier_removal.  Which "within" boundary applies follows
    the cloud's is_dense flag (setInputCloud)."""

    def __init__(self, ctx=None, extract_removed_indices=False):
        super().__init__(ctx, extract_removed_indices)
        self._radius = 0.0
        self._min_pts = 1

    def setRadiusSearch(self, r):
        self._radius = float(r)

    def getRadiusSearch(self):
        return self._radius

    def setMinNeighborsInRadius(self, n):
        self._min_pts = int(n)

    def getMinNeighborsInRadius(self):
        return self._min_pts

    def _call(self, h, iptr, m, kp, nk, rp, nr):
        return self.lib.pclhip_radius_outlier_removal(h, iptr, m, self._radius, self._min_pts, int(self._dense()),
                                                      int(self._negative), kp, nk, rp, nr)


class FPFHEstimation:
    """pcl::FPFHEstimation<PointInT, PointNT, pcl::FPFHSignature33> with setRadiusSearch (features/include/pcl/features/
    fpfh.h, impl/fpfh.hpp:51-303) over pclhip_fpfh: search surface == input, 11 / 11 / 11 bins.  The normals are the ones
    given with setInputNormals, or the ones the tree already holds (a NormalEstimation that ran on the same tree)."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.tree = None
        self.radius = 0.0
        self.cloud = None
        self.normals = None
        self.indices = None
        self.nan_count = 0

    def setInputCloud(self, cloud):
        self.cloud = cloud

    def setInputNormals(self, normals):
        """FeatureFromNormals::setInputNormals (feature.h:339-349): one normal per record of the input cloud, (n, c >= 3)."""
        self.normals = normals

    def getInputNormals(self):
        return self.normals

    def setSearchMethod(self, tree):
        self.tree = tree

    def getSearchMethod(self):
        return self.tree

    def setIndices(self, indices):
        """PCLBase::setIndices: one descriptor per input[indices[j]], in that order (None: every record)."""
        self.indices = None if indices is None else np.ascontiguousarray(indices, np.int32)

    def setRadiusSearch(self, radius):
        self.radius = float(radius)

    def getRadiusSearch(self):
        return self.radius

    def setKSearch(self, k):
        if int(k) != 0:
            raise NotImplementedError("FPFHEstimation searches by radius only (setRadiusSearch)")

    def getKSearch(self):
        return 0

    def lastPassMs(self):
        """GPU time (ms) of the SPFH kernel and of the weighting kernel of the last compute()."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self.lib.pclhip_index_last_fpfh_ms(self.tree.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def _run(self, want_fpfh, want_spfh):
        if self.radius == 0.0:  # Feature::initCompute (impl/feature.hpp:131-155)
            raise ValueError("Neither radius nor K defined! Set one of them to a positive number first")
        if self.tree is None:
            self.tree = KdTree(self.ctx)
        if self.tree.h is None or self.tree._cloud_id != (id(self.cloud), None):
            self.tree.setInputCloud(self.cloud)
        if self.normals is not None:
            self.tree.setNormals(self.normals)
        n = self.tree.n_cloud
        m = n if self.indices is None else len(self.indices)
        torch_out = _is_torch(self.cloud)
        if torch_out:
            import torch

            def make(rows):
                t = torch.empty((rows, 33), dtype=torch.float32, device=self.cloud.device)
                return t, C.c_void_p(t.data_ptr())
        else:
            def make(rows):
                a = np.empty((rows, 33), np.float32)
                return a, C.c_void_p(a.ctypes.data)
        out, optr = make(m if want_fpfh else 0)
        spfh, sptr = make(n) if want_spfh else (None, None)
        nan = C.c_uint64(0)
        none = np.zeros(1, np.int32)
        if want_fpfh:
            ind = None if self.indices is None else C.c_void_p(self.indices.ctypes.data)
            ni = 0 if self.indices is None else m
        else:  # an empty index list: no query, the SPFH pass alone
            ind, ni = C.c_void_p(none.ctypes.data), 0
        check(self.lib.pclhip_fpfh(self.tree.h, ind, ni, self.radius, optr, 132, C.cast(sptr, C.POINTER(C.c_float)),
                                   C.byref(nan)), self.ctx.h)
        self.nan_count = int(nan.value)
        return out, spfh

    def compute(self):
        """-> (m, 33) float32: the f1, f2 and f3 histograms of every query (NaN rows are counted in nan_count)."""
        return self._run(True, False)[0]

    def computeSPFH(self):
        """-> (n, 33) float32: the SPFH signature of every record of the input cloud (computePointSPFHSignature)."""
        return self._run(False, True)[1]

    def computeBoth(self):
        """-> ((m, 33) FPFH, (n, 33) SPFH) of one call."""
        return self._run(True, True)


class ISSKeypoint3D:
    """pcl::ISSKeypoint3D<PointInT, PointOutT> without boundary estimation (keypoints/include/pcl/keypoints/iss_3d.h,
    impl/iss_3d.hpp:164-208, 302-473) over pclhip_iss_keypoints.  The input is an (n, c >= 3) float32 cloud, numpy or a
    torch CUDA tensor; the keypoint indices come back ascending, in the same kind of array."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.tree = None
        self.cloud = None
        self.salient_radius = 0.0      # iss_3d.h:117-131: the reference's defaults
        self.non_max_radius = 0.0
        self.gamma_21 = 0.975
        self.gamma_32 = 0.975
        self.min_neighbors = 5
        self._indices = None
        self._saliency = None
        self._eigenvalues = None

    def getClassName(self):
        return "ISSKeypoint3D"

    def setInputCloud(self, cloud):
        self.cloud = cloud

    def getInputCloud(self):
        return self.cloud

    def setSearchMethod(self, tree):
        """An index over the same whole, unscaled cloud (a KdTree another stage built) is reused as it is."""
        self.tree = tree

    def getSearchMethod(self):
        return self.tree

    def setSalientRadius(self, r):
        self.salient_radius = float(r)

    def setNonMaxRadius(self, r):
        self.non_max_radius = float(r)

    def setThreshold21(self, gamma_21):
        self.gamma_21 = float(gamma_21)

    def setThreshold32(self, gamma_32):
        self.gamma_32 = float(gamma_32)

    def setMinNeighbors(self, n):
        self.min_neighbors = int(n)

    def setBorderRadius(self, r):
        if float(r) > 0.0:
            raise NotImplementedError("ISSKeypoint3D: boundary estimation (border_radius > 0) is not built")

    def setNormalRadius(self, r):
        if float(r) > 0.0:
            raise NotImplementedError("ISSKeypoint3D: boundary estimation (normal_radius > 0) is not built")

    def setNumberOfThreads(self, n=0):
        pass

    def lastPassMs(self):
        """GPU time (ms) of the scatter kernel and of the non-maximum kernel of the last compute()."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self.lib.pclhip_index_last_iss_ms(self.tree.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def lastKernelMs(self):
        return float(self.lib.pclhip_index_last_kernel_ms(self.tree.h))

    def _run(self, want_saliency, want_eigenvalues):
        assert self.cloud is not None, "setInputCloud first"
        if self.tree is None:
            self.tree = KdTree(self.ctx)
        if self.tree.h is None or self.tree._cloud_id != (id(self.cloud), None):
            self.tree.setInputCloud(self.cloud)
        n = self.tree.n_cloud
        if _is_torch(self.cloud):
            import torch

            def make(shape, dtype):
                t = torch.empty(shape, dtype={np.int32: torch.int32, np.float64: torch.float64}[dtype],
                                device=self.cloud.device)
                return t, C.c_void_p(t.data_ptr())
        else:
            def make(shape, dtype):
                a = np.empty(shape, dtype)
                return a, C.c_void_p(a.ctypes.data)
        idx, ip = make(max(n, 1), np.int32)
        sal, sp = make(n, np.float64) if want_saliency else (None, None)
        eig, ep = make((n, 3), np.float64) if want_eigenvalues else (None, None)
        k = C.c_uint64(0)
        check(self.lib.pclhip_iss_keypoints(self.tree.h, self.salient_radius, self.non_max_radius, self.gamma_21,
                                            self.gamma_32, self.min_neighbors, ip, n, C.byref(k), sp, ep), self.ctx.h)
        self._indices = idx[:k.value]
        self._saliency, self._eigenvalues = sal, eig
        return self._indices

    def compute(self):
        """-> int32 [k]: the keypoints' indices into the input cloud, ascending."""
        return self._run(False, False)

    def computeAll(self):
        """-> (indices int32 [k], saliency float64 [n], eigenvalues float64 [n, 3] descending) of one call."""
        idx = self._run(True, True)
        return idx, self._saliency, self._eigenvalues

    def getKeypointsIndices(self):
        return self._indices

    def getKeypoints(self):
        """The records of the input cloud at the keypoints of the last compute()."""
        if _is_torch(self.cloud):
            return self.cloud[self._indices.long()]
        return np.asarray(self.cloud)[self._indices]


class BoundaryEstimation:
    """pcl::BoundaryEstimation<PointInT, PointNT, pcl::Boundary> (features/include/pcl/features/boundary.h, impl/
    boundary.hpp:87-209) over pclhip_boundary: search surface == input, by radius or by k.  The normals are the ones given
    with setInputNormals, or the ones the tree already holds.  The input is an (n, c >= 3) float32 cloud, numpy or a torch
    CUDA tensor; the flags come back as uint8 in the same kind of array, one per query."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.tree = None
        self.radius = 0.0
        self.k = 0
        self.angle_threshold = math.pi / 2.0   # boundary.h:91: the reference's default
        self.min_neighbors = 3
        self.cloud = None
        self.normals = None
        self.indices = None
        self.invalid_count = 0

    def getClassName(self):
        return "BoundaryEstimation"

    def setInputCloud(self, cloud):
        self.cloud = cloud

    def getInputCloud(self):
        return self.cloud

    def setInputNormals(self, normals):
        """FeatureFromNormals::setInputNormals: one normal per record of the input cloud, (n, c >= 3)."""
        self.normals = normals

    def getInputNormals(self):
        return self.normals

    def setSearchMethod(self, tree):
        self.tree = tree

    def getSearchMethod(self):
        return self.tree

    def setIndices(self, indices):
        """PCLBase::setIndices: one flag per input[indices[j]], in that order (None: every record)."""
        self.indices = None if indices is None else np.ascontiguousarray(indices, np.int32)

    def setRadiusSearch(self, radius):
        self.radius = float(radius)

    def getRadiusSearch(self):
        return self.radius

    def setKSearch(self, k):
        self.k = int(k)

    def getKSearch(self):
        return self.k

    def setAngleThreshold(self, angle):
        self.angle_threshold = float(angle)

    def getAngleThreshold(self):
        return self.angle_threshold

    def setNumberOfThreads(self, n=0):
        pass

    def lastPassMs(self):
        """GPU time (ms) of the mask pass and of the resolve passes of the last compute()."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self.lib.pclhip_index_last_boundary_ms(self.tree.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def lastResolved(self):
        """How many queries of the last compute() the mask pass left to the resolve pass."""
        return int(self.lib.pclhip_index_last_boundary_resolved(self.tree.h))

    def lastKernelMs(self):
        return float(self.lib.pclhip_index_last_kernel_ms(self.tree.h))

    def compute(self):
        """-> uint8 [m]: 1 for a boundary point; the queries without a defined feature are counted in invalid_count."""
        assert self.cloud is not None, "setInputCloud first"
        if self.tree is None:
            self.tree = KdTree(self.ctx)
        if self.tree.h is None or self.tree._cloud_id != (id(self.cloud), None):
            self.tree.setInputCloud(self.cloud)
        if self.normals is not None:
            self.tree.setNormals(self.normals)
        n = self.tree.n_cloud
        m = n if self.indices is None else len(self.indices)
        if _is_torch(self.cloud):
            import torch
            out = torch.empty(m, dtype=torch.uint8, device=self.cloud.device)
            optr = C.c_void_p(out.data_ptr())
        else:
            out = np.empty(m, np.uint8)
            optr = C.c_void_p(out.ctypes.data)
        bad = C.c_uint64(0)
        none = np.zeros(1, np.int32)
        if self.indices is None:
            ind, ni = None, 0
        else:  # (an empty list is a list: no query)
            ind, ni = C.c_void_p((self.indices if m > 0 else none).ctypes.data), m
        self.invalid_count = 0
        check(self.lib.pclhip_boundary(self.tree.h, ind, ni, self.radius, self.k, self.angle_threshold, self.min_neighbors,
                                       optr, C.byref(bad)), self.ctx.h)
        self.invalid_count = int(bad.value)
        return out


class MovingLeastSquares:
    """pcl::MovingLeastSquares<PointInT, PointOutT> without upsampling (surface/include/pcl/surface/mls.h, impl/mls.hpp)
    over pclhip_mls_process: polynomial orders 0 .. 2, the projection methods NONE and SIMPLE.  The input is an
    (n, c >= 3) float32 cloud, numpy or a torch CUDA tensor; the outputs come back in the same kind of array, one record per
    input point with at least 3 neighbours, in ascending input index."""
    NONE, SIMPLE, ORTHOGONAL = 0, 1, 2                                    # MLSResult::ProjectionMethod
    UPSAMPLING_NONE, DISTINCT_CLOUD, SAMPLE_LOCAL_PLANE, RANDOM_UNIFORM_DENSITY, VOXEL_GRID_DILATION = range(5)

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.tree = None
        self.cloud = None
        self.search_radius = 0.0       # mls.h:297-313: the reference's defaults
        self.sqr_gauss_param = 0.0
        self.order = 2
        self.projection_method = self.SIMPLE
        self.compute_normals = False
        self._indices = None
        self._double = None

    def getClassName(self):
        return "MovingLeastSquares"

    def setInputCloud(self, cloud):
        self.cloud = cloud

    def getInputCloud(self):
        return self.cloud

    def setSearchMethod(self, tree):
        """An index over the same whole, unscaled cloud (a KdTree another stage built) is reused as it is."""
        self.tree = tree

    def getSearchMethod(self):
        return self.tree

    def setSearchRadius(self, r):
        """mls.h:365: also sets sqr_gauss_param = r * r."""
        self.search_radius = float(r)
        self.sqr_gauss_param = self.search_radius * self.search_radius

    def getSearchRadius(self):
        return self.search_radius

    def setSqrGaussParam(self, s):
        self.sqr_gauss_param = float(s)

    def getSqrGaussParam(self):
        return self.sqr_gauss_param

    def setPolynomialOrder(self, order):
        self.order = int(order)

    def getPolynomialOrder(self):
        return self.order

    def setProjectionMethod(self, method):
        self.projection_method = int(method)

    def getProjectionMethod(self):
        return self.projection_method

    def setComputeNormals(self, compute_normals):
        self.compute_normals = bool(compute_normals)

    def setUpsamplingMethod(self, method):
        if int(method) != self.UPSAMPLING_NONE:
            raise NotImplementedError("MovingLeastSquares: upsampling is not built")

    def setNumberOfThreads(self, n=0):
        pass

    def lastPassMs(self):
        """GPU time (ms) of the plane kernel and of the fit kernel of the last process()."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self.lib.pclhip_index_last_mls_ms(self.tree.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def lastKernelMs(self):
        return float(self.lib.pclhip_index_last_kernel_ms(self.tree.h))

    def _run(self, want_double):
        assert self.cloud is not None, "setInputCloud first"
        if self.tree is None:
            self.tree = KdTree(self.ctx)
        if self.tree.h is None or self.tree._cloud_id != (id(self.cloud), None):
            self.tree.setInputCloud(self.cloud)
        n = self.tree.n_cloud
        if _is_torch(self.cloud):
            import torch

            def make(shape, dtype):
                t = torch.empty(shape, dtype={np.int32: torch.int32, np.float32: torch.float32,
                                              np.float64: torch.float64}[dtype], device=self.cloud.device)
                return t, C.c_void_p(t.data_ptr())
        else:
            def make(shape, dtype):
                a = np.empty(shape, dtype)
                return a, C.c_void_p(a.ctypes.data)
        pts, pp = make((max(n, 1), 3), np.float32)
        nrm, npp = make((max(n, 1), 4), np.float32) if self.compute_normals else (None, None)
        idx, ip = make(max(n, 1), np.int32)
        dbl, dp = make((max(n, 1), 8), np.float64) if want_double else (None, None)
        k = C.c_uint64(0)
        check(self.lib.pclhip_mls_process(self.tree.h, self.search_radius, self.sqr_gauss_param, self.order,
                                          self.projection_method, pp, npp, ip, n, C.byref(k), dp), self.ctx.h)
        k = int(k.value)
        self._indices = idx[:k]
        self._double = None if dbl is None else dbl[:k]
        if nrm is None:
            return pts[:k], None, None, self._indices
        return pts[:k], nrm[:k, :3], nrm[:k, 3], self._indices

    def process(self):
        """-> (points float32 [k, 3], normals float32 [k, 3], curvature float32 [k], corresponding indices int32 [k]);
        normals and curvature are None without setComputeNormals(True)."""
        return self._run(False)

    def processAll(self):
        """process() and the unrounded records: float64 [k, 8] = point (3), normal (3), curvature, neighbour count."""
        out = self._run(True)
        return out + (self._double,)

    def getCorrespondingIndices(self):
        return self._indices


class EuclideanClusterExtraction:
    """pcl::EuclideanClusterExtraction<PointT> (segmentation/include/pcl/segmentation/extract_clusters.h:330-435,
    impl/extract_clusters.hpp:124-253) over pclhip_euclidean_clusters.  The input is an (n, c >= 3) float32 cloud, numpy or
    a torch CUDA tensor; the clusters come back in the same kind of array, largest first, ties by smallest index."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self._tree = None
        self._cloud = None
        self._indices = None
        self._tolerance = 0.0                 # extract_clusters.h:360-435: the reference's defaults
        self._min = 1
        self._max = 0xFFFFFFFF
        self._labels = None
        self._ms = 0.0

    def getClassName(self):
        return "EuclideanClusterExtraction"

    def setInputCloud(self, cloud):
        self._cloud = cloud

    def getInputCloud(self):
        return self._cloud

    def setIndices(self, indices):
        """PCLBase::setIndices: only these records are clustered (None: every record)."""
        self._indices = indices

    def getIndices(self):
        return self._indices

    def setSearchMethod(self, tree):
        self._tree = tree

    def getSearchMethod(self):
        return self._tree

    def setClusterTolerance(self, tolerance):
        self._tolerance = float(tolerance)

    def getClusterTolerance(self):
        return self._tolerance

    def setMinClusterSize(self, n):
        self._min = int(n)

    def getMinClusterSize(self):
        return self._min

    def setMaxClusterSize(self, n):
        self._max = int(n)

    def getMaxClusterSize(self):
        return self._max

    def lastKernelMs(self):
        """GPU time of the last extract() (all of its kernels)."""
        return self._ms

    def lastStats(self):
        """dict(hook_ms, flatten_ms, unions) of the last extract(): the two union-find kernels and the unions attempted."""
        a, b, u = C.c_double(0.0), C.c_double(0.0), C.c_uint64(0)
        self.lib.pclhip_index_last_cluster_stats(self._tree.h, C.byref(a), C.byref(b), C.byref(u))
        return dict(hook_ms=a.value, flatten_ms=b.value, unions=int(u.value))

    def extractCSR(self):
        """-> (offsets uint64 [k + 1] (numpy), indices int32 [n_clustered], labels int32 [n]) of one call; indices and
        labels are torch device tensors for a torch cloud."""
        assert self._cloud is not None, "setInputCloud first"
        if self._tree is None:
            self._tree = KdTree(self.ctx)
        key = (id(self._cloud), None if self._indices is None else id(self._indices))
        if self._tree.h is None or self._tree._cloud_id != key:  # a tree built for another cloud or index set
            self._tree.setInputCloud(self._cloud, self._indices)
        n = self._tree.n_cloud
        offsets = np.zeros(n + 1, np.uint64)
        if _is_torch(self._cloud):
            import torch
            labels = torch.empty(n, dtype=torch.int32, device=self._cloud.device)
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=self._cloud.device)
            lp, ip = C.c_void_p(labels.data_ptr()), C.c_void_p(idx.data_ptr())
        else:
            labels = np.empty(n, np.int32)
            idx = np.empty(max(n, 1), np.int32)
            lp, ip = C.c_void_p(labels.ctypes.data), C.c_void_p(idx.ctypes.data)
        k, nc = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.pclhip_euclidean_clusters(self._tree.h, self._tolerance, max(self._min, 0), min(self._max, 0xFFFFFFFF),
                                                 lp, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), n + 1, ip, n,
                                                 C.byref(k), C.byref(nc)), self.ctx.h)
        self._ms = float(self.lib.pclhip_index_last_kernel_ms(self._tree.h))
        self._labels = labels
        return offsets[:k.value + 1], idx[:nc.value], labels

    def extract(self):
        """extract(std::vector<PointIndices>&): a list of ascending int32 index arrays."""
        offsets, idx, _ = self.extractCSR()
        off = offsets.astype(np.int64).tolist()
        return [idx[off[c]:off[c + 1]] for c in range(len(off) - 1)]

    def labels(self):
        """Per record of the cloud: the rank of its cluster in the last extract(), -1 for a record in no returned cluster."""
        return self._labels


class RegionGrowing:
    """pcl::RegionGrowing<PointT, NormalT> (segmentation/include/pcl/segmentation/region_growing.h:66-340,
    impl/region_growing.hpp:231-548) over pclhip_region_growing: smooth mode, curvature test on, no residual test.  The
    cloud is (n, c >= 3) float32, the normals (n, c >= 4) float32 = (nx, ny, nz, curvature), what NormalEstimation.compute()
    returns; numpy or torch CUDA tensors.  The segments come back in the order their seeds were taken."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.p = _lib.RegionGrowingParams()
        self.lib.pclhip_region_growing_params_default(C.byref(self.p))
        self._min = int(self.p.min_cluster_size)
        self._max = int(self.p.max_cluster_size)
        self._tree = None
        self._cloud = None
        self._indices = None
        self._normals = None
        self._labels = None
        self._last = None      # (offsets, indices) of the last extract
        self._ms = 0.0

    def getClassName(self):
        return "RegionGrowing"

    def setInputCloud(self, cloud):
        self._cloud = cloud

    def getInputCloud(self):
        return self._cloud

    def setIndices(self, indices):
        """PCLBase::setIndices: only these records are segmented (None: every record)."""
        self._indices = indices

    def getIndices(self):
        return self._indices

    def setSearchMethod(self, tree):
        self._tree = tree

    def getSearchMethod(self):
        return self._tree

    def setInputNormals(self, normals):
        self._normals = normals

    def getInputNormals(self):
        return self._normals

    def setNumberOfNeighbours(self, k):
        self.p.number_of_neighbours = int(k)

    def getNumberOfNeighbours(self):
        return int(self.p.number_of_neighbours)

    def setSmoothnessThreshold(self, theta):
        self.p.smoothness_threshold = float(theta)

    def getSmoothnessThreshold(self):
        return float(self.p.smoothness_threshold)

    def setCurvatureThreshold(self, curvature):
        self.p.curvature_threshold = float(curvature)

    def getCurvatureThreshold(self):
        return float(self.p.curvature_threshold)

    def setMinClusterSize(self, n):
        self._min = int(n)

    def getMinClusterSize(self):
        return self._min

    def setMaxClusterSize(self, n):
        self._max = int(n)

    def getMaxClusterSize(self):
        return self._max

    def getSmoothModeFlag(self):
        return True

    def setSmoothModeFlag(self, value):
        if not value:
            raise NotImplementedError("RegionGrowing: only the smooth mode is built (the other tests every neighbour against "
                                      "the initial seed's normal)")

    def getCurvatureTestFlag(self):
        return True

    def setCurvatureTestFlag(self, value):
        """region_growing.hpp:120-126: switching the curvature test off switches the residual test on."""
        if not value:
            raise NotImplementedError("RegionGrowing: without the curvature test the reference turns the residual test on, "
                                      "which is not built (its result depends on the flood's order inside a region)")

    def getResidualTestFlag(self):
        return False

    def setResidualTestFlag(self, value):
        if value:
            raise NotImplementedError("RegionGrowing: the residual test is not built (its result depends on the flood's "
                                      "order inside a region)")

    def setResidualThreshold(self, residual):
        self.p.residual_threshold = float(residual)

    def getResidualThreshold(self):
        return float(self.p.residual_threshold)

    def lastKernelMs(self):
        """GPU time of the last extract() (all of its kernels)."""
        return self._ms

    def lastStats(self):
        """dict(lists_ms, collapse_ms, phase1_ms, phase2_ms, phase1_rounds, phase2_rounds, unions, leftover) of the last
        extract()."""
        ms = [C.c_double(0.0) for _ in range(4)]
        r1, r2, u, left = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self.lib.pclhip_index_last_region_growing_stats(self._tree.h, C.byref(ms[0]), C.byref(ms[1]), C.byref(ms[2]),
                                                        C.byref(ms[3]), C.byref(r1), C.byref(r2), C.byref(u), C.byref(left))
        return dict(lists_ms=ms[0].value, collapse_ms=ms[1].value, phase1_ms=ms[2].value, phase2_ms=ms[3].value,
                    phase1_rounds=int(r1.value), phase2_rounds=int(r2.value), unions=int(u.value), leftover=int(left.value))

    def _empty(self, n):
        if _is_torch(self._cloud):
            import torch
            labels = torch.full((n,), -1, dtype=torch.int32, device=self._cloud.device)
            idx = torch.empty(0, dtype=torch.int32, device=self._cloud.device)
        else:
            labels = np.full(n, -1, np.int32)
            idx = np.empty(0, np.int32)
        self._labels = labels
        self._last = (np.zeros(1, np.uint64), idx)
        self._ms = 0.0
        return self._last[0], idx, labels

    def extractCSR(self):
        """-> (offsets uint64 [k + 1] (numpy), indices int32 [n_clustered], labels int32 [n]) of one call; indices and
        labels are torch device tensors for a torch cloud.  No cloud, no normals, normals of another size or
        number_of_neighbours == 0: no segment (prepareForSegmentation, region_growing.hpp:278-304)."""
        n = 0 if self._cloud is None else int(self._cloud.shape[0])
        if n == 0 or self._normals is None or int(self._normals.shape[0]) != n or self.p.number_of_neighbours == 0:
            return self._empty(n)
        if self._tree is None:
            self._tree = KdTree(self.ctx)
        key = (id(self._cloud), None if self._indices is None else id(self._indices))
        if self._tree.h is None or self._tree._cloud_id != key:  # a tree built for another cloud or index set
            self._tree.setInputCloud(self._cloud, self._indices)
        assert self._normals.shape[1] >= 4, "the normals are (nx, ny, nz, curvature) records"
        nptr, nstride, _, keep = _cloud(self._normals)
        offsets = np.zeros(n + 1, np.uint64)
        if _is_torch(self._cloud):
            import torch
            labels = torch.empty(n, dtype=torch.int32, device=self._cloud.device)
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=self._cloud.device)
            lp, ip = C.c_void_p(labels.data_ptr()), C.c_void_p(idx.data_ptr())
        else:
            labels = np.empty(n, np.int32)
            idx = np.empty(max(n, 1), np.int32)
            lp, ip = C.c_void_p(labels.ctypes.data), C.c_void_p(idx.ctypes.data)
        self.p.min_cluster_size = min(max(self._min, 0), 0xFFFFFFFF)
        self.p.max_cluster_size = min(max(self._max, 0), 0xFFFFFFFF)
        k, nc = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.pclhip_region_growing(self._tree.h, nptr, nstride, C.byref(self.p), lp,
                                             offsets.ctypes.data_as(C.POINTER(C.c_uint64)), n + 1, ip, n, C.byref(k),
                                             C.byref(nc)), self.ctx.h)
        del keep
        self._ms = float(self.lib.pclhip_index_last_kernel_ms(self._tree.h))
        self._labels = labels
        self._last = (offsets[:k.value + 1], idx[:nc.value])
        return self._last[0], self._last[1], labels

    def extract(self):
        """extract(std::vector<PointIndices>&): a list of ascending int32 index arrays."""
        offsets, idx, _ = self.extractCSR()
        off = offsets.astype(np.int64).tolist()
        return [idx[off[c]:off[c + 1]] for c in range(len(off) - 1)]

    def labels(self):
        """Per record of the cloud: the number of its segment in the last extract(), -1 for a record in no returned one."""
        return self._labels

    def getSegmentFromPoint(self, index):
        """The segment of the last extract() that holds record `index`; empty when it is in no returned segment.  (The
        reference runs the segmentation if none has been run; so does this.)"""
        if self._last is None:
            self.extractCSR()
        offsets, idx = self._last
        lab = int(self._labels[int(index)]) if 0 <= int(index) < len(self._labels) else -1
        if lab < 0:
            return idx[:0]
        return idx[int(offsets[lab]):int(offsets[lab + 1])]


class SACSegmentation:
    """pcl::SACSegmentation<PointT> (segmentation/include/pcl/segmentation/sac_segmentation.h:77-330,
    impl/sac_segmentation.hpp:79-133,230-262) for SACMODEL_PLANE, SACMODEL_PERPENDICULAR_PLANE and SACMODEL_PARALLEL_PLANE
    (setAxis, setEpsAngle) under SAC_RANSAC, over pclhip_sac_segment_plane and pclhip_sac_segment_model.  The input is an
    (n, c >= 3) float32 cloud, numpy or a torch CUDA tensor; the index lists come back in the same kind of array.  The draws
    are a pure function of (seed, trial, slot) (include/pclhip.h): setSeed."""

    _MODELS = (_lib.SACMODEL_PLANE, _lib.SACMODEL_PERPENDICULAR_PLANE, _lib.SACMODEL_PARALLEL_PLANE)
    _NORMAL_MODELS = (_lib.SACMODEL_NORMAL_PLANE, _lib.SACMODEL_NORMAL_PARALLEL_PLANE)

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.p = _lib.SacPlaneParams()
        self.lib.pclhip_sac_plane_params_default(C.byref(self.p))
        self.m = _lib.SacModelParams()
        self.lib.pclhip_sac_model_params_default(C.byref(self.m))
        self._normals = None
        self._model = -1       # sac_segmentation.h:83-84: neither is set by default
        self._method = 0
        self._cloud = None
        self._indices = None
        self._outliers = None
        self._stats = None

    def getClassName(self):
        return "SACSegmentation"

    def setModelType(self, model):
        model = int(model)
        if model not in self._MODELS:
            if model in self._NORMAL_MODELS:  # sac_segmentation.hpp:136-370: SACSegmentation builds no model with normals
                raise ValueError("%s: model type %d needs SACSegmentationFromNormals" % (self.getClassName(), model))
            raise NotImplementedError("%s: only the plane models %s are built" % (self.getClassName(), list(self._MODELS)))
        self._model = model
        self.m.model_type = model

    def getModelType(self):
        return self._model

    def setAxis(self, axis):
        """The axis of the constrained planes: the normal's for SACMODEL_PERPENDICULAR_PLANE and
        SACMODEL_NORMAL_PARALLEL_PLANE, one the plane runs along for SACMODEL_PARALLEL_PLANE."""
        a = np.asarray(axis, np.float32).reshape(3)
        self.m.axis[0], self.m.axis[1], self.m.axis[2] = float(a[0]), float(a[1]), float(a[2])

    def getAxis(self):
        return np.array(self.m.axis, np.float32)

    def setEpsAngle(self, eps_angle):
        """The largest deviation from the axis, in radians (0: no constraint)."""
        self.m.eps_angle = float(eps_angle)

    def getEpsAngle(self):
        return float(self.m.eps_angle)

    def setMethodType(self, method):
        if int(method) != _lib.SAC_RANSAC:
            raise NotImplementedError("SACSegmentation: only SAC_RANSAC is built")
        self._method = int(method)

    def getMethodType(self):
        return self._method

    def setDistanceThreshold(self, threshold):
        self.p.distance_threshold = float(threshold)

    def getDistanceThreshold(self):
        return float(self.p.distance_threshold)

    def setMaxIterations(self, n):
        self.p.max_iterations = int(n)

    def getMaxIterations(self):
        return int(self.p.max_iterations)

    def setProbability(self, probability):
        self.p.probability = float(probability)

    def getProbability(self):
        return float(self.p.probability)

    def setOptimizeCoefficients(self, optimize):
        self.p.optimize_coefficients = int(bool(optimize))

    def getOptimizeCoefficients(self):
        return bool(self.p.optimize_coefficients)

    def setSeed(self, seed):
        self.p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def getSeed(self):
        return int(self.p.seed)

    def setBatchSize(self, n):
        """Trials per scoring pass (0: automatic); never changes a result."""
        self.p.batch_size = int(n)

    def setInputCloud(self, cloud):
        self._cloud = cloud

    def getInputCloud(self):
        return self._cloud

    def setIndices(self, indices):
        """PCLBase::setIndices: the point set, in this order (None: every record)."""
        self._indices = indices

    def getIndices(self):
        return self._indices

    def _inputs(self):
        assert self._cloud is not None, "setInputCloud first"
        if self._model < 0:
            raise ValueError("SACSegmentation: no model type was set (setModelType(SACMODEL_PLANE))")
        ptr, stride, n, keep = _cloud(self._cloud)
        idx, ip, ni = None, None, 0
        if self._indices is not None:
            if _is_torch(self._indices):
                import torch
                idx = self._indices.to(torch.int32).contiguous()
                ip, ni = C.c_void_p(idx.data_ptr()), int(idx.numel())
            else:
                idx = np.ascontiguousarray(self._indices, np.int32).reshape(-1)
                ip, ni = C.c_void_p(idx.ctypes.data), len(idx)
            if ni == 0:  # an empty point set, not "every record"
                idx = np.zeros(1, np.int32)
                ip = C.c_void_p(idx.ctypes.data)
        return ptr, stride, n, ip, ni, (keep, idx)

    def _through_model(self):
        """the call goes through pclhip_sac_segment_model / _evaluate (the plain plane keeps the plane's entry points)"""
        return self._model != _lib.SACMODEL_PLANE

    def _normal_records(self, n):
        """-> (pointer, stride_bytes, keepalive) of the (n, >= 4) normal records; (None, 0, None) without normals"""
        if self._normals is None:
            return None, 0, None
        nptr, nstride, nn, nkeep = _cloud_rows(self._normals)
        if nn != n or nstride < 16:
            raise ValueError("%s: the normals must be (n, >= 4) records (nx, ny, nz, curvature), one per record of the cloud"
                             % self.getClassName())
        return nptr, nstride, nkeep

    def segment(self, inliers_capacity=None, outliers_capacity=None):
        """segment(PointIndices&, ModelCoefficients&) -> (inliers int32, coefficients float32 [4]); both empty when no model
        was found.  getOutliers() gives the rest of the point set.  The capacities default to the size of the point set."""
        ptr, stride, n, ip, ni, keep = self._inputs()
        m = ni if self._indices is not None else n
        cap_in = m if inliers_capacity is None else int(inliers_capacity)
        cap_out = m if outliers_capacity is None else int(outliers_capacity)
        if _is_torch(self._cloud):
            import torch
            inl = torch.empty(max(cap_in, 1), dtype=torch.int32, device=self._cloud.device)
            outl = torch.empty(max(cap_out, 1), dtype=torch.int32, device=self._cloud.device)
            pin, pout = C.c_void_p(inl.data_ptr()), C.c_void_p(outl.data_ptr())
        else:
            inl = np.empty(max(cap_in, 1), np.int32)
            outl = np.empty(max(cap_out, 1), np.int32)
            pin, pout = C.c_void_p(inl.ctypes.data), C.c_void_p(outl.ctypes.data)
        coeff = np.zeros(4, np.float32)
        n_in, n_out = C.c_uint64(0), C.c_uint64(0)
        st = _lib.SacPlaneStats()
        self._outliers = None
        self._stats = None
        if self._through_model():
            nptr, nstride, nkeep = self._normal_records(n)
            rc = self.lib.pclhip_sac_segment_model(self.ctx.h, ptr, n, stride, nptr, nstride, ip, ni, C.byref(self.p),
                                                   C.byref(self.m), _fp(coeff), pin, cap_in, C.byref(n_in), pout, cap_out,
                                                   C.byref(n_out), C.byref(st))
        else:
            rc = self.lib.pclhip_sac_segment_plane(self.ctx.h, ptr, n, stride, ip, ni, C.byref(self.p), _fp(coeff), pin, cap_in,
                                                   C.byref(n_in), pout, cap_out, C.byref(n_out), C.byref(st))
        self._stats = dict(trials=int(st.trials), iterations=int(st.iterations), skipped=int(st.skipped),
                           batches=int(st.batches), best_trial=int(st.best_trial), best_count=int(st.best_count),
                           refined=bool(st.refined), count_ms=float(st.count_ms), total_ms=float(st.total_ms),
                           n_inliers=int(n_in.value), n_outliers=int(n_out.value))
        check(rc, self.ctx.h)
        self._outliers = outl[:n_out.value]
        if st.best_trial < 0:
            return inl[:0], np.zeros(0, np.float32)
        return inl[:n_in.value], coeff

    def getOutliers(self):
        """The entries of the point set (cloud indices) that the last segment() left over, in the set's order
        (ExtractIndices::setNegative(true) on its inliers)."""
        return self._outliers

    def lastStats(self):
        """dict of the last segment(): trials, iterations, skipped, batches, best_trial, best_count, refined, count_ms (GPU
        time of the scoring launches), total_ms (GPU time of the call), n_inliers, n_outliers."""
        return self._stats

    def trace(self, capacity=65536):
        """One dict per trial the last segment() consumed: samples, skipped, coefficients, count, valid (False for a
        skipped trial and for a hypothesis that failed its model's gate: isModelValid)."""
        n = C.c_uint64(0)
        check(self.lib.pclhip_sac_last_model_trace(self.ctx.h, None, 0, C.byref(n)), self.ctx.h)
        m = min(int(n.value), int(capacity))
        buf = (_lib.SacModelTrace * max(1, m))()
        check(self.lib.pclhip_sac_last_model_trace(self.ctx.h, buf, m, C.byref(n)), self.ctx.h)
        return [dict(samples=list(t.samples), skipped=bool(t.skipped), coefficients=np.array(t.coefficients, np.float32),
                     count=int(t.count), valid=bool(t.valid)) for t in buf[:m]]

    def evaluate(self, models):
        """countWithinDistance and isModelValid of (H, 4) coefficient rows -> ((H,) uint32 counts, (H,) bool valid)."""
        ptr, stride, n, ip, ni, keep = self._inputs()
        M = np.ascontiguousarray(models, np.float32).reshape(-1, 4)
        cnt = np.zeros(len(M), np.uint32)
        valid = np.ones(len(M), np.uint8)
        if self._through_model():
            nptr, nstride, nkeep = self._normal_records(n)
            check(self.lib.pclhip_sac_model_evaluate(self.ctx.h, ptr, n, stride, nptr, nstride, ip, ni,
                                                     float(self.p.distance_threshold), C.byref(self.m), _fp(M), len(M),
                                                     C.c_void_p(cnt.ctypes.data), C.c_void_p(valid.ctypes.data)), self.ctx.h)
        else:
            check(self.lib.pclhip_sac_plane_evaluate(self.ctx.h, ptr, n, stride, ip, ni, float(self.p.distance_threshold), _fp(M),
                                                     len(M), C.c_void_p(cnt.ctypes.data)), self.ctx.h)
        return cnt, valid.astype(bool)

    def countWithinDistance(self, models):
        """SampleConsensusModel::countWithinDistance of (H, 4) coefficient rows over the point set, batched ->
        (H,) uint32 (0 for a hypothesis that fails its model's gate)."""
        return self.evaluate(models)[0]


class SACSegmentationFromNormals(SACSegmentation):
    """pcl::SACSegmentationFromNormals<PointT, PointNT> (segmentation/include/pcl/segmentation/sac_segmentation.h:305-415,
    impl/sac_segmentation.hpp:374-531) for the plane models: SACMODEL_NORMAL_PLANE and SACMODEL_NORMAL_PARALLEL_PLANE score
    with the points' normals (include/pclhip.h), the three models of SACSegmentation are built as there.  The normals are
    (n, >= 4) float32 records (nx, ny, nz, curvature), one per record of the cloud (what NormalEstimation.compute() returns),
    numpy or a torch CUDA tensor; every call needs them, as the reference's does.  Every model goes through
    pclhip_sac_segment_model."""

    _MODELS = SACSegmentation._MODELS + SACSegmentation._NORMAL_MODELS
    _NORMAL_MODELS = ()

    def getClassName(self):
        return "SACSegmentationFromNormals"

    def setInputNormals(self, normals):
        self._normals = normals

    def getInputNormals(self):
        return self._normals

    def setNormalDistanceWeight(self, weight):
        """The share of the angle between a point's normal and the plane's in the distance (default 0.1)."""
        self.m.normal_distance_weight = float(weight)

    def getNormalDistanceWeight(self):
        return float(self.m.normal_distance_weight)

    def setDistanceFromOrigin(self, d):
        """SACMODEL_NORMAL_PARALLEL_PLANE's distance from the origin.  The class sets no tolerance for it
        (sac_segmentation.hpp:440-468), so it constrains nothing; the C interface has eps_dist."""
        self.m.distance_from_origin = float(d)

    def getDistanceFromOrigin(self):
        return float(self.m.distance_from_origin)

    def _through_model(self):
        return True

    def _normal_records(self, n):
        if self._normals is None:  # sac_segmentation.hpp:376-380
            raise ValueError("SACSegmentationFromNormals: setInputNormals first")
        return super()._normal_records(n)


def _index_list(indices):
    """-> (pointer, count, keepalive) of an int32 list, numpy or torch; an empty list still has a pointer"""
    if _is_torch(indices):
        import torch
        idx = indices.to(torch.int32).contiguous()
        if idx.numel() > 0:
            return C.c_void_p(idx.data_ptr()), int(idx.numel()), idx
        indices = np.zeros(0, np.int32)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
    n = len(idx)
    if n == 0:
        idx = np.zeros(1, np.int32)
    return C.c_void_p(idx.ctypes.data), n, idx


class SampleConsensusModelCylinder:
    """pcl::SampleConsensusModelCylinder<PointT, PointNT> (sample_consensus/include/pcl/sample_consensus/
    sac_model_cylinder.h, impl/sac_model_cylinder.hpp) over the pclhip_sac_cylinder_* calls (include/pclhip.h states the
    semantics).  The cloud is (n, c >= 3) float32, the normals (n, >= 4) float32 records (nx, ny, nz, curvature), numpy or
    torch CUDA tensors; `indices` is the point set (None: every record).  Coefficients: (line_pt, line_dir, radius), 7 floats.
    The segmentation classes still refuse SACMODEL_CYLINDER: run this model with RandomSampleConsensus.  Not built:
    projectPoints, doSamplesVerifyModel, setSamplesMaxDist."""

    def __init__(self, cloud, indices=None, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.m = _lib.SacCylinderParams()
        self.lib.pclhip_sac_cylinder_params_default(C.byref(self.m))
        self._cloud = cloud
        self._indices = indices
        self._normals = None

    def setInputCloud(self, cloud):
        self._cloud = cloud

    def getInputCloud(self):
        return self._cloud

    def setIndices(self, indices):
        self._indices = indices

    def getIndices(self):
        return self._indices

    def setInputNormals(self, normals):
        self._normals = normals

    def getInputNormals(self):
        return self._normals

    def setNormalDistanceWeight(self, weight):
        self.m.normal_distance_weight = float(weight)

    def getNormalDistanceWeight(self):
        return float(self.m.normal_distance_weight)

    def setRadiusLimits(self, min_radius, max_radius):
        self.m.radius_min, self.m.radius_max = float(min_radius), float(max_radius)

    def getRadiusLimits(self):
        return float(self.m.radius_min), float(self.m.radius_max)

    def setAxis(self, axis):
        a = np.asarray(axis, np.float32).reshape(3)
        self.m.axis[0], self.m.axis[1], self.m.axis[2] = float(a[0]), float(a[1]), float(a[2])

    def getAxis(self):
        return np.array(self.m.axis, np.float32)

    def setEpsAngle(self, eps_angle):
        self.m.eps_angle = float(eps_angle)

    def getEpsAngle(self):
        return float(self.m.eps_angle)

    def getSampleSize(self):
        return 2

    def getModelSize(self):
        return 7

    def _inputs(self):
        """-> (cloud ptr, n, stride, normals ptr, normals stride, indices ptr, indices count, keepalive)"""
        assert self._cloud is not None, "the model has no cloud"
        ptr, stride, n, keep = _cloud(self._cloud)
        if self._normals is None:  # impl/sac_model_cylinder.hpp:85-89
            raise ValueError("SampleConsensusModelCylinder: setInputNormals first")
        nptr, nstride, nn, nkeep = _cloud_rows(self._normals)
        if nn != n or nstride < 16:
            raise ValueError("SampleConsensusModelCylinder: the normals must be (n, >= 4) records (nx, ny, nz, curvature), "
                             "one per record of the cloud")
        ip, ni, ikeep = (None, 0, None) if self._indices is None else _index_list(self._indices)
        return ptr, n, stride, nptr, nstride, ip, ni, (keep, nkeep, ikeep)

    def _set_size(self, n, ni):
        return ni if self._indices is not None else n

    @staticmethod
    def _coeff(coeff):
        c = np.ascontiguousarray(coeff, np.float32).reshape(-1)
        if len(c) != 7:  # sac_model.h: isModelValid refuses another size
            raise ValueError("SampleConsensusModelCylinder: 7 coefficients (line_pt, line_dir, radius), got %d" % len(c))
        return c

    def computeModelCoefficients(self, samples):
        """-> the 7 coefficients of the two samples (cloud indices, in this order), or None where the reference returns false
        (identical points, a radius outside the limits)"""
        ptr, n, stride, nptr, nstride, ip, ni, keep = self._inputs()
        s = np.ascontiguousarray(samples, np.int32).reshape(-1)
        if len(s) != 2:  # :52-56
            raise ValueError("SampleConsensusModelCylinder: a sample holds 2 indices, got %d" % len(s))
        coeff = np.zeros(7, np.float32)
        found = C.c_int(0)
        check(self.lib.pclhip_sac_cylinder_model(self.ctx.h, ptr, n, stride, nptr, nstride,
                                                 s.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(self.m), _fp(coeff),
                                                 C.byref(found)), self.ctx.h)
        return coeff if found.value else None

    def evaluate(self, coeffs, threshold):
        """countWithinDistance and isModelValid of (H, 7) coefficient rows -> ((H,) uint32 counts, (H,) bool valid)"""
        ptr, n, stride, nptr, nstride, ip, ni, keep = self._inputs()
        M = np.ascontiguousarray(coeffs, np.float32).reshape(-1, 7)
        cnt = np.zeros(len(M), np.uint32)
        valid = np.ones(len(M), np.uint8)
        check(self.lib.pclhip_sac_cylinder_evaluate(self.ctx.h, ptr, n, stride, nptr, nstride, ip, ni, float(threshold),
                                                    C.byref(self.m), _fp(M), len(M), C.c_void_p(cnt.ctypes.data),
                                                    C.c_void_p(valid.ctypes.data)), self.ctx.h)
        return cnt, valid.astype(bool)

    def countWithinDistance(self, coeff, threshold):
        return int(self.evaluate(self._coeff(coeff), threshold)[0][0])

    def selectWithinDistance(self, coeff, threshold):
        """-> the inliers (cloud indices in the point set's order), int32: a torch tensor for a torch cloud"""
        ptr, n, stride, nptr, nstride, ip, ni, keep = self._inputs()
        c = self._coeff(coeff)
        m = max(self._set_size(n, ni), 1)
        if _is_torch(self._cloud):
            import torch
            inl = torch.empty(m, dtype=torch.int32, device=self._cloud.device)
            pin = C.c_void_p(inl.data_ptr())
        else:
            inl = np.empty(m, np.int32)
            pin = C.c_void_p(inl.ctypes.data)
        n_in = C.c_uint64(0)
        check(self.lib.pclhip_sac_cylinder_select(self.ctx.h, ptr, n, stride, nptr, nstride, ip, ni, float(threshold),
                                                  C.byref(self.m), _fp(c), pin, m, C.byref(n_in)), self.ctx.h)
        return inl[:n_in.value]

    def getDistancesToModel(self, coeff):
        """-> (n,) float64, one per entry of the point set; empty for a model that fails isModelValid"""
        ptr, n, stride, nptr, nstride, ip, ni, keep = self._inputs()
        c = self._coeff(coeff)
        m = max(self._set_size(n, ni), 1)
        dist = np.empty(m, np.float64)
        n_out = C.c_uint64(0)
        check(self.lib.pclhip_sac_cylinder_distances(self.ctx.h, ptr, n, stride, nptr, nstride, ip, ni, C.byref(self.m), _fp(c),
                                                     C.c_void_p(dist.ctypes.data), m, C.byref(n_out)), self.ctx.h)
        return dist[:n_out.value]

    def optimizeModelCoefficients(self, inliers, coeff):
        """-> the refined coefficients (the given ones where nothing was refined); lastOptimize() tells which"""
        assert self._cloud is not None, "the model has no cloud"
        ptr, stride, n, keep = _cloud(self._cloud)
        c = self._coeff(coeff)
        ip, ni, ikeep = _index_list(inliers)
        out = np.zeros(7, np.float32)
        refined, iters = C.c_int(0), C.c_int(0)
        check(self.lib.pclhip_sac_cylinder_optimize(self.ctx.h, ptr, n, stride, ip, ni, C.byref(self.m), _fp(c), _fp(out),
                                                    C.byref(refined), C.byref(iters)), self.ctx.h)
        self._last_optimize = dict(refined=bool(refined.value), iterations=int(iters.value))
        return out

    def lastOptimize(self):
        """dict(refined, iterations: Levenberg-Marquardt steps tried) of the last optimizeModelCoefficients()"""
        return getattr(self, "_last_optimize", None)


class RandomSampleConsensus:
    """pcl::RandomSampleConsensus<PointT> (sample_consensus/include/pcl/sample_consensus/ransac.h, impl/ransac.hpp:56-217) for a
    SampleConsensusModelCylinder, over pclhip_sac_cylinder_segment without the refit.  The draws are a pure function of
    (seed, trial, slot): setSeed.  Not built: refineModel, setNumberOfThreads (the trials are scored in batches on the
    device)."""

    def __init__(self, model, threshold=None):
        if not isinstance(model, SampleConsensusModelCylinder):
            raise NotImplementedError("RandomSampleConsensus: only SampleConsensusModelCylinder is built")
        self.model = model
        self.ctx = model.ctx
        self.lib = model.lib
        self.p = _lib.SacPlaneParams()
        self.lib.pclhip_sac_plane_params_default(C.byref(self.p))
        self.p.optimize_coefficients = 0
        self.p.max_iterations = 10000       # ransac.h:90,101
        self.p.distance_threshold = float(np.finfo(np.float64).max) if threshold is None else float(threshold)
        self._reset()

    def _reset(self):
        self._inliers = None
        self._coeff = np.zeros(0, np.float32)
        self._sample = []
        self._stats = None

    def setDistanceThreshold(self, threshold):
        self.p.distance_threshold = float(threshold)

    def getDistanceThreshold(self):
        return float(self.p.distance_threshold)

    def setMaxIterations(self, n):
        self.p.max_iterations = int(n)

    def getMaxIterations(self):
        return int(self.p.max_iterations)

    def setProbability(self, probability):
        self.p.probability = float(probability)

    def getProbability(self):
        return float(self.p.probability)

    def setSeed(self, seed):
        self.p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def setBatchSize(self, n):
        """Trials per scoring pass (0: automatic); never changes a result."""
        self.p.batch_size = int(n)

    def refineModel(self, *a, **k):
        raise NotImplementedError("RandomSampleConsensus: refineModel is not built")

    def setNumberOfThreads(self, *a, **k):
        raise NotImplementedError("RandomSampleConsensus: setNumberOfThreads is not built")

    def _segment(self, optimize):
        """pclhip_sac_cylinder_segment -> (found, inliers, outliers, coefficients, stats)"""
        md = self.model
        ptr, n, stride, nptr, nstride, ip, ni, keep = md._inputs()
        m = max(md._set_size(n, ni), 1)
        if _is_torch(md._cloud):
            import torch
            inl = torch.empty(m, dtype=torch.int32, device=md._cloud.device)
            outl = torch.empty(m, dtype=torch.int32, device=md._cloud.device)
            pin, pout = C.c_void_p(inl.data_ptr()), C.c_void_p(outl.data_ptr())
        else:
            inl, outl = np.empty(m, np.int32), np.empty(m, np.int32)
            pin, pout = C.c_void_p(inl.ctypes.data), C.c_void_p(outl.ctypes.data)
        coeff = np.zeros(7, np.float32)
        n_in, n_out = C.c_uint64(0), C.c_uint64(0)
        st = _lib.SacPlaneStats()
        p = _lib.SacPlaneParams.from_buffer_copy(self.p)
        p.optimize_coefficients = int(bool(optimize))
        rc = self.lib.pclhip_sac_cylinder_segment(self.ctx.h, ptr, n, stride, nptr, nstride, ip, ni, C.byref(p), C.byref(md.m),
                                                  _fp(coeff), pin, m, C.byref(n_in), pout, m, C.byref(n_out), C.byref(st))
        check(rc, self.ctx.h)
        stats = dict(trials=int(st.trials), iterations=int(st.iterations), skipped=int(st.skipped), batches=int(st.batches),
                     best_trial=int(st.best_trial), best_count=int(st.best_count), refined=bool(st.refined),
                     count_ms=float(st.count_ms), total_ms=float(st.total_ms), n_inliers=int(n_in.value),
                     n_outliers=int(n_out.value))
        return st.best_trial >= 0, inl[:n_in.value], outl[:n_out.value], coeff, stats

    def computeModel(self):
        """-> True when a model was found (ransac.hpp:204-216)"""
        self._reset()
        found, inl, outl, coeff, stats = self._segment(False)
        self._stats = stats
        if not found:
            return False
        self._inliers, self._coeff = inl, coeff
        tr = self.trace(stats["best_trial"] + 1)
        if len(tr) > stats["best_trial"]:
            pos = tr[stats["best_trial"]]["samples"]
            ids = self.model._indices
            self._sample = [int(ids[p]) for p in pos] if ids is not None else [int(p) for p in pos]
        return True

    def segment(self, optimize=True):
        """What SACSegmentation::segment does with this model and method in ONE call (sac_segmentation.hpp:79-133):
        computeModel, optimizeModelCoefficients, selectWithinDistance -> (inliers, coefficients [7], outliers); empty lists
        and coefficients when no model was found"""
        found, inl, outl, coeff, stats = self._segment(optimize)
        self._stats = stats
        if not found:
            return inl[:0], np.zeros(0, np.float32), outl
        return inl, coeff, outl

    def getModel(self):
        """The winner's sample (cloud indices)."""
        return list(self._sample)

    def getInliers(self):
        return self._inliers if self._inliers is not None else np.zeros(0, np.int32)

    def getModelCoefficients(self):
        return self._coeff

    def stats(self):
        """dict of the last computeModel() / segment(): trials, iterations, skipped, batches, best_trial, best_count, refined,
        count_ms, total_ms, n_inliers, n_outliers"""
        return self._stats

    def trace(self, capacity=65536):
        """One dict per trial the last call consumed: samples (positions in the point set), skipped, coefficients, count,
        valid"""
        n = C.c_uint64(0)
        check(self.lib.pclhip_sac_last_cylinder_trace(self.ctx.h, None, 0, C.byref(n)), self.ctx.h)
        m = min(int(n.value), int(capacity))
        buf = (_lib.SacCylinderTrace * max(1, m))()
        check(self.lib.pclhip_sac_last_cylinder_trace(self.ctx.h, buf, m, C.byref(n)), self.ctx.h)
        return [dict(samples=list(t.samples), skipped=bool(t.skipped), coefficients=np.array(t.coefficients, np.float32),
                     count=int(t.count), valid=bool(t.valid)) for t in buf[:m]]


def featureKSearch(ctx, target_rows, query_rows, k):
    """KdTreeFLANN<FeatureT>::nearestKSearch by exact brute force over pclhip_feature_knn: (n, D) float32 rows, numpy or
    torch device tensors -> (indices (nq, k) int32, d2 (nq, k) float32, counts (nq,) uint32), ascending (d2, index); -1 /
    +inf behind the count.  A non-finite target row is never a candidate; a non-finite query row gets count 0."""
    ctx = ctx or default_context()
    tp, ts, nt, tk = _cloud_rows(target_rows)
    qp, qs, nq, qk = _cloud_rows(query_rows)
    D = tk.shape[1]
    assert qk.shape[1] == D, "target and query rows of one dimension"
    idx = np.empty((nq, int(k)), np.int32)
    d2 = np.empty((nq, int(k)), np.float32)
    cnt = np.empty(nq, np.uint32)
    check(ctx.lib.pclhip_feature_knn(ctx.h, tp, ts, nt, qp, qs, nq, D, int(k), C.c_void_p(idx.ctypes.data),
                                     C.c_void_p(d2.ctypes.data), C.c_void_p(cnt.ctypes.data)), ctx.h)
    return idx, d2, cnt


def _cloud_rows(a):
    """-> (pointer, stride_bytes, n, keepalive) of (n, D) float32 rows (any D >= 1)."""
    if _is_torch(a):
        assert a.dtype.is_floating_point and a.element_size() == 4 and a.dim() == 2
        a = a.contiguous()
        return C.c_void_p(a.data_ptr()), a.shape[1] * 4, a.shape[0], a
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2
    return C.c_void_p(a.ctypes.data), a.shape[1] * 4, a.shape[0], a


class SampleConsensusPrerejective:
    """pcl::SampleConsensusPrerejective<PointXYZ, PointXYZ, FeatureT> (registration/include/pcl/registration/
    sample_consensus_prerejective.h, impl/sample_consensus_prerejective.hpp:78-348) over pclhip_scp_*.  Clouds and features
    are numpy arrays or torch device tensors; features are (n, D) float32 rows, one per record of their cloud (D = 33:
    FPFHSignature33).  The draws are a pure function of (seed, iteration, slot) (include/pclhip.h): setSeed."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.p = _lib.ScpParams()
        self.lib.pclhip_scp_params_default(C.byref(self.p))
        self.h = None
        self.tree = None
        self.src = None
        self.target = None
        self.src_features = None
        self.tgt_features = None
        self._dirty = dict(tgt=True, src=True, sf=True, tf=True)
        self.result = None
        self.trace = []
        self.ctx._adopt(self)

    def _release(self):
        self._drop()

    def _drop(self):
        if getattr(self, "h", None):
            if self.ctx.h is not None:
                self.lib.pclhip_scp_destroy(self.h)
            self.h = None
        self._dirty = dict(tgt=True, src=True, sf=True, tf=True)

    def getClassName(self):
        return "SampleConsensusPrerejective"

    # --- inputs (sample_consensus_prerejective.h:136-160, registration.h:195-240) ---
    def setInputSource(self, cloud):
        self.src = cloud
        self._dirty["src"] = True

    def setInputTarget(self, cloud):
        self.target = cloud
        self._dirty["tgt"] = True

    def setSearchMethodTarget(self, tree, force_no_recompute=False):
        """A KdTree over the target (built over the cloud of setInputTarget when none is given)."""
        self.tree = tree
        self._dirty["tgt"] = True

    def setSourceFeatures(self, features):
        self.src_features = features
        self._dirty["sf"] = True

    def getSourceFeatures(self):
        return self.src_features

    def setTargetFeatures(self, features):
        self.tgt_features = features
        self._dirty["tf"] = True

    def getTargetFeatures(self):
        return self.tgt_features

    def setIndices(self, indices):
        if indices is not None:
            raise NotImplementedError("SampleConsensusPrerejective: source subsets (setIndices) are not supported")

    def setCommunicator(self, comm):
        raise NotImplementedError("SampleConsensusPrerejective: multi-GPU registration is not supported")

    # --- parameters (:162-232) ---
    def setNumberOfSamples(self, nr_samples):
        self.p.nr_samples = int(nr_samples)

    def getNumberOfSamples(self):
        return int(self.p.nr_samples)

    def setCorrespondenceRandomness(self, k):
        self.p.k_correspondences = int(k)

    def getCorrespondenceRandomness(self):
        return int(self.p.k_correspondences)

    def setSimilarityThreshold(self, similarity_threshold):
        self.p.similarity_threshold = float(similarity_threshold)

    def getSimilarityThreshold(self):
        return float(self.p.similarity_threshold)

    def setInlierFraction(self, inlier_fraction):
        self.p.inlier_fraction = float(inlier_fraction)

    def getInlierFraction(self):
        return float(self.p.inlier_fraction)

    def setMaximumIterations(self, n):
        self.p.max_iterations = int(n)

    def getMaximumIterations(self):
        return int(self.p.max_iterations)

    def setMaxCorrespondenceDistance(self, d):
        self.p.max_correspondence_distance = float(d)

    def getMaxCorrespondenceDistance(self):
        return float(self.p.max_correspondence_distance)

    def setSeed(self, seed):
        self.p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def getSeed(self):
        return int(self.p.seed)

    def setBatchSize(self, n):
        """Iterations per batch of launches; never changes a result."""
        self.p.batch_size = int(n)

    def _ensure(self):
        if self.target is None and (self.tree is None or self.tree.h is None):
            raise ValueError("No input target dataset was given!")
        if self.src is None:
            raise ValueError("No input source dataset was given!")
        if self._dirty["tgt"]:
            if self.h is not None:
                self._drop()
            if self.tree is None:
                self.tree = KdTree(self.ctx)
            if self.target is not None and (self.tree.h is None or self.tree._cloud_id != (id(self.target), None)):
                self.tree.setInputCloud(self.target)
            h = C.c_void_p()
            check(self.lib.pclhip_scp_create(self.tree.h, C.byref(h)), self.ctx.h)
            self.h = h
            self._dirty["tgt"] = False
        if self._dirty["src"]:
            ptr, stride, n, keep = _cloud(self.src)
            check(self.lib.pclhip_scp_set_source(self.h, ptr, stride, n), self.ctx.h)
            self._dirty["src"] = False
        for key, rows, fn in (("sf", self.src_features, self.lib.pclhip_scp_set_source_features),
                              ("tf", self.tgt_features, self.lib.pclhip_scp_set_target_features)):
            if self._dirty[key] and rows is not None:
                ptr, stride, n, keep = _cloud_rows(rows)
                check(fn(self.h, ptr, stride, n, int(keep.shape[1])), self.ctx.h)
                self._dirty[key] = False

    def align(self, guess=None, trace_capacity=0, want_output=False):
        """Registration::align -> computeTransformation (:157-306).  Returns the registered source (the input moved by the
        final transformation, transformPointCloud's order) when want_output and the alignment converged, else None; with
        trace_capacity > 0 one dict per iteration in self.trace (samples, matches, rejected, transformation, inliers,
        error)."""
        self._ensure()
        cap = int(trace_capacity)
        buf = (_lib.ScpTrace * max(1, cap))()
        check(self.lib.pclhip_scp_set_trace(self.h, buf, cap), self.ctx.h)
        r = _lib.ScpResult()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(16)
        try:
            check(self.lib.pclhip_scp_align(self.h, C.byref(self.p), _fp(g) if g is not None else None, C.byref(r)),
                  self.ctx.h)
        finally:
            self.lib.pclhip_scp_set_trace(self.h, None, 0)
        self.result = r
        ns = int(self.p.nr_samples)
        self.trace = [dict(iteration=int(t.iteration), rejected=int(t.rejected), samples=list(t.samples)[:ns],
                           matches=list(t.matches)[:ns], transformation=np.array(t.transformation, np.float32).reshape(4, 4),
                           inliers=int(t.inliers), error=np.float32(t.error)) for t in buf[:r.trace_count]]
        if not want_output or not r.converged:
            return None
        ptr, stride, n, keep = _cloud(self.src)
        out = keep.clone() if _is_torch(self.src) else keep.copy()
        optr = C.c_void_p(out.data_ptr() if _is_torch(self.src) else out.ctypes.data)
        check(self.lib.pclhip_transform_cloud(self.ctx.h, _fp(np.ascontiguousarray(self.getFinalTransformation()).reshape(16)),
                                              1, ptr, optr, stride, n, 0), self.ctx.h)
        return out

    def evaluate(self, transforms):
        """getFitness (:310-348) of (H, 4, 4) transforms in batched launches -> (counts (H,) uint32, errors (H,) float32)."""
        self._ensure()
        T = np.ascontiguousarray(transforms, np.float32).reshape(-1, 16)
        cnt = np.zeros(len(T), np.uint32)
        err = np.zeros(len(T), np.float32)
        check(self.lib.pclhip_scp_evaluate(self.h, C.byref(self.p), _fp(T), len(T), C.c_void_p(cnt.ctypes.data),
                                           C.c_void_p(err.ctypes.data)), self.ctx.h)
        return cnt, err

    def getFinalTransformation(self):
        return np.array(self.result.final_transformation, np.float32).reshape(4, 4)

    def hasConverged(self):
        return bool(self.result.converged)

    def getInliers(self):
        """The accepted hypothesis' inlier indices into the source, ascending (empty when nothing was accepted)."""
        n = C.c_uint64(0)
        check(self.lib.pclhip_scp_inliers(self.h, None, 0, C.byref(n)), self.ctx.h)
        out = np.zeros(int(n.value), np.int32)
        if len(out):
            check(self.lib.pclhip_scp_inliers(self.h, C.c_void_p(out.ctypes.data), len(out), C.byref(n)), self.ctx.h)
        return out

    def getFitnessScore(self, max_range=float(np.finfo(np.float64).max)):
        """Registration::getFitnessScore (impl/registration.hpp:132-168) with the final transformation."""
        self._ensure()
        T = np.ascontiguousarray(self.getFinalTransformation(), np.float32).reshape(16)
        score = C.c_double(0.0)
        nr = C.c_uint64(0)
        check(self.lib.pclhip_scp_fitness_score(self.h, _fp(T), C.c_double(max_range), C.byref(score), C.byref(nr)),
              self.ctx.h)
        return float(score.value)

    def lastMs(self):
        """GPU time (ms) of the feature k-NN, hypothesis and fitness launches of the last align()."""
        a, b, c = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        self.lib.pclhip_scp_last_ms(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass
