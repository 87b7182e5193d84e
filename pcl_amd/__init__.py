"""pcl_amd -- MI355X-native ICP hot path (k-NN correspondences, normals, point-to-plane ICP,
VoxelGrid) behind PCL's plugin surface.  Compute lives in libpclhip.so (pcl_amd/csrc, HIP/gfx950)
behind the C ABI of include/pclhip.h; this package is the ctypes host mirror used by tests and
bench.py.  The C++ mirror of the same surface is include/pclhip/pcl_compat.hpp."""
from . import synth  # noqa: F401
from ._lib import (POINT_TO_PLANE, POINT_TO_POINT, SAC_RANSAC, SACMODEL_NORMAL_PARALLEL_PLANE, SACMODEL_NORMAL_PLANE,  # noqa: F401
                   SACMODEL_PARALLEL_PLANE, SACMODEL_PERPENDICULAR_PLANE, SACMODEL_PLANE, SYMMETRIC, PclHipError,
                   PclHipUnavailable)
from .api import (BoundaryEstimation, Communicator, Context, CorrespondenceEstimation, CorrespondenceRejectorDistance,  # noqa: F401
                  CorrespondenceRejectorMedianDistance, CorrespondenceRejectorOneToOne, CorrespondenceRejectorSampleConsensus,
                  CorrespondenceRejectorTrimmed, DefaultConvergenceCriteria, EuclideanClusterExtraction, FPFHEstimation, GeneralizedIterativeClosestPoint,
                  ISSKeypoint3D, IterativeClosestPoint,
                  IterativeClosestPointWithNormals, KdTree, MovingLeastSquares, NormalDistributionsTransform, NormalEstimation,
                  RadiusOutlierRemoval, RandomSampleConsensus, RegionGrowing, SACSegmentation, SACSegmentationFromNormals,
                  SampleConsensusModelCylinder, SampleConsensusPrerejective,
                  StatisticalOutlierRemoval, VoxelGrid,
                  default_context, estimateRigidTransformation, featureKSearch, getPCDHeader, loadPCDField, loadPCDFile, savePCDFile)
