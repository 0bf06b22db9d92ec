"""nconv_amd — MI355X-native normalized-convolution (NConv) depth completion.

Drop-in for the hot path of lllllcf/Realtime-Depth-Estimation-Nconv (models/step1.py, models/step2.py):
the same nn.Module classes, signatures and state_dict keys, computed by hand-written gfx950 HIP
kernels behind the C ABI of include/nconv.h (libnconv.so, built in-tree).

The directory name is not a Python identifier; import it through the repo-root helper
`nconv_pkg.load()`, which registers it as the module `nconv_amd`.
"""
from . import _lib, data, dense, dp, export, frames, guided, metrics, pointcloud, train
from .nconv import EnforcePos, LayerSpec, NConv2d, NConvLayerFn, nconv_layer, weight_prep
from .dnet import DNET, SETP1_NCONV, crop_hw
from .guided import SETP2_BP_EXPORT, SETP2_BP_TRAIN, RGBEncoder
from .metrics import DepthMetrics, depth_metric_sums
from .frames import Ingest, export_depth16, ingest, write_depth_png16
from .pointcloud import (PointCloud, backproject, backproject_map, normal_image, normals, normals_and_image,
                         write_ply)
from . import lidar
from .lidar import LidarProjector, kitti_projection, project_points, projection_from_k, read_velodyne_bin
from . import visualize
from .visualize import COLORMAPS, Colorizer, colorize, overlay, write_png8
from .sparsify import Sparsifier, SparsifyBatch, sparsify
from . import occlusion
from .occlusion import OcclusionFilter, RemoveOccluded, remove_occluded
from .augment import Augment, Augmenter, augment
from .sparsification import SparsificationCurves, sparsification
from . import ipbasic
from .ipbasic import IPBasic, IPBasicFill, IPBasicFiller, ipbasic_fill
from . import nearest
from .nearest import NearestFill, NearestFiller, NearestSample, nearest_sample
from .train import ConfidenceLoss, ConfLossFn, confidence_loss
from . import warp
from .warp import (MinReprojectionLoss, MinReprojector, PhotometricLoss, ViewWarper, halve_intrinsics,
                   halve_projection, min_reprojection_loss, photometric_loss, photometric_ssim_loss, view_warp,
                   warp_projection)
from . import pose
from .pose import EstimatePose, PoseEstimator, estimate_pose, pool_sparse, pose_projection, pose_step
from . import smooth
from .smooth import EdgeWeights, Smoother, SmoothnessLoss, edge_weights, smoothness_loss
from . import consistency
from .consistency import (DepthFuser, GeometryConsistency, GeometryConsistencyLoss, depth_consistency,
                          geometry_consistency_loss, inverse_pose)
from . import voxelmap
from .voxelmap import VoxelMap, VoxelMerger, voxel_merge

__all__ = ["VoxelMap", "VoxelMerger", "voxel_merge",
           "DepthFuser", "GeometryConsistency", "GeometryConsistencyLoss", "depth_consistency",
           "geometry_consistency_loss", "inverse_pose", "EstimatePose", "PoseEstimator", "estimate_pose", "pool_sparse", "pose_projection", "pose_step",
           "EdgeWeights", "Smoother", "SmoothnessLoss", "edge_weights", "smoothness_loss", "halve_intrinsics",
           "halve_projection", "MinReprojectionLoss", "MinReprojector", "min_reprojection_loss", "PhotometricLoss", "ViewWarper", "photometric_loss", "photometric_ssim_loss", "view_warp", "warp_projection", "ConfidenceLoss", "ConfLossFn", "confidence_loss", "NearestFill", "NearestFiller", "NearestSample", "nearest_sample",
           "IPBasic", "IPBasicFill", "IPBasicFiller", "ipbasic_fill", "SparsificationCurves", "sparsification","Augment", "Augmenter", "augment","OcclusionFilter", "RemoveOccluded", "remove_occluded","Sparsifier", "SparsifyBatch", "sparsify", "COLORMAPS", "Colorizer", "colorize", "overlay", "write_png8",
"LidarProjector", "kitti_projection", "project_points", "projection_from_k", "read_velodyne_bin",
"PointCloud", "backproject", "backproject_map", "write_ply", "normals", "normal_image", "normals_and_image","EnforcePos", "LayerSpec", "NConv2d", "NConvLayerFn", "nconv_layer", "weight_prep", "DNET",
           "SETP1_NCONV", "crop_hw", "SETP2_BP_EXPORT", "SETP2_BP_TRAIN", "RGBEncoder", "DepthMetrics",
           "depth_metric_sums", "Ingest", "export_depth16", "ingest", "write_depth_png16"]
