"""ctypes binding of libnconv.so (the C ABI in include/nconv.h).

Loaded lazily on first use, after `import torch`, so the dynamic loader resolves the library's
libamdhip64.so.7 to the HIP runtime torch already mapped (one HIP runtime per process).
There is deliberately no fallback: a missing or unloadable library raises.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# NCONV_LIB: an alternative build of the same library (kernel-tuning experiments)
LIB_PATH = os.environ.get("NCONV_LIB") or os.path.join(_HERE, "libnconv.so")
ABI_VERSION = 27
BWD_ACCUMULATE = 1
BWD_DEFER_REDUCE = 2
BWD_SEPARATE = 4  # accepted and ignored since ABI 21 (include/nconv.h)
DEPTH_METRICS_SUMS = 12  # NCONV_DEPTH_METRICS_SUMS

# enum nconv_load_mode
PLAIN, THRESH, POOL2, UPCAT_SKIP_FIRST, UPCAT_UP_FIRST = 0, 1, 2, 3, 4
# enum nconv_math
MATH_FP32, MATH_BF16X3, MATH_BF16X9 = 0, 1, 2
# enum nconv_kernel (nconv_plan)
KERNEL_GENERIC, KERNEL_TILED_FP32, KERNEL_MFMA_FP32, KERNEL_MFMA_BF16X3, KERNEL_MFMA_BF16X9 = 0, 1, 2, 3, 4
KERNEL_TILED_FP32_PHASE = 5
KERNEL_NAMES = ("generic", "tiled_fp32", "mfma_fp32", "mfma_bf16x3", "mfma_bf16x9", "tiled_fp32_phase")
# enum nconv_dense_kind
DENSE_3X3, DENSE_1X1, DENSE_TRANSPOSED_4X4, DENSE_CONV4X4_S2 = 0, 1, 2, 3
# enum nconv_dense_math
DENSE_MATHS = {"fp32": 0, "bf16x9": 2, "bf16x6": 3}
# enum nconv_frame_dtype
FRAME_U8, FRAME_U16, FRAME_F32 = 0, 1, 2
# enum nconv_color_kind
COLOR_NONE, COLOR_F32_PLANAR, COLOR_U8_INTERLEAVED = 0, 1, 2
# nconv_depth_colorize.cmap_id
CMAP_IDS = {"inferno": 0, "magma": 1, "viridis": 2, "turbo": 3, "gray": 4}
# enum nconv_sparsify_mode
SPARSIFY_ALL, SPARSIFY_COUNT, SPARSIFY_COUNT_DEV, SPARSIFY_FRACTION = 0, 1, 2, 3
# enum nconv_augment_crop
AUGMENT_CROPS = {"random": 0, "center": 1, "min": 2, "max": 3}
SPARSIFICATION_MAX_STEPS = 1024  # NCONV_SPARSIFICATION_MAX_STEPS
# enum nconv_ipbasic_kernel, enum nconv_ipbasic_blur
IPBASIC_KERNELS = {"full": 0, "cross": 1, "diamond": 2}
IPBASIC_BLURS = {None: 0, "none": 0, "gaussian": 1}

EXPORTED = (
    "nconv_abi_version",
    "nconv_last_error",
    "nconv_weight_prep",
    "nconv_fwd",
    "nconv_fwd_pooled",
    "nconv_fwd_tail",
    "nconv_fwd_head",
    "nconv_head_weights",
    "nconv_plan",
    "nconv_phase_weights_floats",
    "nconv_phase_weights",
    "nconv_weight_prologue",
    "nconv_train_prologue",
    "nconv_bwd_workspace_bytes",
    "nconv_bwd",
    "nconv_bwd_ex",
    "nconv_bwd_head_workspace_bytes",
    "nconv_bwd_tail_workspace_bytes",
    "nconv_bwd_tail_conf",
    "nconv_wgrad_reduce",
    "nconv_wgrad_reduce_ex",
    "nconv_sum_workspace_bytes",
    "nconv_dense_packed_floats",
    "nconv_dense_pack",
    "nconv_dense_conv_fwd",
    "nconv_conv3x3_c1",
    "nconv_bilinear_ac",
    "nconv_dense_wgrad_workspace_bytes",
    "nconv_dense_conv_wgrad",
    "nconv_bn_workspace_bytes",
    "nconv_bn_train_fwd",
    "nconv_bn_train_bwd",
    "nconv_relu_bias_bwd_workspace_bytes",
    "nconv_relu_bias_bwd",
    "nconv_depth_loss_workspace_bytes",
    "nconv_depth_loss_fwd",
    "nconv_depth_loss_bwd",
    "nconv_conf_loss_workspace_bytes",
    "nconv_conf_loss_fwd",
    "nconv_conf_loss_bwd",
    "nconv_depth_metrics_workspace_bytes",
    "nconv_depth_metrics",
    "nconv_frame_ingest",
    "nconv_depth_export_u16",
    "nconv_backproject_map",
    "nconv_backproject_workspace_bytes",
    "nconv_backproject_points",
    "nconv_lidar_project_workspace_bytes",
    "nconv_lidar_project",
    "nconv_depth_colorize_workspace_bytes",
    "nconv_depth_colorize",
    "nconv_depth_normals",
    "nconv_depth_normals_points",
    "nconv_depth_sparsify_workspace_bytes",
    "nconv_depth_sparsify",
    "nconv_depth_occlusion",
    "nconv_frame_augment",
    "nconv_depth_sparsification_workspace_bytes",
    "nconv_depth_sparsification",
    "nconv_depth_ipbasic",
    "nconv_depth_nearest",
    "nconv_view_warp_fwd",
    "nconv_view_warp_bwd",
    "nconv_photo_loss_workspace_bytes",
    "nconv_photo_loss_fwd",
    "nconv_photo_loss_bwd",
    "nconv_photo_ssim_workspace_bytes",
    "nconv_photo_ssim_loss_fwd",
    "nconv_photo_ssim_loss_bwd",
    "nconv_photo_min_workspace_bytes",
    "nconv_photo_min_loss_fwd",
    "nconv_photo_min_loss_bwd",
    "nconv_pose_workspace_bytes",
    "nconv_pose_normal_eq",
    "nconv_pose_update",
    "nconv_smooth_loss_workspace_bytes",
    "nconv_smooth_loss_fwd",
    "nconv_smooth_loss_bwd",
    "nconv_edge_weights",
    "nconv_depth_consistency",
    "nconv_geo_consistency_workspace_bytes",
    "nconv_geo_consistency_loss_fwd",
    "nconv_geo_consistency_loss_bwd",
    "nconv_voxel_merge_workspace_bytes",
    "nconv_voxel_merge",
)


class NconvSrc(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("c", ctypes.c_void_p), ("C", ctypes.c_int),
                ("H", ctypes.c_int), ("W", ctypes.c_int)]


class NconvLayer(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("Cin", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("Cout", ctypes.c_int), ("Ho", ctypes.c_int), ("Wo", ctypes.c_int),
                ("KH", ctypes.c_int), ("KW", ctypes.c_int), ("SH", ctypes.c_int), ("SW", ctypes.c_int),
                ("PH", ctypes.c_int), ("PW", ctypes.c_int), ("DH", ctypes.c_int), ("DW", ctypes.c_int),
                ("groups", ctypes.c_int), ("eps", ctypes.c_float), ("load_mode", ctypes.c_int),
                ("thresh", ctypes.c_float), ("a", NconvSrc), ("b", NconvSrc),
                ("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("wsum", ctypes.c_void_p),
                ("math", ctypes.c_int), ("bwd_math", ctypes.c_int), ("waux", ctypes.c_void_p)]


class NconvBwdIo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("y", "cout", "gy", "gcout", "gxa", "gca", "gxb", "gcb", "gw",
                                               "gbias", "gy_pool", "gcout_pool", "pool_argmax")] + [
        ("head", ctypes.POINTER(NconvLayer)), ("head_workspace", ctypes.c_void_p),
        ("head_workspace_bytes", ctypes.c_size_t), ("head_gw", ctypes.c_void_p), ("head_gbias", ctypes.c_void_p),
        ("head_nparts", ctypes.c_int), ("tail", ctypes.POINTER(NconvLayer)), ("tail_y", ctypes.c_void_p),
        ("tail_cout", ctypes.c_void_p), ("tail_gy", ctypes.c_void_p), ("tail_workspace", ctypes.c_void_p),
        ("tail_workspace_bytes", ctypes.c_size_t), ("tail_gw", ctypes.c_void_p), ("tail_nparts", ctypes.c_int),
        ("box_weights", ctypes.c_void_p), ("tail_crop0", ctypes.c_int), ("tail_h", ctypes.c_int),
        ("tail_w", ctypes.c_int)]


class NconvDenseConv(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("x0", ctypes.c_void_p), ("C0", ctypes.c_int),
                ("x1", ctypes.c_void_p), ("C1", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("Cout", ctypes.c_int), ("Ho", ctypes.c_int), ("Wo", ctypes.c_int),
                ("kind", ctypes.c_int), ("stride", ctypes.c_int), ("wpack", ctypes.c_void_p),
                ("bias", ctypes.c_void_p), ("relu", ctypes.c_int), ("wshort", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("out_C", ctypes.c_int), ("out_c0", ctypes.c_int),
                ("math", ctypes.c_int)]


class NconvDenseWgrad(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("kind", ctypes.c_int), ("stride", ctypes.c_int),
                ("x0", ctypes.c_void_p), ("C0", ctypes.c_int), ("x1", ctypes.c_void_p), ("C1", ctypes.c_int),
                ("H", ctypes.c_int), ("W", ctypes.c_int), ("gy", ctypes.c_void_p), ("Cout", ctypes.c_int),
                ("Ho", ctypes.c_int), ("Wo", ctypes.c_int), ("gw", ctypes.c_void_p), ("math", ctypes.c_int)]


class NconvBnTrain(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("x", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("running_mean", ctypes.c_void_p), ("running_var", ctypes.c_void_p),
                ("momentum", ctypes.c_float), ("eps", ctypes.c_float), ("relu", ctypes.c_int),
                ("y", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("invstd", ctypes.c_void_p)]


class NconvFramePlane(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("image_stride", ctypes.c_longlong), ("row_stride", ctypes.c_longlong),
                ("dtype", ctypes.c_int), ("shift", ctypes.c_int), ("scale", ctypes.c_float),
                ("out", ctypes.c_void_p)]


class NconvFrameIngest(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("reverse", ctypes.c_int),
                ("rgb", ctypes.c_void_p), ("rgb_image_stride", ctypes.c_longlong),
                ("rgb_row_stride", ctypes.c_longlong), ("rgb_out", ctypes.c_void_p),
                ("plane", NconvFramePlane * 2)]


class NconvBackproject(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("color_kind", ctypes.c_int),
                ("depth", ctypes.c_void_p), ("depth_image_stride", ctypes.c_longlong),
                ("depth_row_stride", ctypes.c_longlong), ("conf", ctypes.c_void_p),
                ("conf_image_stride", ctypes.c_longlong), ("conf_row_stride", ctypes.c_longlong),
                ("color", ctypes.c_void_p), ("color_image_stride", ctypes.c_longlong),
                ("color_channel_stride", ctypes.c_longlong), ("color_row_stride", ctypes.c_longlong),
                ("reverse", ctypes.c_int), ("z_min", ctypes.c_float), ("z_max", ctypes.c_float),
                ("conf_min", ctypes.c_float), ("k", ctypes.c_void_p), ("k_image_stride", ctypes.c_longlong)]


class NconvLidarProject(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("point_stride", ctypes.c_int),
                ("points", ctypes.c_void_p), ("n_rows", ctypes.c_longlong), ("offsets", ctypes.c_void_p),
                ("m", ctypes.c_void_p), ("m_image_stride", ctypes.c_longlong), ("z_min", ctypes.c_float),
                ("z_max", ctypes.c_float)]


class NconvSmoothLoss(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("order", ctypes.c_int),
                ("depth", ctypes.c_void_p), ("depth_image_stride", ctypes.c_longlong),
                ("depth_row_stride", ctypes.c_longlong), ("mask", ctypes.c_void_p),
                ("mask_image_stride", ctypes.c_longlong), ("mask_row_stride", ctypes.c_longlong),
                ("weights", ctypes.c_void_p)]


class NconvEdgeWeights(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("image", ctypes.c_void_p), ("image_stride", ctypes.c_longlong),
                ("channel_stride", ctypes.c_longlong), ("row_stride", ctypes.c_longlong), ("alpha", ctypes.c_float)]


class NconvDepthColorize(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("radius", ctypes.c_int),
                ("depth", ctypes.c_void_p), ("image_stride", ctypes.c_longlong), ("row_stride", ctypes.c_longlong),
                ("lut", ctypes.c_void_p), ("cmap_id", ctypes.c_int), ("auto_range", ctypes.c_int),
                ("vmin", ctypes.c_float), ("vmax", ctypes.c_float), ("floor", ctypes.c_float), ("bgr", ctypes.c_int),
                ("background", ctypes.c_void_p), ("background_image_stride", ctypes.c_longlong),
                ("background_row_stride", ctypes.c_longlong), ("empty_rgb", ctypes.c_ubyte * 3)]


class NconvNormalsOpts(ctypes.Structure):
    _fields_ = [("jump_rel", ctypes.c_float), ("jump_abs", ctypes.c_float), ("empty_rgb", ctypes.c_ubyte * 3)]


class NconvDepthSparsify(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("mode", ctypes.c_int),
                ("src", ctypes.c_void_p), ("src_image_stride", ctypes.c_longlong),
                ("src_row_stride", ctypes.c_longlong), ("mask", ctypes.c_void_p),
                ("mask_image_stride", ctypes.c_longlong), ("mask_row_stride", ctypes.c_longlong),
                ("state", ctypes.c_void_p), ("n_dev", ctypes.c_void_p), ("n", ctypes.c_int),
                ("keep", ctypes.c_float), ("all_pixels", ctypes.c_int), ("floor", ctypes.c_float),
                ("key_mask", ctypes.c_uint), ("noise_threshold", ctypes.c_uint), ("noise_amp", ctypes.c_float)]


class NconvDepthOcclusion(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("rh", ctypes.c_int),
                ("rw", ctypes.c_int), ("min_support", ctypes.c_int), ("src", ctypes.c_void_p),
                ("src_image_stride", ctypes.c_longlong), ("src_row_stride", ctypes.c_longlong),
                ("jump_abs", ctypes.c_float), ("jump_rel", ctypes.c_float), ("floor", ctypes.c_float)]


class NconvAugmentPlane(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("image_stride", ctypes.c_longlong), ("row_stride", ctypes.c_longlong),
                ("out", ctypes.c_void_p)]


class NconvFrameAugment(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("h", ctypes.c_int),
                ("w", ctypes.c_int), ("mode_y", ctypes.c_int), ("mode_x", ctypes.c_int),
                ("flip_threshold", ctypes.c_ulonglong), ("state", ctypes.c_void_p), ("rgb", ctypes.c_void_p),
                ("rgb_image_stride", ctypes.c_longlong), ("rgb_channel_stride", ctypes.c_longlong),
                ("rgb_row_stride", ctypes.c_longlong), ("rgb_out", ctypes.c_void_p),
                ("plane", NconvAugmentPlane * 3), ("mask", ctypes.c_void_p),
                ("mask_image_stride", ctypes.c_longlong), ("mask_row_stride", ctypes.c_longlong),
                ("mask_out", ctypes.c_void_p), ("k", ctypes.c_void_p), ("k_out", ctypes.c_void_p),
                ("params", ctypes.c_void_p), ("gains", ctypes.c_void_p), ("brightness", ctypes.c_float),
                ("contrast", ctypes.c_float), ("color", ctypes.c_float), ("pivot", ctypes.c_float),
                ("rgb_max", ctypes.c_float)]


class NconvDepthSparsification(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("steps", ctypes.c_int),
                ("pred", ctypes.c_void_p), ("pred_image_stride", ctypes.c_longlong),
                ("pred_row_stride", ctypes.c_longlong), ("gt", ctypes.c_void_p),
                ("gt_image_stride", ctypes.c_longlong), ("gt_row_stride", ctypes.c_longlong),
                ("conf", ctypes.c_void_p), ("conf_image_stride", ctypes.c_longlong),
                ("conf_row_stride", ctypes.c_longlong), ("gt_min", ctypes.c_float), ("gt_max", ctypes.c_float),
                ("clamp_lo", ctypes.c_float), ("clamp_hi", ctypes.c_float), ("uncertainty", ctypes.c_int),
                ("curves", ctypes.c_void_p), ("order", ctypes.c_void_p)]


class NconvDepthIpbasic(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("src", ctypes.c_void_p),
                ("src_image_stride", ctypes.c_longlong), ("src_row_stride", ctypes.c_longlong),
                ("max_depth", ctypes.c_float), ("kernel_shape", ctypes.c_int), ("kernel_size", ctypes.c_int),
                ("extrapolate", ctypes.c_int), ("median", ctypes.c_int), ("blur", ctypes.c_int),
                ("keep_samples", ctypes.c_int)]


class NconvDepthNearest(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("src", ctypes.c_void_p),
                ("src_image_stride", ctypes.c_longlong), ("src_row_stride", ctypes.c_longlong),
                ("floor", ctypes.c_float), ("max_dist2", ctypes.c_int)]


class NconvViewWarp(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("Hs", ctypes.c_int), ("Ws", ctypes.c_int), ("depth", ctypes.c_void_p),
                ("depth_image_stride", ctypes.c_longlong), ("depth_row_stride", ctypes.c_longlong),
                ("mask", ctypes.c_void_p), ("mask_image_stride", ctypes.c_longlong),
                ("mask_row_stride", ctypes.c_longlong), ("src", ctypes.c_void_p),
                ("src_image_stride", ctypes.c_longlong), ("src_channel_stride", ctypes.c_longlong),
                ("src_row_stride", ctypes.c_longlong), ("k", ctypes.c_void_p), ("k_image_stride", ctypes.c_longlong),
                ("m", ctypes.c_void_p), ("m_image_stride", ctypes.c_longlong), ("z_min", ctypes.c_float),
                ("z_max", ctypes.c_float)]


class NconvConsistencySource(ctypes.Structure):
    _fields_ = [("k_src", ctypes.c_void_p), ("k_src_image_stride", ctypes.c_longlong),
                ("m_back", ctypes.c_void_p), ("m_back_image_stride", ctypes.c_longlong)]


class NconvPoseAlign(ctypes.Structure):
    _fields_ = NconvViewWarp._fields_ + [
        ("tgt", ctypes.c_void_p), ("tgt_image_stride", ctypes.c_longlong), ("tgt_channel_stride", ctypes.c_longlong),
        ("tgt_row_stride", ctypes.c_longlong), ("k_src", ctypes.c_void_p), ("k_src_image_stride", ctypes.c_longlong),
        ("pose", ctypes.c_void_p), ("status", ctypes.c_void_p), ("cost", ctypes.c_void_p), ("n_hist", ctypes.c_void_p),
        ("history", ctypes.c_int), ("huber", ctypes.c_float), ("damping", ctypes.c_float),
        ("min_points", ctypes.c_int)]


class NconvVoxelMerge(ctypes.Structure):
    _fields_ = [("n_points", ctypes.c_longlong), ("xyz", ctypes.c_void_p), ("xyz_row_stride", ctypes.c_longlong),
                ("rgb", ctypes.c_void_p), ("rgb_row_stride", ctypes.c_longlong), ("normals", ctypes.c_void_p),
                ("normals_row_stride", ctypes.c_longlong), ("weights", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("poses", ctypes.c_void_p), ("n_segments", ctypes.c_int), ("nx", ctypes.c_int), ("ny", ctypes.c_int),
                ("nz", ctypes.c_int), ("voxel", ctypes.c_float), ("origin", ctypes.c_float * 3),
                ("max_voxels", ctypes.c_longlong), ("out_xyz", ctypes.c_void_p), ("out_rgb", ctypes.c_void_p),
                ("out_normals", ctypes.c_void_p), ("out_count", ctypes.c_void_p), ("out_key", ctypes.c_void_p),
                ("stats", ctypes.c_void_p)]


_lib = None
_lock = threading.Lock()


def _declare(lib):
    P = ctypes.c_void_p
    lib.nconv_abi_version.restype = ctypes.c_int
    lib.nconv_abi_version.argtypes = []
    lib.nconv_last_error.restype = ctypes.c_char_p
    lib.nconv_last_error.argtypes = []
    lib.nconv_weight_prep.restype = ctypes.c_int
    lib.nconv_weight_prep.argtypes = [ctypes.c_int, P, P, P, P, P, P]
    lib.nconv_fwd.restype = ctypes.c_int
    lib.nconv_fwd.argtypes = [ctypes.POINTER(NconvLayer), P, P, P]
    lib.nconv_fwd_pooled.restype = ctypes.c_int
    lib.nconv_fwd_pooled.argtypes = [ctypes.POINTER(NconvLayer), P, P, P, P, P, P]
    lib.nconv_fwd_head.restype = ctypes.c_int
    lib.nconv_fwd_head.argtypes = [ctypes.POINTER(NconvLayer), ctypes.POINTER(NconvLayer), P, P, P, P, P, P, P, P]
    lib.nconv_head_weights.restype = ctypes.c_int
    lib.nconv_head_weights.argtypes = [ctypes.POINTER(NconvLayer), ctypes.POINTER(NconvLayer), P, P]
    lib.nconv_fwd_tail.restype = ctypes.c_int
    lib.nconv_fwd_tail.argtypes = [ctypes.POINTER(NconvLayer), P, P, P, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_float, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P]
    lib.nconv_plan.restype = ctypes.c_int
    lib.nconv_plan.argtypes = [ctypes.POINTER(NconvLayer), P, P, P]
    lib.nconv_phase_weights_floats.restype = ctypes.c_size_t
    lib.nconv_phase_weights_floats.argtypes = [ctypes.POINTER(NconvLayer)]
    lib.nconv_phase_weights.restype = ctypes.c_int
    lib.nconv_phase_weights.argtypes = [ctypes.c_int, P, P, P, P, P]
    lib.nconv_weight_prologue.restype = ctypes.c_int
    lib.nconv_weight_prologue.argtypes = [ctypes.c_int, P, P, P, P, P, P, P, ctypes.c_int, P, P, P, P, P]
    lib.nconv_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_bwd_workspace_bytes.argtypes = [ctypes.POINTER(NconvLayer)]
    lib.nconv_bwd.restype = ctypes.c_int
    lib.nconv_bwd.argtypes = [ctypes.POINTER(NconvLayer), P, P, P, P, P, P, P, P, P, P, P,
                              ctypes.c_size_t, ctypes.c_uint, P]
    lib.nconv_bwd_ex.restype = ctypes.c_int
    lib.nconv_bwd_ex.argtypes = [ctypes.POINTER(NconvLayer), ctypes.POINTER(NconvBwdIo), P, ctypes.c_size_t,
                                 ctypes.c_uint, P]
    lib.nconv_bwd_head_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_bwd_head_workspace_bytes.argtypes = [ctypes.POINTER(NconvLayer)]
    lib.nconv_bwd_tail_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_bwd_tail_workspace_bytes.argtypes = [ctypes.POINTER(NconvLayer)]
    lib.nconv_bwd_tail_conf.restype = ctypes.c_int
    lib.nconv_bwd_tail_conf.argtypes = [ctypes.POINTER(NconvLayer), ctypes.POINTER(NconvBwdIo), P, P, ctypes.c_size_t,
                                        ctypes.c_uint, P]
    lib.nconv_wgrad_reduce.restype = ctypes.c_int
    lib.nconv_wgrad_reduce.argtypes = [ctypes.c_int, ctypes.POINTER(NconvLayer), P, P, P, P, P]
    lib.nconv_wgrad_reduce_ex.restype = ctypes.c_int
    lib.nconv_wgrad_reduce_ex.argtypes = [ctypes.c_int, ctypes.POINTER(NconvLayer), P, P, P, P, ctypes.c_int, P, P,
                                          P, P, ctypes.c_size_t, P]
    lib.nconv_sum_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_sum_workspace_bytes.argtypes = [ctypes.c_int]
    lib.nconv_train_prologue.restype = ctypes.c_int
    lib.nconv_train_prologue.argtypes = [ctypes.c_int, P, P, P, P, P, ctypes.c_int, ctypes.c_int, P, P,
                                         ctypes.c_int, P, P, P, P, P]
    I = ctypes.c_int
    lib.nconv_dense_packed_floats.restype = ctypes.c_size_t
    lib.nconv_dense_packed_floats.argtypes = [I, I, I]
    lib.nconv_dense_pack.restype = I
    lib.nconv_dense_pack.argtypes = [I, I, I, P, P, P, P]
    lib.nconv_dense_conv_fwd.restype = I
    lib.nconv_dense_conv_fwd.argtypes = [ctypes.POINTER(NconvDenseConv), P]
    lib.nconv_conv3x3_c1.restype = I
    lib.nconv_conv3x3_c1.argtypes = [P, I, I, I, I, P, P, P, P]
    lib.nconv_bilinear_ac.restype = I
    lib.nconv_bilinear_ac.argtypes = [P, I, I, I, I, P, I, I, P]
    lib.nconv_dense_wgrad_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_dense_wgrad_workspace_bytes.argtypes = [ctypes.POINTER(NconvDenseWgrad)]
    lib.nconv_dense_conv_wgrad.restype = I
    lib.nconv_dense_conv_wgrad.argtypes = [ctypes.POINTER(NconvDenseWgrad), P, ctypes.c_size_t, P]
    lib.nconv_bn_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_bn_workspace_bytes.argtypes = [ctypes.POINTER(NconvBnTrain)]
    lib.nconv_bn_train_fwd.restype = I
    lib.nconv_bn_train_fwd.argtypes = [ctypes.POINTER(NconvBnTrain), P, ctypes.c_size_t, P]
    lib.nconv_bn_train_bwd.restype = I
    lib.nconv_bn_train_bwd.argtypes = [ctypes.POINTER(NconvBnTrain), P, P, P, P, P, ctypes.c_size_t, P]
    lib.nconv_relu_bias_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_relu_bias_bwd_workspace_bytes.argtypes = [I, I, I, I]
    lib.nconv_relu_bias_bwd.restype = I
    lib.nconv_relu_bias_bwd.argtypes = [I, I, I, I, P, P, P, P, P, ctypes.c_size_t, P]
    L = ctypes.c_longlong
    lib.nconv_depth_loss_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_depth_loss_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_depth_loss_fwd.restype = I
    lib.nconv_depth_loss_fwd.argtypes = [P, L, L, P, L, L, I, I, I, I, P, P, ctypes.c_size_t, P]
    lib.nconv_depth_loss_bwd.restype = I
    lib.nconv_depth_loss_bwd.argtypes = [P, L, L, P, L, L, I, I, I, I, P, P, ctypes.c_size_t, P, P]
    F = ctypes.c_float
    lib.nconv_conf_loss_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_conf_loss_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_conf_loss_fwd.restype = I
    lib.nconv_conf_loss_fwd.argtypes = [P, L, L, P, L, L, P, L, L, I, I, I, I, F, P, P, P, ctypes.c_size_t, P]
    lib.nconv_conf_loss_bwd.restype = I
    lib.nconv_conf_loss_bwd.argtypes = [P, L, L, P, L, L, P, L, L, I, I, I, I, F, P, P, P, P, P]
    lib.nconv_depth_metrics_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_depth_metrics_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_depth_metrics.restype = I
    lib.nconv_depth_metrics.argtypes = [P, L, L, P, L, L, I, I, I, F, F, F, F, P, P, P, ctypes.c_size_t, P]
    lib.nconv_frame_ingest.restype = I
    lib.nconv_frame_ingest.argtypes = [ctypes.POINTER(NconvFrameIngest), P]
    lib.nconv_depth_export_u16.restype = I
    lib.nconv_depth_export_u16.argtypes = [P, L, L, I, I, I, F, P, P]
    lib.nconv_backproject_map.restype = I
    lib.nconv_backproject_map.argtypes = [ctypes.POINTER(NconvBackproject), P, P]
    lib.nconv_backproject_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_backproject_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_backproject_points.restype = I
    lib.nconv_backproject_points.argtypes = [ctypes.POINTER(NconvBackproject), P, P, P, L, P, P, ctypes.c_size_t, P]
    lib.nconv_lidar_project_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_lidar_project_workspace_bytes.argtypes = [I, I, I, I]
    lib.nconv_lidar_project.restype = I
    lib.nconv_lidar_project.argtypes = [ctypes.POINTER(NconvLidarProject), P, P, P, ctypes.c_size_t, P]
    lib.nconv_depth_colorize_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_depth_colorize_workspace_bytes.argtypes = [I]
    lib.nconv_depth_colorize.restype = I
    lib.nconv_depth_colorize.argtypes = [ctypes.POINTER(NconvDepthColorize), P, P, ctypes.c_size_t, P]
    lib.nconv_depth_normals.restype = I
    lib.nconv_depth_normals.argtypes = [ctypes.POINTER(NconvBackproject), ctypes.POINTER(NconvNormalsOpts), P, P, P]
    lib.nconv_depth_normals_points.restype = I
    lib.nconv_depth_normals_points.argtypes = [ctypes.POINTER(NconvBackproject), ctypes.POINTER(NconvNormalsOpts),
                                               P, P, L, P, P]
    lib.nconv_depth_sparsify_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_depth_sparsify_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_depth_sparsify.restype = I
    lib.nconv_depth_sparsify.argtypes = [ctypes.POINTER(NconvDepthSparsify), P, L, L, P, P, ctypes.c_size_t, P]
    lib.nconv_depth_occlusion.restype = I
    lib.nconv_depth_occlusion.argtypes = [ctypes.POINTER(NconvDepthOcclusion), P, L, L, P, P, P, P]
    lib.nconv_frame_augment.restype = I
    lib.nconv_frame_augment.argtypes = [ctypes.POINTER(NconvFrameAugment), P]
    lib.nconv_depth_sparsification_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_depth_sparsification_workspace_bytes.argtypes = [I, I, I, I]
    lib.nconv_depth_sparsification.restype = I
    lib.nconv_depth_sparsification.argtypes = [ctypes.POINTER(NconvDepthSparsification), P, ctypes.c_size_t, P]
    lib.nconv_depth_ipbasic.restype = I
    lib.nconv_depth_ipbasic.argtypes = [ctypes.POINTER(NconvDepthIpbasic), P, L, L, P, P, P]
    lib.nconv_depth_nearest.restype = I
    lib.nconv_depth_nearest.argtypes = [ctypes.POINTER(NconvDepthNearest), P, L, L, P, P, P, P, P]
    lib.nconv_view_warp_fwd.restype = I
    lib.nconv_view_warp_fwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, P, P]
    lib.nconv_view_warp_bwd.restype = I
    lib.nconv_view_warp_bwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, P, P]
    lib.nconv_photo_loss_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_photo_loss_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_photo_loss_fwd.restype = I
    lib.nconv_photo_loss_fwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, L, L, L, P, P, ctypes.c_size_t, P]
    lib.nconv_photo_loss_bwd.restype = I
    lib.nconv_photo_loss_bwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, L, L, L, P, P, ctypes.c_size_t, P, P]
    lib.nconv_photo_ssim_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_photo_ssim_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_photo_ssim_loss_fwd.restype = I
    lib.nconv_photo_ssim_loss_fwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, L, L, L, F, F, F, P, P, ctypes.c_size_t, P]
    lib.nconv_photo_ssim_loss_bwd.restype = I
    lib.nconv_photo_ssim_loss_bwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, L, L, L, F, F, F, P, P, ctypes.c_size_t,
                                              P, P]
    lib.nconv_photo_min_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_photo_min_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_photo_min_loss_fwd.restype = I
    lib.nconv_photo_min_loss_fwd.argtypes = [ctypes.POINTER(NconvViewWarp), I, P, L, L, L, F, F, F, I, P, P, P, P,
                                             ctypes.c_size_t, P]
    lib.nconv_photo_min_loss_bwd.restype = I
    lib.nconv_photo_min_loss_bwd.argtypes = [ctypes.POINTER(NconvViewWarp), I, P, L, L, L, F, F, F, I, P, P,
                                             ctypes.c_size_t, P, P]
    lib.nconv_pose_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_pose_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_pose_normal_eq.restype = I
    lib.nconv_pose_normal_eq.argtypes = [ctypes.POINTER(NconvPoseAlign), P, ctypes.c_size_t, P]
    lib.nconv_pose_update.restype = I
    lib.nconv_pose_update.argtypes = [ctypes.POINTER(NconvPoseAlign), P, ctypes.c_size_t, I, I, P]
    lib.nconv_smooth_loss_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_smooth_loss_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_smooth_loss_fwd.restype = I
    lib.nconv_smooth_loss_fwd.argtypes = [ctypes.POINTER(NconvSmoothLoss), P, P, ctypes.c_size_t, P]
    lib.nconv_smooth_loss_bwd.restype = I
    lib.nconv_smooth_loss_bwd.argtypes = [ctypes.POINTER(NconvSmoothLoss), P, P, ctypes.c_size_t, P, P]
    lib.nconv_edge_weights.restype = I
    lib.nconv_edge_weights.argtypes = [ctypes.POINTER(NconvEdgeWeights), P, P]
    lib.nconv_depth_consistency.restype = I
    lib.nconv_depth_consistency.argtypes = [ctypes.POINTER(NconvViewWarp), ctypes.POINTER(NconvConsistencySource), I,
                                            F, F, I, P, P, P, P, P, P]
    lib.nconv_geo_consistency_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_geo_consistency_workspace_bytes.argtypes = [I, I, I]
    lib.nconv_geo_consistency_loss_fwd.restype = I
    lib.nconv_geo_consistency_loss_fwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, P, P, ctypes.c_size_t, P]
    lib.nconv_geo_consistency_loss_bwd.restype = I
    lib.nconv_geo_consistency_loss_bwd.argtypes = [ctypes.POINTER(NconvViewWarp), P, P, ctypes.c_size_t, P, P]
    lib.nconv_voxel_merge_workspace_bytes.restype = ctypes.c_size_t
    lib.nconv_voxel_merge_workspace_bytes.argtypes = [L, I, I, I]
    lib.nconv_voxel_merge.restype = I
    lib.nconv_voxel_merge.argtypes = [ctypes.POINTER(NconvVoxelMerge), P, ctypes.c_size_t, P]


def lib():
    """The loaded library. Raises RuntimeError if it is missing or incompatible."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"libnconv.so not found at {LIB_PATH}; build it with "
                    "`python -c 'import __graft_entry__ as g; g.build()'` (no fallback path exists)")
            handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
            _declare(handle)
            v = handle.nconv_abi_version()
            if v != ABI_VERSION:
                raise RuntimeError(f"libnconv ABI {v} != expected {ABI_VERSION}")
            _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().nconv_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def stream_handle(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def src(x, c):
    """NconvSrc for a (B, C, H, W) pair (c may be None)."""
    s = NconvSrc()
    if x is not None:
        s.x = x.data_ptr()
        s.c = c.data_ptr() if c is not None else None
        s.C, s.H, s.W = x.shape[1], x.shape[2], x.shape[3]
    return s
