"""The argument checks metrics, frames, pointcloud and lidar share (_views.py): one malformed input
of each kind through each module, and the exact text of the exception, which names the module the
caller used. CPU only: every check runs before the library is called."""
import re
import types

import pytest
import torch

NO_GPU = " on ROCm devices only (no PyTorch fallback), move the tensors to the GPU"
NOT_PLANES = " is not an (H, W), (1, H, W) or (B, 1, H, W) set of unit-stride rows"


def _raises(exc, text, fn, *args, **kw):
    with pytest.raises(exc, match="^" + re.escape(text) + "$"):
        fn(*args, **kw)


def test_metrics_messages(nconv_amd):
    M, V = nconv_amd.metrics, nconv_amd._views
    ok = torch.zeros(4, 6)
    _raises(TypeError, "depth metrics: pred must be a tensor, got list", M.depth_metric_sums, [1.0], ok)
    _raises(RuntimeError, "depth metrics: pred is on cpu; the sums are computed by libnconv" + NO_GPU,
            M.depth_metric_sums, ok, ok)
    _raises(RuntimeError, "depth metrics: pred is on cpu; the sums are computed by libnconv" + NO_GPU,
            M.DepthMetrics().update, ok, ok)
    # a tensor's device is checked first, so the two remaining kinds are reached on a device only
    _raises(TypeError, "depth metrics: gt: expected float32, got torch.float64", V.require_tensor, ok.double(), "gt",
            (torch.float32,), "depth metrics", expected="float32")
    _raises(ValueError, "depth metrics: gt of shape (2, 4, 6) / strides (24, 6, 1)" + NOT_PLANES, V.plane_view,
            torch.zeros(2, 4, 6), "gt", "depth metrics")


def test_frames_messages(nconv_amd):
    F = nconv_amd.frames
    _raises(TypeError, "frames: rgb must be a tensor, got list", F.ingest, rgb=[1])
    _raises(TypeError, "frames: rgb: expected torch.uint8, got torch.float32", F.ingest, rgb=torch.zeros(1, 2, 2, 3))
    _raises(TypeError, "frames: depth: expected torch.uint16 / torch.uint8 / torch.float32, got torch.int32", F.ingest,
            depth=torch.zeros(1, 2, 2, dtype=torch.int32))
    _raises(ValueError, "frames: rgb must be (B, h, w, 3), got (2, 3, 4)", F.ingest,
            rgb=torch.zeros(2, 3, 4, dtype=torch.uint8))
    _raises(ValueError, "frames: rgb of strides (48, 24, 6, 1) is not interleaved (unit innermost stride, pixel "
            "stride 3)", F.ingest, rgb=torch.zeros(1, 2, 4, 6, dtype=torch.uint8)[..., :3])
    _raises(ValueError, "frames: gt must be (B, h, w) or (B, 1, h, w), got (2, 2)", F.ingest, gt=torch.zeros(2, 2))
    _raises(RuntimeError, "frames: rgb is on cpu; frames are converted by libnconv" + NO_GPU, F.ingest,
            rgb=torch.zeros(1, 2, 2, 3, dtype=torch.uint8))
    _raises(TypeError, "frames: pred must be a tensor, got NoneType", F.export_depth16, None)
    _raises(TypeError, "frames: pred: expected torch.float32, got torch.float16", F.export_depth16,
            torch.zeros(4, 6).half())
    _raises(ValueError, "frames: pred of shape (2, 4, 6) / strides (24, 6, 1)" + NOT_PLANES, F.export_depth16,
            torch.zeros(2, 4, 6))
    _raises(RuntimeError, "frames: pred is on cpu; frames are converted by libnconv" + NO_GPU, F.export_depth16,
            torch.zeros(4, 6))
    cpu = torch.device("cpu")
    _raises(TypeError, "frames: out['rgb'] must be a contiguous torch.float32 tensor of shape (1, 3, 2, 2)", F._output,
            {"rgb": torch.zeros(1, 3, 2, 3)}, "rgb", (1, 3, 2, 2), torch.float32, cpu)
    _raises(RuntimeError, "frames: out['rgb'] on cpu, the source on cuda:0", F._output, {"rgb": torch.zeros(1, 3, 2, 2)},
            "rgb", (1, 3, 2, 2), torch.float32, torch.device("cuda:0"))
    assert F._output({"gt": None}, "gt", (1, 1, 2, 2), torch.float32, cpu).shape == (1, 1, 2, 2)


def test_pointcloud_messages(nconv_amd):
    P = nconv_amd.pointcloud
    k = torch.eye(3)
    _raises(TypeError, "pointcloud: depth must be a tensor, got tuple", P.backproject_map, (1.0,), k)
    _raises(TypeError, "pointcloud: depth: expected torch.float32, got torch.float64", P.backproject, torch.zeros(4, 6).double(), k)
    _raises(TypeError, "pointcloud: k: expected torch.float32, got torch.int64", P.backproject_map, torch.zeros(4, 6),
            torch.eye(3, dtype=torch.int64))
    _raises(ValueError, "pointcloud: depth of shape (2, 4, 6) / strides (24, 6, 1)" + NOT_PLANES, P.backproject_map,
            torch.zeros(2, 4, 6), k)
    _raises(RuntimeError, "pointcloud: depth is on cpu; points are computed by libnconv" + NO_GPU, P.backproject,
            torch.zeros(4, 6), k)
    # the colour is looked at after the depth, which has to be on a device: its checks directly
    d, cpu = types.SimpleNamespace(), torch.device("cpu")
    _raises(TypeError, "pointcloud: color must be a tensor, got str", P._color, d, "red", False, (1, 4, 6), cpu)
    _raises(ValueError, "pointcloud: uint8 color must be (1, 4, 6, 3) interleaved, got (1, 4, 5, 3)", P._color, d,
            torch.zeros(4, 5, 3, dtype=torch.uint8), False, (1, 4, 6), cpu)
    _raises(ValueError, "pointcloud: color of strides (96, 24, 4, 1) is not interleaved (unit innermost stride, pixel "
            "stride 3)", P._color, d, torch.zeros(1, 4, 6, 4, dtype=torch.uint8)[..., :3], False, (1, 4, 6), cpu)
    _raises(RuntimeError, "pointcloud: color is on cpu; points are computed by libnconv" + NO_GPU, P._color, d,
            torch.zeros(1, 4, 6, 3, dtype=torch.uint8), False, (1, 4, 6), cpu)
    assert (d.color_image_stride, d.color_row_stride) == (72, 18)
    _raises(TypeError, "pointcloud: out['xyz'] must be a contiguous torch.float32 tensor of shape (5, 3)", P._output,
            {"xyz": torch.zeros(5, 3, dtype=torch.float64)}, "xyz", (5, 3), torch.float32, cpu)
    _raises(RuntimeError, "pointcloud: out['xyz'] on cpu, the source on cuda:0", P._output, {"xyz": torch.zeros(5, 3)},
            "xyz", (5, 3), torch.float32, torch.device("cuda:0"))


def test_lidar_messages(nconv_amd):
    L = nconv_amd.lidar
    pts, m = torch.zeros(5, 4), torch.zeros(3, 4)
    _raises(TypeError, "lidar: points must be a tensor, got list", L.project_points, [[0.0] * 3], None, m, (4, 6))
    _raises(TypeError, "lidar: points: expected torch.float32, got torch.float64", L.project_points, pts.double(), None,
            m, (4, 6))
    _raises(TypeError, "lidar: offsets: expected torch.int32, got torch.int64", L.project_points, pts,
            torch.tensor([0, 5]), m, (4, 6))
    _raises(TypeError, "lidar: m must be a tensor, got NoneType", L.project_points, pts, None, None, (4, 6))
    _raises(TypeError, "lidar: m: expected torch.float32, got torch.float16", L.project_points, pts, None, m.half(),
            (4, 6))
    _raises(RuntimeError, "lidar: points is on cpu; scans are projected by libnconv" + NO_GPU, L.project_points, pts,
            None, m, (4, 6))
    cpu = torch.device("cpu")
    _raises(TypeError, "lidar: out['depth'] must be a contiguous torch.float32 tensor of shape (1, 1, 4, 6)", L._output,
            {"depth": torch.zeros(1, 4, 6)}, "depth", (1, 1, 4, 6), torch.float32, cpu)
    _raises(RuntimeError, "lidar: out['depth'] on cpu, the points on cuda:0", L._output,
            {"depth": torch.zeros(1, 1, 4, 6)}, "depth", (1, 1, 4, 6), torch.float32, torch.device("cuda:0"))
