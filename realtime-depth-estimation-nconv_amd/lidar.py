"""A LiDAR scan and a 3 x 4 projection to the sparse depth plane S the models take, on the device.

A live sensor delivers an unordered list of (x, y, z, intensity) points in the LiDAR frame and two
calibration files, not the velodyne_raw PNG the loaders of data.py read. This is the missing first
stage, the inverse of pointcloud.backproject under the same convention (pixel centres at integer
coordinates, one fp32 rounding per operation):

  project_points      points (N, C >= 3), offsets (B + 1), m (3, 4) or (B, 3, 4) -> depth (B, 1, H, W),
                      optionally the winning row of every pixel; three libnconv launches and no host
                      synchronisation (nconv_lidar_project, csrc/lidar_project.hip)
  LidarProjector      the same with its outputs and workspace kept between calls (hipGraph capture)
  kitti_projection    KITTI's calib_cam_to_cam.txt and calib_velo_to_cam.txt -> the 3 x 4 matrix, with
                      the loaders' crop folded in
  projection_from_k   [K | 0]: project_points(pc.xyz, pc.offsets, projection_from_k(k), (H, W))
                      inverts backproject
  read_velodyne_bin   a KITTI .bin scan as an (N, 4) float32 array

Per point p = (x, y, z) and row r of m: dot(r, p) = ((r0 x + r1 y) + r2 z) + r3; a, b, c the three
dots; u = a / c, v = b / c; the pixel is (rint(v), rint(u)), ties to even. The point is valid iff
c > z_min, c <= z_max and the pixel is inside the plane; a pixel keeps the smallest c of its valid
points (0 where there is none) and, among bit-equal c, the smallest row number: the result is the
same on every run. Device tensors only: there is no PyTorch path.
"""
import ctypes

import numpy as np
import torch

from . import _views
from .data import read_calib_file

FLT_MAX = float(np.finfo(np.float32).max)


def _on_device(x, what):
    _views.on_device(x, what, "lidar", "scans are projected by libnconv")


def _output(out, key, shape, dtype, device):
    return _views.output(out, key, shape, dtype, device, "lidar", source="points")


def _size(size):
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise TypeError(f"lidar: size must be (H, W), got {size!r}") from None
    if H <= 0 or W <= 0:
        raise ValueError(f"lidar: size (H, W) = {(H, W)} is not positive")
    return H, W


def workspace_bytes(B, H, W, with_index=True):
    """Bytes of project_points' workspace (nconv_lidar_project_workspace_bytes): 8 per pixel with the
    index, none without."""
    from . import _lib
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 2 ** 31:
        raise ValueError(f"lidar: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31)")
    return _lib.lib().nconv_lidar_project_workspace_bytes(B, H, W, int(bool(with_index)))


def project_points(points, offsets, m, size, *, z_min=0.0, z_max=FLT_MAX, return_index=False, out=None):
    """The sparse depth plane (B, 1, H, W) fp32 of a scan, or (depth, index) with return_index:
    index (B, H, W) int32 is the row of `points` that won the pixel, -1 where the pixel is empty.
    points: (N, C >= 3) fp32 on the device, unit inner stride, any row stride >= 3 (a KITTI scan has
    C = 4, PointCloud.xyz 3); only x, y, z are read. offsets: (B + 1) int32 on the device, image b owns
    rows [offsets[b], offsets[b + 1]) (PointCloud.offsets), or a Python list (uploaded from pinned
    memory, no synchronisation), or None: one image holding all rows. m: (3, 4) or (B, 3, 4) fp32 on
    the device. size: (H, W). out: an optional dict of preallocated contiguous buffers 'depth', 'index',
    'workspace' (uint8, workspace_bytes(B, H, W)). Three launches, no allocation when out is complete
    and offsets is a tensor, no host synchronisation."""
    from . import _lib
    _views.require_tensor(points, "points", (torch.float32,), "lidar")
    if points.dim() != 2 or points.shape[1] < 3:
        raise ValueError(f"lidar: points must be (N, C >= 3), got {tuple(points.shape)}")
    N, C = points.shape
    if N > 0 and points.stride(1) != 1:
        raise ValueError(f"lidar: points of strides {points.stride()} has no unit inner stride")
    stride = points.stride(0) if N > 1 else C
    if stride < 3:
        raise ValueError(f"lidar: points of strides {points.stride()}: rows overlap (row stride below 3)")
    H, W = _size(size)
    if offsets is None:
        offsets = [0, N]
    if torch.is_tensor(offsets):
        _views.require_tensor(offsets, "offsets", (torch.int32,), "lidar")
        if offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
            raise ValueError(f"lidar: offsets must be a contiguous (B + 1) vector, got {tuple(offsets.shape)}")
        B = offsets.numel() - 1
    else:
        host = [int(v) for v in offsets]
        if len(host) < 2:
            raise ValueError(f"lidar: offsets must have B + 1 >= 2 entries, got {len(host)}")
        if any(b < a for a, b in zip(host, host[1:])) or host[0] < 0 or host[-1] > N:
            raise ValueError(f"lidar: offsets {host} must be non-decreasing inside [0, {N}]")
        B = len(host) - 1
    _views.require_tensor(m, "m", (torch.float32,), "lidar")
    if tuple(m.shape) not in ((3, 4), (B, 3, 4)):
        raise ValueError(f"lidar: m must be (3, 4) or ({B}, 3, 4), got {tuple(m.shape)}")
    if not m.is_contiguous():
        raise ValueError(f"lidar: m of strides {m.stride()} is not contiguous")
    z_min, z_max = float(z_min), float(z_max)
    if not z_min >= 0.0:
        raise ValueError(f"lidar: z_min = {z_min} is negative (a valid depth is positive)")
    if not z_max >= z_min or z_max == 0.0:
        raise ValueError(f"lidar: z_max = {z_max} < z_min = {z_min}, or both 0 (selects no point)")
    _on_device(points, "points")
    _on_device(m, "m")
    dev = points.device
    if m.device != dev:
        raise RuntimeError(f"lidar: m on {m.device}, points on {dev}")
    if torch.is_tensor(offsets):
        _on_device(offsets, "offsets")
        if offsets.device != dev:
            raise RuntimeError(f"lidar: offsets on {offsets.device}, points on {dev}")
    else:
        offsets = torch.tensor(host, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    depth = _output(out, "depth", (B, 1, H, W), torch.float32, dev)
    index = ws = None
    nws = 0
    if return_index:
        index = _output(out, "index", (B, H, W), torch.int32, dev)
        nws = workspace_bytes(B, H, W)
        ws = _output(out, "workspace", (nws,), torch.uint8, dev)
    d = _lib.NconvLidarProject()
    d.B, d.H, d.W, d.point_stride = B, H, W, stride
    d.points, d.n_rows = (points.data_ptr() if N else None), N
    d.offsets, d.m, d.m_image_stride = offsets.data_ptr(), m.data_ptr(), (12 if m.dim() == 3 else 0)
    d.z_min, d.z_max = z_min, z_max
    rc = _lib.lib().nconv_lidar_project(ctypes.byref(d), _lib.ptr(depth), _lib.ptr(index), _lib.ptr(ws), nws,
                                        _lib.stream_handle(dev))
    _lib.check(rc, "nconv_lidar_project")
    return (depth, index) if return_index else depth


class LidarProjector:
    """project_points for a fixed image size with the outputs (and, with_index, the workspace) kept
    between calls: no allocation after the first call of a batch size, so a call can be captured with
    torch.cuda.graph (offsets must then be a device tensor) and replayed on points, offsets and m
    refilled in place. Returns depth, or (depth, index): the kept tensors, overwritten by the next call."""

    def __init__(self, size, with_index=False):
        self.size, self.with_index = _size(size), bool(with_index)
        self._key, self._out = None, None

    def __call__(self, points, offsets, m, *, z_min=0.0, z_max=FLT_MAX):
        if torch.is_tensor(points) and points.is_cuda:
            B = 1 if offsets is None else (offsets.numel() if torch.is_tensor(offsets) else len(offsets)) - 1
            key = (B, points.device)
            if key != self._key and B >= 1:
                H, W = self.size
                out = {"depth": torch.empty(B, 1, H, W, device=points.device)}
                if self.with_index:
                    out["index"] = torch.empty(B, H, W, dtype=torch.int32, device=points.device)
                    out["workspace"] = torch.empty(workspace_bytes(B, H, W), dtype=torch.uint8, device=points.device)
                self._key, self._out = key, out
        return project_points(points, offsets, m, self.size, z_min=z_min, z_max=z_max, return_index=self.with_index,
                              out=self._out)


def projection_from_k(k):
    """[K | 0]: the 3 x 4 projection of points already in the camera frame, for a (3, 3) or (B, 3, 3)
    `k` (a tensor, or an array: the result is of the same kind, on the same device)."""
    if torch.is_tensor(k):
        if k.dim() not in (2, 3) or tuple(k.shape[-2:]) != (3, 3):
            raise ValueError(f"lidar: k must be (3, 3) or (B, 3, 3), got {tuple(k.shape)}")
        return torch.cat((k, k.new_zeros(k.shape[:-1] + (1,))), dim=-1).contiguous()
    k = np.asarray(k)
    if k.ndim not in (2, 3) or k.shape[-2:] != (3, 3):
        raise ValueError(f"lidar: k must be (3, 3) or (B, 3, 3), got {k.shape}")
    return np.ascontiguousarray(np.concatenate((k, np.zeros(k.shape[:-1] + (1,), dtype=k.dtype)), axis=-1))


def kitti_projection(cam_to_cam, velo_to_cam, cam=2, crop_top=0, crop_left=0):
    """The (3, 4) float32 matrix that takes a velodyne point to the pixels of rectified camera `cam`:
    P_rect_0{cam} . [R_rect_00 | 0; 0 1] . [R | T; 0 1] from the two calibration files of a KITTI raw
    drive (data.read_calib_file), computed in float64. A crop whose first row / column is crop_top /
    crop_left (the loaders' bottom crop) subtracts crop_left * row 2 from row 0 and crop_top * row 2
    from row 1, so that pixel (0, 0) is the crop's corner. Host code (numpy)."""
    c2c, v2c = read_calib_file(cam_to_cam), read_calib_file(velo_to_cam)
    p = np.asarray(c2c[f"P_rect_0{int(cam)}"], dtype=np.float64).reshape(3, 4)
    rect, tr = np.eye(4), np.eye(4)
    rect[:3, :3] = np.asarray(c2c["R_rect_00"], dtype=np.float64).reshape(3, 3)
    tr[:3, :3] = np.asarray(v2c["R"], dtype=np.float64).reshape(3, 3)
    tr[:3, 3] = np.asarray(v2c["T"], dtype=np.float64).reshape(3)
    m = p @ rect @ tr
    m[0] -= float(crop_left) * m[2]
    m[1] -= float(crop_top) * m[2]
    return m.astype(np.float32)


def read_velodyne_bin(path):
    """A KITTI velodyne scan (.bin: little-endian float32 x, y, z, intensity per point) as an (N, 4)
    float32 array."""
    a = np.fromfile(path, dtype="<f4")
    if a.size % 4:
        raise ValueError(f"lidar: {path} holds {a.size} floats, not a whole number of 4-float points")
    return a.reshape(-1, 4).astype(np.float32, copy=False)
