"""Predicted depth and the camera intrinsics to a metric 3-D point cloud, on the device.

Every loader of data.py returns `k`, the 3 x 3 intrinsics with the principal point shifted by the
crop, and DevicePrefetcher ships it with the frame. With it a completed depth map becomes points:

  backproject_map   organised xyz planes (B, 3, H, W), NaN where the pixel is not valid; one libnconv
                    launch (nconv_backproject_map, csrc/backproject.hip)
  backproject       the valid pixels compacted to a PointCloud (xyz, optional rgb and pixel index,
                    per-image offsets) in raster order, three launches and no host synchronisation
                    (nconv_backproject_points)
  write_ply         points (and colours) as a binary little-endian PLY, on the host

A pixel is valid iff z > z_min and z <= z_max and (no conf or conf >= conf_min); its point is
x = ((float)j - cx) * z / fx, y = ((float)i - cy) * z / fy, z: fp32, one rounding per operation.
The confidence is the network's own (DNET.forward_with_confidence). Device tensors only: there is no
PyTorch path.
"""
import ctypes

import numpy as np
import torch

from . import _views

FLT_MAX = float(np.finfo(np.float32).max)


def _on_device(x, what):
    _views.on_device(x, what, "pointcloud", "points are computed by libnconv")


def _f32(x, what):
    return _views.require_tensor(x, what, (torch.float32,), "pointcloud")


def _plane_geometry(x, what):
    """(B, H, W, image stride, row stride) of an (H, W), (1, H, W) or (B, 1, H, W) fp32 view."""
    return _views.plane_view(_f32(x, what), what, "pointcloud")


def _descriptor(depth, k, conf, conf_min, z_min, z_max):
    """(descriptor, (B, H, W)) of the sources shared by the two calls; raises on a malformed one."""
    from . import _lib
    B, H, W, bs, rs = _plane_geometry(depth, "depth")
    _f32(k, "k")
    if tuple(k.shape) not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"pointcloud: k must be (3, 3) or ({B}, 3, 3), got {tuple(k.shape)}")
    if not k.is_contiguous():
        raise ValueError(f"pointcloud: k of strides {k.stride()} is not contiguous")
    _on_device(depth, "depth")
    _on_device(k, "k")
    if k.device != depth.device:
        raise RuntimeError(f"pointcloud: k on {k.device}, depth on {depth.device}")
    d = _lib.NconvBackproject()
    d.B, d.H, d.W = B, H, W
    d.depth, d.depth_image_stride, d.depth_row_stride = depth.data_ptr(), bs, rs
    d.k, d.k_image_stride = k.data_ptr(), (9 if k.dim() == 3 else 0)
    if conf is not None:
        g = _plane_geometry(conf, "conf")
        if g[:3] != (B, H, W):
            raise ValueError(f"pointcloud: conf is (B, H, W) = {g[:3]}, depth {(B, H, W)}")
        _on_device(conf, "conf")
        if conf.device != depth.device:
            raise RuntimeError(f"pointcloud: conf on {conf.device}, depth on {depth.device}")
        d.conf, d.conf_image_stride, d.conf_row_stride = conf.data_ptr(), g[3], g[4]
    z_min, z_max = float(z_min), float(z_max)
    if not z_max >= z_min:
        raise ValueError(f"pointcloud: z_max = {z_max} < z_min = {z_min}")
    if z_max == 0.0 and z_min >= 0.0:  # (0, 0] is empty; in the C descriptor this pair means "no upper bound"
        raise ValueError("pointcloud: z_min = z_max = 0 selects no pixel")
    d.z_min, d.z_max, d.conf_min = z_min, z_max, float(conf_min)
    return d, (B, H, W)


def _color(d, color, reverse, geom, device):
    from . import _lib
    B, H, W = geom
    if not torch.is_tensor(color):
        raise TypeError(f"pointcloud: color must be a tensor, got {type(color).__name__}")
    if color.dtype == torch.float32:
        if color.dim() == 3:
            color = color[None]
        if tuple(color.shape) != (B, 3, H, W):
            raise ValueError(f"pointcloud: fp32 color must be ({B}, 3, {H}, {W}) planes, got {tuple(color.shape)}")
        if color.stride(3) != 1:
            raise ValueError(f"pointcloud: color of strides {color.stride()} has no unit innermost stride")
        d.color_kind = _lib.COLOR_F32_PLANAR
        d.color_image_stride, d.color_channel_stride, d.color_row_stride = color.stride(0), color.stride(1), color.stride(2)
    elif color.dtype == torch.uint8:
        d.color_kind = _lib.COLOR_U8_INTERLEAVED
        d.color_image_stride, d.color_row_stride = _views.interleaved_u8_view(color, "color", "pointcloud", geom)[3:]
    else:
        raise TypeError(f"pointcloud: color: expected torch.float32 planes or torch.uint8 interleaved, got {color.dtype}")
    _on_device(color, "color")
    if color.device != device:
        raise RuntimeError(f"pointcloud: color on {color.device}, depth on {device}")
    d.color, d.reverse = color.data_ptr(), int(bool(reverse))


def _output(out, key, shape, dtype, device):
    return _views.output(out, key, shape, dtype, device, "pointcloud")


def backproject_map(depth, k, *, conf=None, conf_min=0.0, z_min=0.0, z_max=FLT_MAX, out=None):
    """Organised points (B, 3, H, W) fp32: planes x, y, z of every pixel, NaN in all three where
    the pixel is not valid. depth (and conf): fp32 device tensors, (H, W), (1, H, W) or (B, 1, H, W)
    with unit-stride rows (a cropped view such as DNET's output works); k: (3, 3) or (B, 3, 3) fp32 on
    the device, of which fx, fy, cx, cy are read. out: an optional preallocated result. One launch."""
    from . import _lib
    d, (B, H, W) = _descriptor(depth, k, conf, conf_min, z_min, z_max)
    res = _output(None if out is None else {"out": out}, "out", (B, 3, H, W), torch.float32, depth.device)
    rc = _lib.lib().nconv_backproject_map(ctypes.byref(d), _lib.ptr(res), _lib.stream_handle(depth.device))
    _lib.check(rc, "nconv_backproject_map")
    return res


class PointCloud:
    """The result of backproject: device tensors at full capacity. xyz (capacity, 3) fp32; rgb
    (capacity, 3) uint8 or None; index (capacity) int32 = (b * H + i) * W + j or None; offsets
    (B + 1) int32: image b's points are rows [offsets[b], offsets[b + 1]) and offsets[B] is the true
    number of valid pixels. Rows from min(offsets[B], capacity) on are not written. Building one does
    not synchronise; count(), image(b) and truncated() read offsets on the host (once)."""

    def __init__(self, xyz, rgb, index, offsets):
        self.xyz, self.rgb, self.index, self.offsets = xyz, rgb, index, offsets
        self._host = None

    @property
    def capacity(self):
        return self.xyz.shape[0]

    def host_offsets(self):
        """offsets as a list of ints: the one host read (a synchronisation), then cached."""
        if self._host is None:
            self._host = self.offsets.cpu().tolist()
        return self._host

    def count(self):
        """The true number of valid pixels (may exceed the capacity)."""
        return self.host_offsets()[-1]

    def truncated(self):
        return self.count() > self.capacity

    def image(self, b):
        """(xyz, rgb, index) rows of image b (what the capacity kept of them)."""
        o = self.host_offsets()
        lo, hi = min(o[b], self.capacity), min(o[b + 1], self.capacity)
        return (self.xyz[lo:hi], None if self.rgb is None else self.rgb[lo:hi],
                None if self.index is None else self.index[lo:hi])


def backproject(depth, k, *, conf=None, conf_min=0.0, color=None, reverse=False, z_min=0.0, z_max=FLT_MAX,
                max_points=None, with_index=False, out=None):
    """The valid pixels of depth as a PointCloud, raster order inside an image, images in batch
    order, the same on every run. depth, conf, k as backproject_map takes them. color: fp32 planes
    (B, 3, H, W) (-> clamp(rint(v), 0, 255), NaN -> 0) or uint8 interleaved (B, H, W, 3), unit
    innermost stride; the point's three bytes keep the source's channel order, reversed with
    reverse=True. max_points: the capacity of the outputs (default B * H * W); points beyond it are
    dropped and PointCloud.truncated() tells. with_index: also the pixel index of every point.
    out: an optional dict of preallocated contiguous buffers 'xyz', 'rgb', 'index', 'offsets',
    'workspace' (uint8, workspace_bytes(B, H, W)) -- static buffers under hipGraph capture. Three
    launches, no allocation when out is complete, no host synchronisation."""
    from . import _lib
    d, (B, H, W) = _descriptor(depth, k, conf, conf_min, z_min, z_max)
    dev = depth.device
    if color is not None:
        _color(d, color, reverse, (B, H, W), dev)
    cap = B * H * W if max_points is None else int(max_points)
    if cap < 0:
        raise ValueError(f"pointcloud: max_points = {max_points} is negative")
    xyz = _output(out, "xyz", (cap, 3), torch.float32, dev)
    rgb = _output(out, "rgb", (cap, 3), torch.uint8, dev) if color is not None else None
    index = _output(out, "index", (cap,), torch.int32, dev) if with_index else None
    offsets = _output(out, "offsets", (B + 1,), torch.int32, dev)
    nws = workspace_bytes(B, H, W)
    ws = _output(out, "workspace", (nws,), torch.uint8, dev)
    # at capacity 0 nothing but offsets is written (an empty tensor has no storage to point at)
    rc = _lib.lib().nconv_backproject_points(
        ctypes.byref(d), _lib.ptr(xyz) if cap else None, _lib.ptr(rgb) if cap else None,
        _lib.ptr(index) if cap else None, cap, _lib.ptr(offsets), _lib.ptr(ws), nws, _lib.stream_handle(dev))
    _lib.check(rc, "nconv_backproject_points")
    return PointCloud(xyz, rgb, index, offsets)


def workspace_bytes(B, H, W):
    """Bytes of backproject's workspace for a (B, H, W) batch (nconv_backproject_workspace_bytes)."""
    from . import _lib
    n = _lib.lib().nconv_backproject_workspace_bytes(int(B), int(H), int(W))
    if n == 0:
        raise ValueError(f"pointcloud: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31, "
                         "at most 2^24 row segments of 256 pixels)")
    return n


def write_ply(path, xyz, rgb=None):
    """Points as a binary little-endian PLY: per vertex float x, y, z and, with rgb, uchar red,
    green, blue. xyz (N, 3) float32, rgb (N, 3) uint8: host or device tensors or arrays, e.g.
    PointCloud.image(b)[:2]. Host code (numpy)."""
    a = xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else np.asarray(xyz)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype != np.float32:
        raise TypeError(f"pointcloud: write_ply takes float32 (N, 3) points, got {a.dtype} {a.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    c = None
    if rgb is not None:
        c = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
        if c.shape != a.shape or c.dtype != np.uint8:
            raise TypeError(f"pointcloud: write_ply takes uint8 {a.shape} colours, got {c.dtype} {c.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(a.shape[0], dtype=np.dtype(fields))  # packed: 12 or 15 bytes per vertex
    for n, name in enumerate("xyz"):
        rec[name] = a[:, n]
    if c is not None:
        for n, name in enumerate(("red", "green", "blue")):
            rec[name] = c[:, n]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {a.shape[0]}",
            "property float x", "property float y", "property float z"]
    if c is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
