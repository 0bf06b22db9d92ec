"""Predicted depth and the camera intrinsics to a metric 3-D point cloud, on the device.

Every loader of data.py returns `k`, the 3 x 3 intrinsics with the principal point shifted by the
crop, and DevicePrefetcher ships it with the frame. With it a completed depth map becomes points:

  backproject_map   organised xyz planes (B, 3, H, W), NaN where the pixel is not valid; one libnconv
                    launch (nconv_backproject_map, csrc/backproject.hip)
  backproject       the valid pixels compacted to a PointCloud (xyz, optional rgb and pixel index,
                    per-image offsets) in raster order, three launches and no host synchronisation
                    (nconv_backproject_points)
  normals           unit surface normals (B, 3, H, W) of the depth map on the image grid, NaN where a
                    pixel has none; one launch (nconv_depth_normals, csrc/normals.hip)
  normal_image      the camera-space normal picture (B, H, W, 3) uint8, ready for write_png8; the same
                    launch, the fp32 map never reaches memory
  write_ply         points (normals and colours) as a binary little-endian PLY, on the host

A pixel is valid iff z > z_min and z <= z_max and (no conf or conf >= conf_min); its point is
x = ((float)j - cx) * z / fx, y = ((float)i - cy) * z / fy, z: fp32, one rounding per operation.
A normal is the normalised cross product of the vertical and the horizontal difference of the
neighbouring points (central where both neighbours are valid and within jump_abs + jump_rel * z of the
pixel's depth, one-sided where one is), turned towards the camera; include/nconv.h has the arithmetic.
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


def _normals_opts(jump_rel, jump_abs, empty=(0, 0, 0)):
    from . import _lib
    jump_rel, jump_abs = float(jump_rel), float(jump_abs)
    if not (jump_rel >= 0.0 and jump_abs >= 0.0):
        raise ValueError(f"pointcloud: jump_rel = {jump_rel} and jump_abs = {jump_abs} must be >= 0")
    empty = tuple(int(c) for c in empty)
    if len(empty) != 3 or not all(0 <= c <= 255 for c in empty):
        raise ValueError(f"pointcloud: empty must be three values in 0..255, got {empty}")
    o = _lib.NconvNormalsOpts()
    o.jump_rel, o.jump_abs = jump_rel, jump_abs
    o.empty_rgb[0], o.empty_rgb[1], o.empty_rgb[2] = empty
    return o


def _depth_normals(depth, k, conf, conf_min, z_min, z_max, jump_rel, jump_abs, empty, out, want_map, want_image):
    from . import _lib
    o = _normals_opts(jump_rel, jump_abs, empty)
    d, (B, H, W) = _descriptor(depth, k, conf, conf_min, z_min, z_max)
    nmap = _output(out, "normals", (B, 3, H, W), torch.float32, depth.device) if want_map else None
    image = _output(out, "image", (B, H, W, 3), torch.uint8, depth.device) if want_image else None
    rc = _lib.lib().nconv_depth_normals(ctypes.byref(d), ctypes.byref(o), None if nmap is None else _lib.ptr(nmap),
                                        None if image is None else _lib.ptr(image), _lib.stream_handle(depth.device))
    _lib.check(rc, "nconv_depth_normals")
    return nmap, image


def normals(depth, k, *, conf=None, conf_min=0.0, z_min=0.0, z_max=FLT_MAX, jump_rel=0.1, jump_abs=0.0, out=None):
    """Unit surface normals (B, 3, H, W) fp32 of the depth map: planes nx, ny, nz in camera
    coordinates, turned towards the camera (n . P <= 0), NaN in all three where the pixel has no
    normal. depth, k, conf and the validity bounds as backproject_map takes them. A neighbour takes
    part in a pixel's differences only where it is valid and its depth is within jump_abs + jump_rel * z
    of the pixel's z (jump_rel = jump_abs = 0: every valid neighbour). out: an optional preallocated
    result. One launch."""
    return _depth_normals(depth, k, conf, conf_min, z_min, z_max, jump_rel, jump_abs, (0, 0, 0),
                          None if out is None else {"normals": out}, True, False)[0]


def normal_image(depth, k, *, conf=None, conf_min=0.0, z_min=0.0, z_max=FLT_MAX, jump_rel=0.1, jump_abs=0.0,
                 empty=(0, 0, 0), out=None):
    """The camera-space normal picture (B, H, W, 3) uint8 of the depth map, ready for write_png8:
    R, G, B = nx, -ny, -nz mapped from [-1, 1] to 0..255, `empty` where the pixel has no normal. The
    arguments are those of normals; the fp32 map is not written. One launch."""
    return _depth_normals(depth, k, conf, conf_min, z_min, z_max, jump_rel, jump_abs, empty,
                          None if out is None else {"image": out}, False, True)[1]


def normals_and_image(depth, k, *, conf=None, conf_min=0.0, z_min=0.0, z_max=FLT_MAX, jump_rel=0.1, jump_abs=0.0,
                      empty=(0, 0, 0), out=None):
    """(normals, normal_image) of the depth map from one launch. out: an optional dict of
    preallocated buffers 'normals' and 'image'."""
    return _depth_normals(depth, k, conf, conf_min, z_min, z_max, jump_rel, jump_abs, empty, out, True, True)


class PointCloud:
    """The result of backproject: device tensors at full capacity. xyz (capacity, 3) fp32; rgb
    (capacity, 3) uint8 or None; index (capacity) int32 = (b * H + i) * W + j or None; normals
    (capacity, 3) fp32 unit normals, (0, 0, 0) where a point has none, or None; offsets
    (B + 1) int32: image b's points are rows [offsets[b], offsets[b + 1]) and offsets[B] is the true
    number of valid pixels. Rows from min(offsets[B], capacity) on are not written. Building one does
    not synchronise; count(), image(b) and truncated() read offsets on the host (once)."""

    def __init__(self, xyz, rgb, index, offsets, normals=None):
        self.xyz, self.rgb, self.index, self.offsets, self.normals = xyz, rgb, index, offsets, normals
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

    def image_normals(self, b):
        """The normals rows of image b, matching image(b); None without normals."""
        o = self.host_offsets()
        lo, hi = min(o[b], self.capacity), min(o[b + 1], self.capacity)
        return None if self.normals is None else self.normals[lo:hi]


def backproject(depth, k, *, conf=None, conf_min=0.0, color=None, reverse=False, z_min=0.0, z_max=FLT_MAX,
                max_points=None, with_index=False, normals=False, jump_rel=0.1, jump_abs=0.0, out=None):
    """The valid pixels of depth as a PointCloud, raster order inside an image, images in batch
    order, the same on every run. depth, conf, k as backproject_map takes them. color: fp32 planes
    (B, 3, H, W) (-> clamp(rint(v), 0, 255), NaN -> 0) or uint8 interleaved (B, H, W, 3), unit
    innermost stride; the point's three bytes keep the source's channel order, reversed with
    reverse=True. max_points: the capacity of the outputs (default B * H * W); points beyond it are
    dropped and PointCloud.truncated() tells. with_index: also the pixel index of every point.
    normals: also every point's unit surface normal as the function normals defines it (jump_rel,
    jump_abs: its gate), (0, 0, 0) where the pixel has none; a fourth launch
    (nconv_depth_normals_points), which needs the index internally (PointCloud.index stays None
    without with_index). out: an optional dict of preallocated contiguous buffers 'xyz', 'rgb', 'index',
    'normals', 'offsets', 'workspace' (uint8, workspace_bytes(B, H, W)) -- static buffers under hipGraph
    capture. Three launches (four with normals), no allocation when out is complete, no host
    synchronisation."""
    from . import _lib
    opts = _normals_opts(jump_rel, jump_abs) if normals else None
    d, (B, H, W) = _descriptor(depth, k, conf, conf_min, z_min, z_max)
    dev = depth.device
    if color is not None:
        _color(d, color, reverse, (B, H, W), dev)
    cap = B * H * W if max_points is None else int(max_points)
    if cap < 0:
        raise ValueError(f"pointcloud: max_points = {max_points} is negative")
    xyz = _output(out, "xyz", (cap, 3), torch.float32, dev)
    rgb = _output(out, "rgb", (cap, 3), torch.uint8, dev) if color is not None else None
    index = _output(out, "index", (cap,), torch.int32, dev) if with_index or normals else None
    nrm = _output(out, "normals", (cap, 3), torch.float32, dev) if normals else None
    offsets = _output(out, "offsets", (B + 1,), torch.int32, dev)
    nws = workspace_bytes(B, H, W)
    ws = _output(out, "workspace", (nws,), torch.uint8, dev)
    # at capacity 0 nothing but offsets is written (an empty tensor has no storage to point at)
    rc = _lib.lib().nconv_backproject_points(
        ctypes.byref(d), _lib.ptr(xyz) if cap else None, _lib.ptr(rgb) if cap else None,
        _lib.ptr(index) if cap else None, cap, _lib.ptr(offsets), _lib.ptr(ws), nws, _lib.stream_handle(dev))
    _lib.check(rc, "nconv_backproject_points")
    if normals and cap:
        rc = _lib.lib().nconv_depth_normals_points(ctypes.byref(d), ctypes.byref(opts), _lib.ptr(index),
                                                   _lib.ptr(offsets), cap, _lib.ptr(nrm), _lib.stream_handle(dev))
        _lib.check(rc, "nconv_depth_normals_points")
    return PointCloud(xyz, rgb, index if with_index else None, offsets, nrm)


def workspace_bytes(B, H, W):
    """Bytes of backproject's workspace for a (B, H, W) batch (nconv_backproject_workspace_bytes)."""
    from . import _lib
    n = _lib.lib().nconv_backproject_workspace_bytes(int(B), int(H), int(W))
    if n == 0:
        raise ValueError(f"pointcloud: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31, "
                         "at most 2^24 row segments of 256 pixels)")
    return n


def write_ply(path, xyz, rgb=None, normals=None):
    """Points as a binary little-endian PLY: per vertex float x, y, z, with normals float nx, ny,
    nz, and with rgb uchar red, green, blue. xyz and normals (N, 3) float32, rgb (N, 3) uint8: host or
    device tensors or arrays, e.g. PointCloud.image(b)[:2] and PointCloud.image_normals(b). Host code
    (numpy)."""
    a = xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else np.asarray(xyz)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype != np.float32:
        raise TypeError(f"pointcloud: write_ply takes float32 (N, 3) points, got {a.dtype} {a.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    c = nv = None
    if normals is not None:
        nv = normals.detach().cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals)
        if nv.shape != a.shape or nv.dtype != np.float32:
            raise TypeError(f"pointcloud: write_ply takes float32 {a.shape} normals, got {nv.dtype} {nv.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb is not None:
        c = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
        if c.shape != a.shape or c.dtype != np.uint8:
            raise TypeError(f"pointcloud: write_ply takes uint8 {a.shape} colours, got {c.dtype} {c.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(a.shape[0], dtype=np.dtype(fields))  # packed: 12 or 15 bytes per vertex, 12 more with normals
    for n, name in enumerate("xyz"):
        rec[name] = a[:, n]
    if nv is not None:
        for n, name in enumerate(("nx", "ny", "nz")):
            rec[name] = nv[:, n]
    if c is not None:
        for n, name in enumerate(("red", "green", "blue")):
            rec[name] = c[:, n]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {a.shape[0]}",
            "property float x", "property float y", "property float z"]
    if nv is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    if c is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
