"""Raw sensor frames in, 16-bit depth out, on the device.

The loaders of data.py decode on the host (uint8 -> fp32, HWC -> CHW) and ship fp32 across the link:
20 bytes per pixel for rgb + depth + gt where the stored data is 7 (3 x u8, u16, u16), 4 against 2
for DNET's sparse depth alone. With `raw=True` they hand out the stored integers instead, and

  ingest            one libnconv launch (nconv_frame_ingest, csrc/frame_io.hip) turns a batch of them
                    into the fp32 tensors the models take, bit for bit what the host decode gives
  Ingest            the same as a callable on a batch dict (DevicePrefetcher(..., ingest=Ingest()))
  export_depth16    a prediction as uint16 fixed point (nconv_depth_export_u16; scale 256 = KITTI)
  write_depth_png16 a uint16 plane as a 16-bit grayscale PNG (KITTI's submission format)

Device tensors only: there is no PyTorch path.
"""
import ctypes

import numpy as np
import torch

from . import _views

# depth_decode -> (shift, scale) of an integer plane: data.imread_gray's two decodes, then / 256
DECODES = {"reference": {torch.uint16: (8, 1.0 / 256.0), torch.uint8: (0, 1.0 / 256.0)},
           "kitti16": {torch.uint16: (0, 1.0 / 256.0), torch.uint8: (0, 1.0 / 256.0)}}


def _on_device(x, what):
    _views.on_device(x, what, "frames", "frames are converted by libnconv")


def _decode(depth_decode, dtype):
    """(shift, scale) of a plane of dtype under depth_decode (a name or an explicit pair)."""
    if isinstance(depth_decode, str):
        if depth_decode not in DECODES:
            raise ValueError(f"depth_decode must be 'reference', 'kitti16' or (shift, scale), got {depth_decode!r}")
        return (0, 1.0) if dtype == torch.float32 else DECODES[depth_decode][dtype]
    shift, scale = depth_decode
    return int(shift), float(scale)


def _rgb_view(x):
    """(B, h, w, image stride, row stride in bytes) of an interleaved uint8 (B, h, w, 3) view."""
    _views.require_tensor(x, "rgb", (torch.uint8,), "frames")
    return _views.interleaved_u8_view(x, "rgb", "frames")


def _plane_view(x, what):
    """(B, h, w, image stride, row stride in bytes) of a (B, h, w) or (B, 1, h, w) view."""
    _views.require_tensor(x, what, (torch.uint16, torch.uint8, torch.float32), "frames")
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3:
        raise ValueError(f"frames: {what} must be (B, h, w) or (B, 1, h, w), got {tuple(x.shape)}")
    if x.stride(2) != 1:
        raise ValueError(f"frames: {what} of strides {x.stride()} has no unit innermost stride")
    e = x.element_size()
    return x.shape[0], x.shape[1], x.shape[2], x.stride(0) * e, x.stride(1) * e


def _output(out, key, shape, dtype, device):
    return _views.output(out, key, shape, dtype, device, "frames")


def ingest(rgb=None, depth=None, gt=None, *, depth_decode="reference", reverse_rgb=True, out=None):
    """{'rgb': (B, 3, h, w), 'depth': (B, 1, h, w), 'gt': (B, 1, h, w)} fp32, for the sources given.

    rgb: uint8 (B, h, w, 3) device tensor, interleaved; reverse_rgb writes the planes in reverse
    channel order (an RGB decode -> cv2.imread's BGR, what the loaders return). depth, gt: uint16 /
    uint8 / float32 (B, h, w) or (B, 1, h, w); an integer v becomes float(v >> shift) * scale with
    (shift, scale) = depth_decode: 'reference' (the 8-bit read of the reference: v >> 8, / 256),
    'kitti16' (v / 256 metres) or an explicit pair; under the two names a float32 plane is copied.
    Sliced views (crops) are accepted as long as the innermost stride is 1. out: an optional dict of
    preallocated contiguous outputs (static buffers under hipGraph capture). One launch."""
    from . import _lib
    if rgb is None and depth is None and gt is None:
        raise ValueError("frames: ingest needs at least one of rgb, depth, gt")
    d = _lib.NconvFrameIngest()
    geom, device = None, None

    def same(g, dev, what):
        nonlocal geom, device
        if geom is None:
            geom, device = g, dev
        elif g != geom:
            raise ValueError(f"frames: {what} is (B, h, w) = {g}, the other sources {geom}")
        elif dev != device:
            raise RuntimeError(f"frames: {what} on {dev}, the other sources on {device}")

    res = {}
    if rgb is not None:
        B, h, w, bs, rs = _rgb_view(rgb)
        _on_device(rgb, "rgb")
        same((B, h, w), rgb.device, "rgb")
        res["rgb"] = _output(out, "rgb", (B, 3, h, w), torch.float32, rgb.device)
        d.rgb, d.rgb_image_stride, d.rgb_row_stride = rgb.data_ptr(), bs, rs
        d.rgb_out, d.reverse = res["rgb"].data_ptr(), int(bool(reverse_rgb))
    for k, (key, x) in enumerate((("depth", depth), ("gt", gt))):
        if x is None:
            continue
        B, h, w, bs, rs = _plane_view(x, key)
        _on_device(x, key)
        same((B, h, w), x.device, key)
        res[key] = _output(out, key, (B, 1, h, w), torch.float32, x.device)
        p = d.plane[k]
        p.src, p.image_stride, p.row_stride = x.data_ptr(), bs, rs
        p.dtype = {torch.uint8: _lib.FRAME_U8, torch.uint16: _lib.FRAME_U16, torch.float32: _lib.FRAME_F32}[x.dtype]
        p.shift, p.scale = _decode(depth_decode, x.dtype)
        p.out = res[key].data_ptr()
    d.B, d.h, d.w = geom
    _lib.check(_lib.lib().nconv_frame_ingest(ctypes.byref(d), _lib.stream_handle(device)), "nconv_frame_ingest")
    return res


def export_depth16(pred, scale=256.0, out=None):
    """pred as uint16 fixed point, of pred's shape: clamp(round_half_even(pred * scale), 0, 65535),
    NaN -> 0. pred: fp32 device tensor, (H, W), (1, H, W) or (B, 1, H, W) with unit-stride rows (a
    cropped view such as DNET's output works). scale = 256 is KITTI's format. One launch."""
    from . import _lib
    _views.require_tensor(pred, "pred", (torch.float32,), "frames")
    B, H, W, bs, rs = _views.plane_view(pred, "pred", "frames")
    _on_device(pred, "pred")
    res = _output(None if out is None else {"out": out}, "out", pred.shape, torch.uint16, pred.device)
    rc = _lib.lib().nconv_depth_export_u16(_lib.ptr(pred), bs, rs, B, H, W, float(scale), _lib.ptr(res),
                                           _lib.stream_handle(pred.device))
    _lib.check(rc, "nconv_depth_export_u16")
    return res


def write_depth_png16(path, plane):
    """A uint16 (H, W) plane (host or device tensor, or array; leading singleton axes dropped) as a
    16-bit grayscale PNG (Pillow mode I;16), e.g. export_depth16(pred)[b] for a KITTI submission."""
    from PIL import Image
    a = plane.detach().cpu().numpy() if torch.is_tensor(plane) else np.asarray(plane)
    if a.dtype != np.uint16:
        raise TypeError(f"frames: write_depth_png16 takes uint16, got {a.dtype}")
    a = a.reshape(a.shape[-2:]) if a.ndim >= 2 and a.size == a.shape[-2] * a.shape[-1] else a
    if a.ndim != 2:
        raise ValueError(f"frames: write_depth_png16 takes one (H, W) plane, got {tuple(plane.shape)}")
    Image.fromarray(np.ascontiguousarray(a)).save(path, format="PNG")


class Ingest:
    """A raw batch (the `raw=True` loaders' collated samples, on the device) -> the batch the loaders
    return today: 'rgb' uint8 (B, h, w, 3) -> fp32 BGR planes (B, 3, h, w); integer 'depth' / 'gt'
    (B, h, w) -> fp32 (B, 1, h, w) under depth_decode; fp32 planes (NYU's) and every other entry are
    passed through. One launch per batch; meant for DevicePrefetcher(..., ingest=Ingest())."""

    def __init__(self, depth_decode="reference", reverse_rgb=True):
        self.depth_decode, self.reverse_rgb = depth_decode, reverse_rgb

    def __call__(self, batch):
        src = {}
        v = batch.get("rgb")
        if torch.is_tensor(v) and v.dtype == torch.uint8:
            src["rgb"] = v
        for k in ("depth", "gt"):
            v = batch.get(k)
            if torch.is_tensor(v) and v.dtype in (torch.uint8, torch.uint16):
                src[k] = v
        if not src:
            return batch
        out = dict(batch)
        out.update(ingest(**src, depth_decode=self.depth_decode, reverse_rgb=self.reverse_rgb))
        return out
