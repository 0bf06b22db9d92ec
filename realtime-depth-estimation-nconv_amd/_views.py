"""Argument checks shared by the modules that hand tensors to libnconv's I/O entry points
(metrics, frames, pointcloud, lidar, visualize, sparsify, occlusion, sparsification, ipbasic, nearest, voxelmap): what a strided view of planes
is on the Python side.

Every helper takes the calling module's `prefix` ("frames", "depth metrics", ...), so the text of an
exception names the module the caller used.
"""
import torch

from .train import _planes


def require_tensor(x, what, dtypes, prefix, expected=None):
    """x if it is a tensor of one of dtypes, else TypeError; expected: how the message names them."""
    if not torch.is_tensor(x):
        raise TypeError(f"{prefix}: {what} must be a tensor, got {type(x).__name__}")
    if x.dtype not in dtypes:
        expected = expected or " / ".join(str(d) for d in dtypes)
        raise TypeError(f"{prefix}: {what}: expected {expected}, got {x.dtype}")
    return x


def on_device(x, what, prefix, doing):
    """RuntimeError unless x is on a GPU; doing: the module's sentence on what libnconv does there."""
    if not x.is_cuda:
        raise RuntimeError(f"{prefix}: {what} is on {x.device}; {doing} on ROCm devices only (no PyTorch fallback), "
                           "move the tensors to the GPU")


def plane_view(x, what, prefix):
    """(B, H, W, image stride, row stride in elements) of an (H, W), (1, H, W) or (B, 1, H, W) view."""
    g = _planes(x)
    if g is None:
        raise ValueError(f"{prefix}: {what} of shape {tuple(x.shape)} / strides {x.stride()} is not an (H, W), "
                         "(1, H, W) or (B, 1, H, W) set of unit-stride rows")
    return g[0], x.shape[-2], x.shape[-1], g[1], g[2]


def interleaved_u8_view(x, what, prefix, shape=None):
    """(B, h, w, image stride, row stride in bytes) of an interleaved uint8 (B, h, w, 3) view; with
    shape = (B, h, w) the view must have it, and an (h, w, 3) tensor is one image."""
    if shape is None:
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"{prefix}: {what} must be (B, h, w, 3), got {tuple(x.shape)}")
    else:
        if x.dim() == 3:
            x = x[None]
        if tuple(x.shape) != (*shape, 3):
            raise ValueError(f"{prefix}: uint8 {what} must be ({shape[0]}, {shape[1]}, {shape[2]}, 3) interleaved, "
                             f"got {tuple(x.shape)}")
    if x.stride(3) != 1 or x.stride(2) != 3:
        raise ValueError(f"{prefix}: {what} of strides {x.stride()} is not interleaved (unit innermost stride, pixel "
                         "stride 3)")
    return x.shape[0], x.shape[1], x.shape[2], x.stride(0), x.stride(1)


def output(out, key, shape, dtype, device, prefix, source="source"):
    """out[key] checked against (shape, dtype, device), or a new tensor where out has none."""
    t = None if out is None else out.get(key)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise TypeError(f"{prefix}: out[{key!r}] must be a contiguous {dtype} tensor of shape {tuple(shape)}")
    if t.device != device:
        raise RuntimeError(f"{prefix}: out[{key!r}] on {t.device}, the {source} on {device}")
    return t


def dest_plane(out, key, B, H, W, device, prefix, source="source"):
    """(tensor, image stride, row stride in elements) of the fp32 destination out[key], any (B, 1, H, W)
    view of unit-stride rows on device, or of a new contiguous tensor where out has none."""
    t = None if out is None else out.get(key)
    if t is None:
        t = torch.empty((B, 1, H, W), dtype=torch.float32, device=device)
    else:
        require_tensor(t, f"out[{key!r}]", (torch.float32,), prefix)
        if t.device != device:
            raise RuntimeError(f"{prefix}: out[{key!r}] on {t.device}, {source} on {device}")
    tB, tH, tW, bs, rs = plane_view(t, f"out[{key!r}]", prefix)
    if (tB, tH, tW) != (B, H, W):
        raise TypeError(f"{prefix}: out[{key!r}] of shape {tuple(t.shape)} does not match {source}'s "
                        f"{B} x {H} x {W}")
    return t, bs, rs
