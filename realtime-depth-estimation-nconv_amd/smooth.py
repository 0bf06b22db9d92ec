"""The edge-aware depth smoothness loss on the device: the regulariser the photometric term (warp.py) is
trained with.

On road, sky and walls every depth explains the image equally well, so the papers that train with a
photometric term pair it with a penalty on the predicted depth's differences: the L1 of its first
differences, relaxed where the image itself has an edge (monodepth; order=1), or the L1 of its second
differences (Ma, Cavalheiro, Karaman, ICRA 2019; order=2).

  edge_weights        rgb (B, C, H, W) -> (B, 2, H, W): wx = E(alpha mean_ch |I[j + 1] - I[j]|), wy likewise
                      down the rows (nconv_edge_weights: one launch); made once per batch, beside the loader
  smoothness_loss     sum wx |tx| / n_x + sum wy |ty| / n_y over the terms whose pixels the mask keeps,
                      differentiable in the depth only (nconv_smooth_loss_fwd / _bwd: two launches forward,
                      one backward)
  SmoothnessLoss      the same as an nn.Module
  Smoother            the same with loss, gradient and workspace kept between calls (hipGraph capture)
  EdgeWeights         a DevicePrefetcher batch stage: batch["edge_w"] = edge_weights(batch["rgb"])

The rule (include/nconv.h, fp32, one rounding per operation): order 1, tx = d[j + 1] - d[j] weighted by
wx(j); order 2, tx = (d[j - 1] + d[j + 1]) - 2 d[j] weighted by min(wx(j - 1), wx(j)); a term counts where
the mask keeps all its pixels; the gradient is gathered per pixel (no atomics), so the results are the same
bits on every run. E is exp(-x) written out as a range reduction, a degree-6 polynomial and a power of
two: no library exponential, so numpy and the device agree bit for bit.

Not offered: normalising the depth by its mean (or a disparity), the mixed derivative, a gradient with
respect to the weights or the image. Device tensors only: there is no PyTorch path.

In a training step:
  loss = calculate_loss(pred, gt, True) + w1 * photo(pred, k, rgb, rgb_near, m) + w2 * smooth(pred, batch["edge_w"])
"""
import ctypes

import torch

from . import _views

PREFIX = "smooth"


def _plane_count(B, H, W):
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31)")
    return B, H, W


def workspace_bytes(B, H, W):
    """Bytes of smoothness_loss's workspace (nconv_smooth_loss_workspace_bytes); its first two int32 are
    n_x and n_y."""
    from . import _lib
    return _lib.lib().nconv_smooth_loss_workspace_bytes(*_plane_count(B, H, W))


def edge_weights(rgb, alpha=1.0 / 255.0, out=None):
    """(B, 2, H, W) fp32: plane 0 the weight E(alpha g) of the edge between columns j and j + 1, g the mean
    over the channels of |rgb[j + 1] - rgb[j]|, plane 1 likewise between rows i and i + 1; the last column
    of plane 0 and the last row of plane 1 are 1. rgb: (B, C, H, W) fp32 view of unit-stride rows, C = 1 or
    3; alpha: 1 / 255 for frames of 8-bit values (the monodepth recipe on [0, 1] images), 1 for frames
    already in [0, 1]. out: an optional contiguous (B, 2, H, W) fp32 tensor to fill. One launch."""
    from . import _lib
    _views.require_tensor(rgb, "rgb", (torch.float32,), PREFIX)
    if rgb.dim() != 4 or rgb.shape[1] not in (1, 3):
        raise ValueError(f"{PREFIX}: rgb must be (B, C, H, W) with C = 1 or 3, got {tuple(rgb.shape)}")
    B, C, H, W = rgb.shape
    _plane_count(B * C, H, W)
    if rgb.stride(3) != 1 and W > 1:
        raise ValueError(f"{PREFIX}: rgb of strides {rgb.stride()} has no unit-stride rows")
    alpha = float(alpha)
    if not 0.0 <= alpha < float("inf"):
        raise ValueError(f"{PREFIX}: alpha = {alpha} must be finite and >= 0")
    _views.on_device(rgb, "rgb", PREFIX, "edge weights are made by libnconv")
    w = _views.output(None if out is None else {"weights": out}, "weights", (B, 2, H, W), torch.float32, rgb.device,
                      PREFIX, source="rgb")
    d = _lib.NconvEdgeWeights()
    d.B, d.C, d.H, d.W, d.alpha = B, C, H, W, alpha
    d.image, d.image_stride, d.channel_stride = rgb.data_ptr(), rgb.stride(0), rgb.stride(1)
    d.row_stride = rgb.stride(2) if H > 1 else max(rgb.stride(2), W)
    _lib.check(_lib.lib().nconv_edge_weights(ctypes.byref(d), _lib.ptr(w), _lib.stream_handle(rgb.device)),
               "nconv_edge_weights")
    return w


def _descriptor(depth, weights, order, mask):
    """The checked operands as (NconvSmoothLoss, (B, H, W), mask as uint8). Shapes, dtypes and gradients
    are checked before the devices, so that a wrong call says what is wrong with it wherever it runs."""
    from . import _lib
    _views.require_tensor(depth, "depth", (torch.float32,), PREFIX)
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"{PREFIX}: depth must be (B, 1, H, W), got {tuple(depth.shape)}")
    B, H, W, dbs, drs = _views.plane_view(depth, "depth", PREFIX)
    if order not in (1, 2):
        raise ValueError(f"{PREFIX}: order must be 1 (first differences) or 2 (second differences), got {order!r}")
    d = _lib.NconvSmoothLoss()
    if weights is not None:
        _views.require_tensor(weights, "weights", (torch.float32,), PREFIX)
        if tuple(weights.shape) != (B, 2, H, W):
            raise ValueError(f"{PREFIX}: weights must be ({B}, 2, {H}, {W}) (edge_weights), got {tuple(weights.shape)}")
        if not weights.is_contiguous():
            raise ValueError(f"{PREFIX}: weights of strides {weights.stride()} is not contiguous")
        if weights.requires_grad:
            raise ValueError(f"{PREFIX}: weights requires a gradient, and only the depth gets one (the weights and "
                             "the image they come from are inputs): pass weights.detach()")
    if mask is not None:
        _views.require_tensor(mask, "mask", (torch.bool, torch.uint8), PREFIX)
        if mask.dim() == 3:
            mask = mask[:, None]
        if tuple(mask.shape) != (B, 1, H, W):
            raise ValueError(f"{PREFIX}: mask must be ({B}, 1, {H}, {W}) or ({B}, {H}, {W}), got {tuple(mask.shape)}")
        if mask.requires_grad:
            raise ValueError(f"{PREFIX}: mask requires a gradient, and only the depth gets one: pass mask.detach()")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        _, _, _, d.mask_image_stride, d.mask_row_stride = _views.plane_view(mask, "mask", PREFIX)
    _plane_count(B, H, W)
    dev = depth.device
    for name, x in (("depth", depth), ("weights", weights), ("mask", mask)):
        if x is None:
            continue
        _views.on_device(x, name, PREFIX, "the smoothness loss is computed by libnconv")
        if x.device != dev:
            raise RuntimeError(f"{PREFIX}: {name} on {x.device}, depth on {dev}")
    d.B, d.H, d.W, d.order = B, H, W, order
    d.depth, d.depth_image_stride, d.depth_row_stride = depth.data_ptr(), dbs, drs
    d.mask = None if mask is None else mask.data_ptr()
    d.weights = None if weights is None else weights.data_ptr()
    return d, (B, H, W), mask


class SmoothLossFn(torch.autograd.Function):
    """smoothness_loss's kernels (nconv_smooth_loss_fwd / _bwd); the gradient reaches the depth alone."""

    @staticmethod
    def forward(ctx, depth, weights, order, mask, out):
        from . import _lib
        d, (B, H, W), mask = _descriptor(depth, weights, order, mask)
        dev = depth.device
        nbytes = workspace_bytes(B, H, W)
        ws = _views.output(out, "workspace", (nbytes,), torch.uint8, dev, PREFIX, source="depth")
        loss = _views.output(out, "loss", (), torch.float32, dev, PREFIX, source="depth")
        rc = _lib.lib().nconv_smooth_loss_fwd(ctypes.byref(d), _lib.ptr(loss), _lib.ptr(ws), nbytes,
                                              _lib.stream_handle(dev))
        _lib.check(rc, "nconv_smooth_loss_fwd")
        ctx.order = order
        ctx.g_depth = None if out is None else out.get("g_depth")
        ctx.save_for_backward(depth, weights, mask, ws)
        counts = ws[:8].view(torch.int32)
        ctx.mark_non_differentiable(counts)
        return loss, counts

    @staticmethod
    def backward(ctx, gloss, _g_counts):
        from . import _lib
        depth, weights, mask, ws = ctx.saved_tensors
        d, (B, H, W), _ = _descriptor(depth, weights, ctx.order, mask)
        gloss = gloss.contiguous()
        g = ctx.g_depth if ctx.g_depth is not None else torch.empty((B, 1, H, W), dtype=torch.float32,
                                                                    device=depth.device)
        rc = _lib.lib().nconv_smooth_loss_bwd(ctypes.byref(d), _lib.ptr(gloss), _lib.ptr(ws), ws.numel(), _lib.ptr(g),
                                              _lib.stream_handle(depth.device))
        _lib.check(rc, "nconv_smooth_loss_bwd")
        return g, None, None, None, None


def smoothness_loss(depth, weights=None, order=1, mask=None, return_counts=False, out=None):
    """sum wx |tx| / max(n_x, 1) + sum wy |ty| / max(n_y, 1): a scalar on the device, or (loss, counts) with
    return_counts, counts the int32 pair (n_x, n_y) of terms that took part (a view of the workspace: no
    host synchronisation). depth: (B, 1, H, W) fp32, any view of unit-stride rows (DNET's cropped output);
    weights: None (every weight 1) or edge_weights' (B, 2, H, W); order: 1, first differences, or 2,
    second differences; mask: optional bool / uint8 (B, 1, H, W), a term counts where all its pixels are
    not 0. Differentiable in depth only: weights or a mask that require a gradient are refused. out: an
    optional dict of kept contiguous buffers 'workspace' (uint8, workspace_bytes(B, H, W)), 'loss' (fp32
    scalar), 'g_depth' (B, 1, H, W). Two launches forward, one backward."""
    loss, counts = SmoothLossFn.apply(depth, weights, order, mask, out)
    return (loss, counts) if return_counts else loss


class SmoothnessLoss(torch.nn.Module):
    """smoothness_loss with its order held: loss(depth, weights=None, mask=None)."""

    def __init__(self, order=1):
        super().__init__()
        if order not in (1, 2):
            raise ValueError(f"{PREFIX}: order must be 1 (first differences) or 2 (second differences), got {order!r}")
        self.order = order

    def forward(self, depth, weights=None, mask=None):
        return smoothness_loss(depth, weights, self.order, mask)


class Smoother:
    """smoothness_loss for a fixed size with its loss, gradient and workspace kept between calls: no
    allocation after construction, so the call and its backward can be captured with torch.cuda.graph and
    replayed on operands refilled in place. smoother(depth, weights) -> loss (or (loss, counts)). The
    returned tensors are the kept ones, overwritten by the next call."""

    def __init__(self, size, B=1, order=1, device=None):
        H, W = (int(v) for v in size)
        if min(H, W, int(B)) <= 0 or order not in (1, 2):
            raise ValueError(f"{PREFIX}: sizes must be positive and order 1 or 2, got {size}, B={B}, order={order!r}")
        self.size, self.B, self.order = (H, W), int(B), order
        dev = torch.device("cuda" if device is None else device)
        self._out = {"workspace": torch.empty(workspace_bytes(self.B, H, W), dtype=torch.uint8, device=dev),
                     "loss": torch.empty((), dtype=torch.float32, device=dev),
                     "g_depth": torch.empty(self.B, 1, H, W, dtype=torch.float32, device=dev)}

    def __call__(self, depth, weights=None, mask=None, return_counts=False):
        if torch.is_tensor(depth) and depth.dim() == 4 and (depth.shape[0], tuple(depth.shape[2:])) != (self.B, self.size):
            raise ValueError(f"{PREFIX}: Smoother was built for B={self.B}, {self.size}; got B={depth.shape[0]}, "
                             f"{tuple(depth.shape[2:])}")
        return smoothness_loss(depth, weights, self.order, mask, return_counts, out=self._out)


class EdgeWeights:
    """A batch-dict stage for data.DevicePrefetcher(..., ingest=EdgeWeights(chain=Ingest())): chain
    (frames.Ingest(), ...) is called on the batch first, so that batch[rgb_key] is fp32 on the device;
    then batch[out_key] = edge_weights(batch[rgb_key], alpha), made on the prefetch stream beside the
    loader. Every other entry is passed through untouched."""

    def __init__(self, alpha=1.0 / 255.0, chain=None, rgb_key="rgb", out_key="edge_w"):
        if not 0.0 <= float(alpha) < float("inf"):
            raise ValueError(f"{PREFIX}: alpha = {alpha} must be finite and >= 0")
        self.alpha, self.chain, self.rgb_key, self.out_key = float(alpha), chain, rgb_key, out_key

    def __call__(self, batch):
        if self.chain is not None:
            batch = self.chain(batch)
        batch = dict(batch)
        batch[self.out_key] = edge_weights(batch[self.rgb_key], self.alpha)
        return batch
