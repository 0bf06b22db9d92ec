"""Sparsification curves and AUSE of a confidence plane on device: does the confidence that normalized
convolution propagates beside the depth say where the depth is wrong?

Remove the least confident valid pixels step by step and watch the error of the rest fall; compare with
the oracle that removes the largest errors first (Ilg et al. 2018; Eldesokey et al. 2020 for this
network family). One libnconv call (nconv_depth_sparsification, csrc/sparsification.hip: twelve launches,
no host synchronisation) sorts the valid pixels of every image twice, by confidence and by error, with a
segmented stable radix sort, and returns for j = 0 .. J-1 the count, sum |e| and sum e^2 of the pixels
kept after removing the first floor(j n / J).

Ties are broken by the pixel number row * W + col, ascending, in both rankings: a propagated confidence
ties a lot (whole regions are 0 or saturated), and with this rule the same input gives the same curve
bits on every run. A NaN confidence is removed first. include/nconv.h states the full definition.

  sparsification         the (B, 2, J, 3) float64 curves of one batch (and the removal order on request);
                         device only: there is no PyTorch path
  SparsificationCurves   a running mean over images of the normalised curves; update() never
                         synchronises and is capturable in a hipGraph; compute() is the one
                         synchronisation and returns the curves and the two AUSE figures
"""
import ctypes

import torch

from . import _views
from .metrics import _bounds

PREFIX = "sparsification"
MAX_STEPS = 1024


def _operand(x, what):
    """(B, H, W, image stride, row stride) of an fp32 device operand."""
    if torch.is_tensor(x):  # a tensor's device is checked before its dtype
        _views.on_device(x, what, PREFIX, "the curves are computed by libnconv")
    _views.require_tensor(x, what, (torch.float32,), PREFIX, expected="float32")
    return _views.plane_view(x, what, PREFIX)


def _steps(steps):
    if isinstance(steps, bool) or not isinstance(steps, int):
        raise TypeError(f"{PREFIX}: steps must be an int, got {type(steps).__name__}")
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"{PREFIX}: steps must be in [1, {MAX_STEPS}], got {steps}")
    return steps


def _launch(pred, gt, conf, steps, bounds, uncertainty, curves, order, ws):
    """One nconv_depth_sparsification call; curves / order / ws: tensors to reuse, or None (order False:
    not wanted). Returns (curves, order or None, ws)."""
    from . import _lib
    B, H, W, pbs, prs = _operand(pred, "pred")
    for x, what in ((gt, "gt"), (conf, "conf")):
        if _operand(x, what)[:3] != (B, H, W):
            raise ValueError(f"{PREFIX}: pred {tuple(pred.shape)} and {what} {tuple(x.shape)} differ")
        if x.device != pred.device:
            raise RuntimeError(f"{PREFIX}: pred on {pred.device}, {what} on {x.device}")
    _, _, _, gbs, grs = _operand(gt, "gt")
    _, _, _, cbs, crs = _operand(conf, "conf")
    lib = _lib.lib()
    nbytes = lib.nconv_depth_sparsification_workspace_bytes(B, H, W, steps)
    if nbytes == 0:
        raise ValueError(f"{PREFIX}: a batch of {B} x {H} x {W} is too large (B * H * W must be below 2^31)")
    dev = pred.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if curves is None:
        curves = torch.empty((B, 2, steps, 3), dtype=torch.float64, device=dev)
    if order is True:
        order = torch.empty((B, 2, H * W), dtype=torch.int32, device=dev)
    elif order is False:
        order = None
    d = _lib.NconvDepthSparsification()
    d.B, d.H, d.W, d.steps = B, H, W, steps
    d.pred, d.pred_image_stride, d.pred_row_stride = pred.data_ptr(), pbs, prs
    d.gt, d.gt_image_stride, d.gt_row_stride = gt.data_ptr(), gbs, grs
    d.conf, d.conf_image_stride, d.conf_row_stride = conf.data_ptr(), cbs, crs
    d.gt_min, d.gt_max, d.clamp_lo, d.clamp_hi = bounds
    d.uncertainty = 1 if uncertainty else 0
    d.curves = curves.data_ptr()
    d.order = None if order is None else order.data_ptr()
    rc = lib.nconv_depth_sparsification(ctypes.byref(d), _lib.ptr(ws), nbytes, _lib.stream_handle(dev))
    _lib.check(rc, "nconv_depth_sparsification")
    return curves, order, ws


def sparsification(pred, gt, conf, steps=100, gt_min=0.0, gt_max=0.0, clamp=(0.0, 0.0), uncertainty=False,
                   return_order=False):
    """The sparsification curves of each image of a batch: (B, 2, steps, 3) float64 on pred's device,
    [b][0] ranked by conf and [b][1] by the oracle, each point {pixels kept, sum |e|, sum e^2}.

    pred, gt, conf: fp32 device tensors of the same shape, (H, W), (1, H, W) or (B, 1, H, W), rows of
    unit stride (cropped views are fine). gt_min / gt_max: validity window of the target; clamp =
    (lo, hi): the prediction is clamped into it first; None or 0 = no bound. uncertainty: conf is an
    uncertainty (the largest is removed first). return_order: also return the (B, 2, H * W) int32 removal
    order: the pixel numbers row * W + col of the valid pixels, then -1."""
    curves, order, _ = _launch(pred, gt, conf, _steps(steps), _bounds(gt_min, gt_max, clamp), uncertainty,
                               None, bool(return_order), None)
    return (curves, order) if return_order else curves


class SparsificationCurves:
    """Running sparsification curves over the images of a validation set.

        s = SparsificationCurves(steps=100, gt_max=80.0)
        for batch in loader:
            d, c = model.forward_with_confidence(batch["depth"])
            s.update(d, batch["gt"], c)                                       # no synchronisation
        print(s.compute()["ause_rmse"])                                       # the one synchronisation

    Per image the MAE curve (sum |e| / kept) and the RMSE curve (sqrt(sum e^2 / kept)) of either ranking
    are divided by their own value at j = 0, so every curve starts at 1; an image without a valid pixel is
    left out, and an image whose error at j = 0 is 0 contributes a curve of zeros. state is the (2, 2, J)
    float64 sum over images of those curves ([figure][ranking][j]); images counts the images."""

    def __init__(self, steps=100, gt_min=None, gt_max=80.0, clamp=None, uncertainty=False, device=None):
        self.steps = _steps(steps)
        self.bounds = _bounds(gt_min, gt_max, clamp)
        self.uncertainty = bool(uncertainty)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.state = torch.zeros((2, 2, self.steps), dtype=torch.float64, device=device)
        self.images = torch.zeros((), dtype=torch.float64, device=device)
        self._buffers = {}  # (device, B, H, W) -> (curves, workspace): an update allocates nothing twice

    def update(self, pred, gt, conf):
        """state += the normalised curves of this batch (nconv_depth_sparsification on the current stream)."""
        key = (pred.device, tuple(pred.shape)) if torch.is_tensor(pred) else None
        curves, ws = self._buffers.get(key, (None, None))
        curves, _, ws = _launch(pred, gt, conf, self.steps, self.bounds, self.uncertainty, curves, False, ws)
        self._buffers[key] = (curves, ws)
        self.state += self.normalised(curves).sum(1)
        self.images += (curves[:, 0, 0, 0] > 0).sum()
        return self

    @staticmethod
    def normalised(curves):
        """(2, B, 2, J): the MAE and RMSE curves of (B, 2, J, 3) raw curves, each over its own j = 0
        value; zeros where that value or the image's valid count is 0."""
        n = curves[..., 0]
        kept = torch.where(n > 0, n, torch.ones_like(n))
        fig = torch.stack((curves[..., 1] / kept, (curves[..., 2] / kept).sqrt()))
        first = fig[..., :1]
        ok = (first > 0) & (n[None, ..., :1] > 0)
        return torch.where(ok, fig / torch.where(ok, first, torch.ones_like(first)), torch.zeros_like(fig))

    def reset(self):
        self.state.zero_()
        self.images.zero_()
        return self

    def compute(self):
        """{fraction, mae_conf, mae_oracle, rmse_conf, rmse_oracle: (J,) float64 CPU tensors; ause_mae,
        ause_rmse: floats, the plain mean over j of (confidence curve - oracle curve), not a trapezoid;
        images: int}. nan where no image had a valid pixel."""
        state, images = self.state.cpu(), float(self.images.cpu())
        mean = state / images if images > 0 else torch.full_like(state, float("nan"))
        out = {"fraction": torch.arange(self.steps, dtype=torch.float64) / self.steps,
               "mae_conf": mean[0, 0], "mae_oracle": mean[0, 1],
               "rmse_conf": mean[1, 0], "rmse_oracle": mean[1, 1]}
        out["ause_mae"] = float((mean[0, 0] - mean[0, 1]).mean())
        out["ause_rmse"] = float((mean[1, 0] - mean[1, 1]).mean())
        out["images"] = int(images)
        return out
