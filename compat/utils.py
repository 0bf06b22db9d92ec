"""Drop-in for the reference's utils.py (`from utils import *` in train_step1.py / train_step2.py):
the training glue of nconv_amd.train (fused loss kernels on device tensors, the reference's
optimizer factory and checkpoint format) and the validation loops, plus the KITTI loader names
that utils.py re-exports (utils.py:1).

save_depth writes the min-max normalised depth as an 8-bit PNG. The reference colours it with
OpenCV's INFERNO map (utils.py:12-16); a device tensor is coloured the same way on the device
(nconv_amd.visualize.colorize: matplotlib's inferno colours times 255, rounded, which is how OpenCV's
table is defined; OpenCV is not a dependency, so parity with cv2 itself is not pinned by a test). A
host array without a cmap is written in grayscale, as it always was.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F  # noqa: F401  (the reference's namespace)
from torch import nn  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nconv_pkg  # noqa: E402

_m = nconv_pkg.load()
from dataset.kittiloader import *  # noqa: E402,F401,F403

calculate_loss = _m.train.calculate_loss
calculate_loss_multi_resolution = _m.train.calculate_loss_multi_resolution
gradient_loss = _m.train.gradient_loss
gradient_x = _m.train.gradient_x
gradient_y = _m.train.gradient_y
get_optimizer = _m.train.get_optimizer
save_checkpoint = _m.train.save_checkpoint
DepthMetrics = _m.metrics.DepthMetrics
depth_metric_sums = _m.metrics.depth_metric_sums
SparsificationCurves = _m.SparsificationCurves
confidence_loss = _m.train.confidence_loss
ConfidenceLoss = _m.train.ConfidenceLoss


def save_depth(depth_data, path, cmap=None):
    """A device tensor ((H, W), (1, H, W) or (1, 1, H, W)): coloured on the device with the reference's
    INFERNO map (or `cmap`, a name of nconv_amd.COLORMAPS) by visualize.colorize and written in R, G, B
    order, which is the picture cv2.imwrite makes of the reference's BGR array. A host array with a cmap
    name: the same rules in numpy. A host array without one: the grayscale image, as before."""
    if torch.is_tensor(depth_data) and depth_data.is_cuda:
        img = _m.visualize.colorize(depth_data.detach().float(), cmap="inferno" if cmap is None else cmap)
        if img.shape[0] != 1:
            raise ValueError(f"save_depth: one image per file, got a batch of {img.shape[0]}")
        return _m.visualize.write_png8(path, img[0])
    if cmap is not None:
        a = depth_data.detach().numpy() if torch.is_tensor(depth_data) else np.asarray(depth_data)
        a = a.reshape(a.shape[-2:]) if a.ndim > 2 and a.size == a.shape[-2] * a.shape[-1] else a
        return _m.visualize.write_png8(path, _m.visualize.colorize_host(a, cmap))
    d = np.asarray(depth_data, dtype=np.float64)
    lo, hi = float(d.min()), float(d.max())
    img = np.zeros(d.shape, np.uint8) if hi <= lo else ((d - lo) / (hi - lo) * 255.0 + 0.5).astype(np.uint8)
    from PIL import Image
    Image.fromarray(img).save(path)


def get_performance(model, val_loader, device_str, use_gradient_loss):
    """Mean validation loss of a step-1 model on element [0] of each batch (utils.py:18-40)."""
    device = torch.device(device_str if device_str == "cuda" and torch.cuda.is_available() else "cpu")
    model.to(device)
    model.eval()
    with torch.no_grad():
        losses = []
        for data in val_loader:
            depth, gt = data["depth"].to(device), data["gt"].to(device)
            est = model(depth)
            losses.append(calculate_loss(est[0, :, :, :], gt[0, :, :, :], use_gradient_loss).item())
    return sum(losses) / len(losses)


def get_performance_confidence(model, val_loader, device_str, lam):
    """Mean validation confidence loss (confidence_loss, smooth-L1, beta 1) of a step-1 model on element
    [0] of each batch, the loop of get_performance on model.forward_with_confidence. Device only: the
    loss and the confidence output are device kernels."""
    device = torch.device(device_str)
    model.to(device)
    model.eval()
    with torch.no_grad():
        losses = []
        for data in val_loader:
            depth, gt = data["depth"].to(device), data["gt"].to(device)
            est, conf = model.forward_with_confidence(depth)
            losses.append(confidence_loss(est[0, :, :, :], gt[0, :, :, :], conf[0, :, :, :], lam).item())
    return sum(losses) / len(losses)


def get_performance_multi_resolution(model, val_loader, device_str, use_gradient_loss):
    """Mean multi-resolution validation loss of a guided model (utils.py:74-93)."""
    device = torch.device(device_str if device_str == "cuda" and torch.cuda.is_available() else "cpu")
    model.to(device)
    losses = []
    for data in val_loader:
        rgb, depth, gt = data["rgb"].to(device), data["depth"].to(device), data["gt"].to(device)
        est, _ = model(rgb, depth, rgb, depth)
        losses.append(calculate_loss_multi_resolution(est, gt, use_gradient_loss).item())
    return sum(losses) / len(losses)


def get_metrics(model, val_loader, device_str, unit_m=1.0, **bounds):
    """Depth-completion figures (nconv_amd.metrics.DepthMetrics.compute: MAE, RMSE, iMAE, iRMSE, REL,
    delta < 1.25^k, ...) of a step-1 model over every image of every batch; the loop of
    get_performance with one fused metrics call per batch and one synchronisation at the end.
    bounds: gt_min, gt_max, clamp=(lo, hi); unit_m: metres per unit of the depth tensors."""
    device = torch.device(device_str if device_str == "cuda" and torch.cuda.is_available() else "cpu")
    model.to(device)
    model.eval()
    metrics = DepthMetrics(device=device, **bounds)
    with torch.no_grad():
        for data in val_loader:
            depth, gt = data["depth"].to(device), data["gt"].to(device)
            metrics.update(model(depth), gt)
    return metrics.compute(unit_m)


def get_sparsification(model, val_loader, device_str, steps=100, **bounds):
    """Sparsification curves and AUSE (nconv_amd.SparsificationCurves.compute) of a step-1 model's output
    confidence over every image of every batch: get_metrics's loop on model.forward_with_confidence, one
    fused call per batch and one synchronisation at the end. bounds: gt_min, gt_max, clamp=(lo, hi)."""
    device = torch.device(device_str if device_str == "cuda" and torch.cuda.is_available() else "cpu")
    model.to(device)
    model.eval()
    curves = SparsificationCurves(steps=steps, device=device, **bounds)
    with torch.no_grad():
        for data in val_loader:
            depth, gt = data["depth"].to(device), data["gt"].to(device)
            pred, conf = model.forward_with_confidence(depth)
            curves.update(pred, gt, conf)
    return curves.compute()


def get_metrics_multi_resolution(model, val_loader, device_str, unit_m=1.0, **bounds):
    """get_metrics for a guided model: the call of get_performance_multi_resolution, the finest scale
    (est[3]) scored against gt."""
    device = torch.device(device_str if device_str == "cuda" and torch.cuda.is_available() else "cpu")
    model.to(device)
    metrics = DepthMetrics(device=device, **bounds)
    with torch.no_grad():
        for data in val_loader:
            rgb, depth, gt = data["rgb"].to(device), data["depth"].to(device), data["gt"].to(device)
            est, _ = model(rgb, depth, rgb, depth)
            fine, gt = est[3], gt[0:1]  # the model returns element [0] of the batch, as the loss scores it
            if fine.shape[-2:] != gt.shape[-2:]:
                fine = F.interpolate(fine, size=gt.shape[-2:], mode="bilinear", align_corners=False)
            metrics.update(fine, gt)
    return metrics.compute(unit_m)
