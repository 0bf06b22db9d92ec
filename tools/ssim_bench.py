"""Timing record of the fused SSIM + L1 photometric loss (warp.photometric_ssim_loss, forward + backward)
against the same term composed from torch ops, against view_warp + torch's SSIM, against the L1 loss alone
and against a plain copy of the planes it must touch, on the same device tensors in the same process
(tools/warp_bench.py's setup and conventions: B = 8, C = 3, 352 x 1216, a 1 m forward motion; HIP events
around each call, 10 warm-up calls, the median of 150 calls taken as three alternating blocks of 50 per
variant; each variant also as a hipGraph of 20 back-to-back calls, per call = replay / 20).

    python tools/ssim_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

  ssim_fused     ViewWarper(alpha=0.85).loss + backward: nconv_photo_ssim_loss_fwd (two launches) and _bwd (one)
  ssim_unfused   ViewWarper() + torch's SSIM (F.avg_pool2d x 5, products, a division, the window-validity
                 product, two masked means) + backward through autograd and nconv_view_warp_bwd
  ssim_torch     the projection, F.grid_sample(align_corners=True) and the same SSIM, all from torch ops
  photo_fused    the L1 loss alone (nconv_photo_loss_*): what the SSIM term costs on top of it
  copy_floor     one copy of a (B, 7, H, W) fp32 tensor (warp_bench.py's: 56 B/px against the 60 B/px the
                 fused pair must move; the halo's re-reads are served by the cache)
The torch compositions' gradients differ from ours in the last bits, so they are compared by their largest
difference relative to the gradient's scale. A record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nconv_pkg  # noqa: E402
from pointcloud_bench import measure  # noqa: E402

ALPHA, R = 0.85, 255.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    mod = nconv_pkg.load()
    dev = torch.device("cuda:0")
    B, H, W, C = a.batch, a.height, a.width, 3
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(B, 1, 6, 20, generator=g) * 55 + 5
    depth0 = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).to(dev)
    tgt = (torch.rand(B, C, H, W, generator=g) * R).to(dev)
    src = (torch.rand(B, C, H, W, generator=g) * R).to(dev)
    k = torch.tensor([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]], device=dev)
    yaw = 0.01
    pose = torch.tensor([[np.cos(yaw), 0.0, np.sin(yaw), 0.05], [0.0, 1.0, 0.0, -0.02],
                         [-np.sin(yaw), 0.0, np.cos(yaw), -1.0]], device=dev)  # the car moved 1 m forward
    m = mod.warp_projection(k, pose).expand(B, 3, 4).contiguous()
    vw = mod.ViewWarper((H, W), (H, W), B=B, C=C, device=dev)
    vs = mod.ViewWarper((H, W), (H, W), B=B, C=C, device=dev, alpha=ALPHA, data_range=R)
    seed = torch.ones((), device=dev)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2

    def leaf():
        return depth0.detach().requires_grad_(True)  # a fresh leaf per call (warp_bench.py says why)

    def loss_of(warped, vf):
        pool = lambda t: F.avg_pool2d(t, 3, 1)  # noqa: E731
        mu_x, mu_y = pool(warped), pool(tgt)
        s_x = pool(warped * warped) - mu_x * mu_x
        s_y = pool(tgt * tgt) - mu_y * mu_y
        s_xy = pool(warped * tgt) - mu_x * mu_y
        ssim = ((2 * mu_x * mu_y + c1) * (2 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_x + s_y + c2))
        wv = -F.max_pool2d(-vf, 3, 1)
        lw = (torch.clamp((1 - ssim) / 2, 0, 1) * wv).sum() / (C * wv.sum().clamp_min(1.0))
        lv = ((warped - tgt).abs() * vf).sum() / (C * vf.sum().clamp_min(1.0))
        return ALPHA * lw + (1 - ALPHA) * lv

    def ssim_fused():
        depth = leaf()
        return torch.autograd.grad(vs.loss(depth, k, tgt, src, m), depth, seed)[0]

    def photo_fused():
        depth = leaf()
        return torch.autograd.grad(vw.loss(depth, k, tgt, src, m), depth, seed)[0]

    def ssim_unfused():
        depth = leaf()
        warped, valid = vw(depth, k, src, m, return_valid=True)
        return torch.autograd.grad(loss_of(warped, valid[:, None].float()), depth, seed)[0]

    jj = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ii = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    mm = m.view(B, 3, 4, 1, 1)

    def ssim_torch():
        depth = leaf()
        z = depth[:, 0]
        x = (jj - k[0, 2]) * z / k[0, 0]
        y = (ii - k[1, 2]) * z / k[1, 1]
        a_, b_, c_ = (mm[:, r, 0] * x + mm[:, r, 1] * y + mm[:, r, 2] * z + mm[:, r, 3] for r in range(3))
        u, v = a_ / c_, b_ / c_
        valid = (z > 0) & (c_ > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        grid = torch.stack((2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1), dim=-1)
        grid = torch.where(valid[..., None], grid, torch.zeros_like(grid))
        vf = valid[:, None].float()
        warped = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * vf
        return torch.autograd.grad(loss_of(warped, vf), depth, seed)[0]

    planes = torch.rand(B, 7, H, W, generator=g).to(dev)
    planes_out = torch.empty_like(planes)

    def copy_floor():
        return planes_out.copy_(planes)

    ours = ssim_fused().clone()
    _, n_v, n_w = mod.photometric_ssim_loss(depth0, k, tgt, src, m, alpha=ALPHA, data_range=R, return_counts=True)
    scale = float(ours.abs().max())
    diff_u = float((ours - ssim_unfused()).abs().max()) / scale
    diff_t = float((ours - ssim_torch()).abs().max()) / scale
    variants = {"ssim_fused": ssim_fused, "ssim_unfused": ssim_unfused, "ssim_torch": ssim_torch,
                "photo_fused": photo_fused, "copy_floor": copy_floor}
    res = measure(variants, graphable=tuple(variants))
    for q in ("ssim_unfused", "ssim_torch", "photo_fused", "copy_floor"):
        res[q]["graph_over_ssim_fused_graph"] = round(res[q]["graph_us"] / res["ssim_fused"]["graph_us"], 2)
    record = {"shape": [B, C, H, W], "alpha": ALPHA, "data_range": R, "valid_share": round(int(n_v) / (B * H * W), 4),
              "window_share": round(int(n_w) / (B * H * W), 4),
              "unfused_gradient_max_diff_over_scale": float(f"{diff_u:.3g}"),
              "torch_gradient_max_diff_over_scale": float(f"{diff_t:.3g}"), **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
