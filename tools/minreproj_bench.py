"""Timing record of the fused minimum-reprojection loss (warp.min_reprojection_loss, forward + backward, two
sources) with and without auto-masking, against two photometric_ssim_loss forward + backward calls on the same
inputs (the nearest thing the single-source entry points offer), against the same term composed from torch ops,
and against a plain copy of the bytes per pixel it must touch, on the same device tensors in the same process
(tools/ssim_bench.py's setup and conventions: B = 8, C = 3, 352 x 1216, the previous and the next frame at 1 m of
forward motion each way; HIP events around each call, 10 warm-up calls, the median of 150 calls taken as three
alternating blocks of 50 per variant; each variant also as a hipGraph of 20 back-to-back calls, per call =
replay / 20).

    python tools/minreproj_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

  min_fused_automask  MinReprojector(S=2) + backward: nconv_photo_min_loss_fwd (two launches) and _bwd (one)
  min_fused_plain     the same with automask=False (no identity pass)
  two_ssim_pairs      ViewWarper(alpha=0.85).loss + backward, once per source: two sums of two means, NOT a minimum
  min_torch           the projection, F.grid_sample, the SSIM and L1 error maps per source, torch.min over the
                      sources, the identity errors, the mask and autograd, all from torch ops
  copy_floor          one copy of a (B, 11, H, W) fp32 tensor: 88 B/px against the 4 (depth) + 12 (tgt) + 24
                      (two sources) bytes read by the forward and again by the backward, the winner byte
                      written and read, and the 4 bytes of g_depth written = 86 B/px (the halo's and the
                      identity pass's re-reads are served by the cache)
The torch composition's gradient differs from ours in the last bits and wherever its minimum or mask falls the
other way, so it is compared by the share of pixels that differ by more than 1e-3 of the gradient's scale. A
record, not a gate."""
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
    srcs = [(torch.rand(B, C, H, W, generator=g) * R).to(dev) for _ in range(2)]
    k = torch.tensor([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]], device=dev)
    ms = []
    for yaw, tz in ((0.01, -1.0), (-0.01, 1.0)):  # the car moved 1 m forward / was 1 m behind
        pose = torch.tensor([[np.cos(yaw), 0.0, np.sin(yaw), 0.05], [0.0, 1.0, 0.0, -0.02],
                             [-np.sin(yaw), 0.0, np.cos(yaw), tz]], device=dev)
        ms.append(mod.warp_projection(k, pose).expand(B, 3, 4).contiguous())
    ra = mod.MinReprojector((H, W), S=2, B=B, C=C, device=dev, alpha=ALPHA, data_range=R, automask=True)
    rp = mod.MinReprojector((H, W), S=2, B=B, C=C, device=dev, alpha=ALPHA, data_range=R, automask=False)
    vs = [mod.ViewWarper((H, W), (H, W), B=B, C=C, device=dev, alpha=ALPHA, data_range=R) for _ in range(2)]
    seed = torch.ones((), device=dev)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2

    def leaf():
        return depth0.detach().requires_grad_(True)  # a fresh leaf per call (warp_bench.py says why)

    def min_fused_automask():
        depth = leaf()
        return torch.autograd.grad(ra(depth, k, tgt, srcs, ms), depth, seed)[0]

    def min_fused_plain():
        depth = leaf()
        return torch.autograd.grad(rp(depth, k, tgt, srcs, ms), depth, seed)[0]

    def two_ssim_pairs():
        depth = leaf()
        loss = vs[0].loss(depth, k, tgt, srcs[0], ms[0]) + vs[1].loss(depth, k, tgt, srcs[1], ms[1])
        return torch.autograd.grad(loss, depth, seed)[0]

    jj = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ii = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    inner = torch.zeros(1, 1, H, W, device=dev)
    inner[..., 1:-1, 1:-1] = 1.0

    def error_map(x, vf):
        """(E (B, H, W), comparable (B, H, W) float) of one source: x the warped (or unwarped) frame."""
        pool = lambda t: F.avg_pool2d(t, 3, 1)  # noqa: E731
        mu_x, mu_y = pool(x), pool(tgt)
        s_x, s_y, s_xy = pool(x * x) - mu_x * mu_x, pool(tgt * tgt) - mu_y * mu_y, pool(x * tgt) - mu_x * mu_y
        ssim = ((2 * mu_x * mu_y + c1) * (2 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_x + s_y + c2))
        tw = F.pad(torch.clamp((1 - ssim) / 2, 0, 1).sum(1), (1, 1, 1, 1))
        wv = F.pad(-F.max_pool2d(-vf, 3, 1), (1, 1, 1, 1))[:, 0]
        return ALPHA * tw + (1 - ALPHA) * (x - tgt).abs().sum(1), wv

    def min_torch():
        depth = leaf()
        z = depth[:, 0]
        x = (jj - k[0, 2]) * z / k[0, 0]
        y = (ii - k[1, 2]) * z / k[1, 1]
        big = torch.full_like(z, float("inf"))
        Es, Is = [], []
        for src, m in zip(srcs, ms):
            mm = m.view(B, 3, 4, 1, 1)
            a_, b_, c_ = (mm[:, r, 0] * x + mm[:, r, 1] * y + mm[:, r, 2] * z + mm[:, r, 3] for r in range(3))
            u, v = a_ / c_, b_ / c_
            valid = (z > 0) & (c_ > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            grid = torch.stack((2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1), dim=-1)
            grid = torch.where(valid[..., None], grid, torch.zeros_like(grid))
            vf = valid[:, None].float()
            warped = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * vf
            E, wv = error_map(warped, vf)
            Es.append(torch.where(wv > 0.5, E, big))
            I, _ = error_map(src, inner.expand(B, 1, H, W))
            Is.append(I)
        best = torch.min(Es[0], Es[1])
        has = torch.isfinite(best)
        kept = has & ~(torch.min(Is[0], Is[1]) <= best)
        loss = torch.where(kept, best, torch.zeros_like(best)).sum() / (C * has.sum().clamp_min(1))
        return torch.autograd.grad(loss, depth, seed)[0]

    planes = torch.rand(B, 11, H, W, generator=g).to(dev)
    planes_out = torch.empty_like(planes)

    def copy_floor():
        return planes_out.copy_(planes)

    ours = min_fused_automask().clone()
    _, n_c, n_m = mod.min_reprojection_loss(depth0, k, tgt, srcs, ms, alpha=ALPHA, data_range=R, return_counts=True)
    scale = float(ours.abs().max())
    differ = float(((ours - min_torch()).abs() > 1e-3 * scale).float().mean())
    variants = {"min_fused_automask": min_fused_automask, "min_fused_plain": min_fused_plain,
                "two_ssim_pairs": two_ssim_pairs, "min_torch": min_torch, "copy_floor": copy_floor}
    res = measure(variants, graphable=tuple(variants))
    for q in ("min_fused_plain", "two_ssim_pairs", "min_torch", "copy_floor"):
        res[q]["graph_over_min_fused_automask_graph"] = round(
            res[q]["graph_us"] / res["min_fused_automask"]["graph_us"], 2)
    record = {"shape": [B, C, H, W], "sources": 2, "alpha": ALPHA, "data_range": R,
              "winner_share": round(int(n_c) / (B * H * W), 4), "masked_share": round(int(n_m) / (B * H * W), 4),
              "torch_gradient_share_differing": float(f"{differ:.3g}"), **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
