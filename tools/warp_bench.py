"""Timing record of the fused photometric loss (warp.photometric_loss, forward + backward) against the
same term composed from torch ops and against a plain copy of the planes it must touch, on the same
device tensors in the same process (DESIGN.md section 5's conventions, as tools/pointcloud_bench.py: HIP
events around each call, 10 warm-up calls, the median of 150 calls taken as three alternating blocks of
50 per variant; each variant also as a hipGraph of 20 back-to-back calls, per call = replay / 20, which
takes the host's launch gap out).

    python tools/warp_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

The frames are seeded and synthetic: a smoothly varying depth of 5 - 60 m, KITTI's camera-2 intrinsics, a
forward motion of 1 m with a small yaw (about ten pixels of flow at the median, growing towards the border),
C = 3.
  photo_fused    ViewWarper.loss + backward: nconv_photo_loss_fwd (two launches) and _bwd (one)
  photo_unfused  ViewWarper() + torch's masked L1 mean + backward through nconv_view_warp_bwd
  photo_torch    meshgrid (precomputed), the elementwise projection, F.grid_sample(align_corners=True), a
                 masked mean, and autograd's backward of all of it with respect to the depth
  copy_floor     one copy of a (B, 7, H, W) fp32 tensor: 28 B/px read and 28 B/px written, the 56 B/px
                 nearest to what the fused pair must move (depth 4 + tgt 12 + src 12 B/px read by the
                 forward and again by the backward, 4 B/px of g_depth written: 60 B/px)
The torch composition's gradient differs from ours in the last bits (it fuses nothing and sums in another
order), so the two are compared by their largest difference relative to the gradient's scale. The roof
is 8 TB/s. A record, not a gate."""
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
from frames_bench import HBM_BPS  # noqa: E402
from pointcloud_bench import measure  # noqa: E402


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
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(B, 1, 6, 20, generator=g) * 55 + 5
    depth0 = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).to(dev)
    tgt = torch.rand(B, C, H, W, generator=g).to(dev)
    src = torch.rand(B, C, H, W, generator=g).to(dev)
    k = torch.tensor([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]], device=dev)
    yaw = 0.01
    pose = torch.tensor([[np.cos(yaw), 0.0, np.sin(yaw), 0.05], [0.0, 1.0, 0.0, -0.02],
                         [-np.sin(yaw), 0.0, np.cos(yaw), -1.0]], device=dev)  # the car moved 1 m forward
    m = mod.warp_projection(k, pose).expand(B, 3, 4).contiguous()
    vw = mod.ViewWarper((H, W), (H, W), B=B, C=C, device=dev)
    seed = torch.ones((), device=dev)

    def leaf():
        """The depth as a fresh leaf per call (a view: no launch). A leaf kept across calls keeps its
        AccumulateGrad node and the stream that node was made on, here the default stream of the eager
        blocks, and a backward under stream capture would then synchronise the capturing stream with it."""
        return depth0.detach().requires_grad_(True)

    def photo_fused():
        depth = leaf()
        return torch.autograd.grad(vw.loss(depth, k, tgt, src, m), depth, seed)[0]

    def photo_unfused():
        depth = leaf()
        warped, valid = vw(depth, k, src, m, return_valid=True)
        vf = valid[:, None].float()
        loss = ((warped - tgt).abs() * vf).sum() / (C * vf.sum().clamp_min(1.0))
        return torch.autograd.grad(loss, depth, seed)[0]

    jj = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ii = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    mm = m.view(B, 3, 4, 1, 1)

    def photo_torch():
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
        warped = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        loss = ((warped - tgt).abs() * vf).sum() / (C * vf.sum().clamp_min(1.0))
        return torch.autograd.grad(loss, depth, seed)[0]

    planes = torch.rand(B, 7, H, W, generator=g).to(dev)
    planes_out = torch.empty_like(planes)

    def copy_floor():
        return planes_out.copy_(planes)

    ours, theirs = photo_fused().clone(), photo_torch()
    n_v = int(vw.loss(depth0, k, tgt, src, m, return_valid_count=True)[1])
    scale = float(ours.abs().max())
    assert float((ours - photo_unfused()).abs().max()) <= 1e-5 * scale
    diff = float((ours - theirs).abs().max()) / scale
    flow = None
    with torch.no_grad():
        z = depth0[:, 0]
        x = (jj - k[0, 2]) * z / k[0, 0]
        c_ = mm[:, 2, 0] * x + mm[:, 2, 1] * ((ii - k[1, 2]) * z / k[1, 1]) + mm[:, 2, 2] * z + mm[:, 2, 3]
        u = (mm[:, 0, 0] * x + mm[:, 0, 1] * ((ii - k[1, 2]) * z / k[1, 1]) + mm[:, 0, 2] * z + mm[:, 0, 3]) / c_
        flow = float((u - jj).abs().median())
    variants = {"photo_fused": photo_fused, "photo_unfused": photo_unfused, "photo_torch": photo_torch,
                "copy_floor": copy_floor}
    res = measure(variants, graphable=tuple(variants))
    for q in ("photo_fused", "photo_unfused", "photo_torch"):
        res[q]["over_copy_floor_graph"] = round(res[q]["graph_us"] / res["copy_floor"]["graph_us"], 2)
    res["photo_fused"]["fraction_of_hbm_roof_at_60B_per_px"] = round(
        60 * px / (res["photo_fused"]["graph_us"] * 1e-6) / HBM_BPS, 3)
    res["photo_torch"]["torch_graph_over_fused_graph"] = round(res["photo_torch"]["graph_us"] / res["photo_fused"]["graph_us"], 2)
    res["photo_torch"]["torch_eager_over_fused_eager"] = round(res["photo_torch"]["eager_us"] / res["photo_fused"]["eager_us"], 2)
    record = {"shape": [B, C, H, W], "valid_share": round(n_v / px, 4), "median_flow_px": round(flow, 2),
              "torch_gradient_max_diff_over_scale": float(f"{diff:.3g}"), **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
