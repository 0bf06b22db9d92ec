"""Timing record of the cross-view depth consistency check with fusion (consistency.DepthFuser, two sources) and
of the geometry-consistency loss forward + backward (consistency.GeometryConsistency), each against the same thing
composed from torch ops and against a plain copy of the bytes it must touch, on the same device tensors in the
same process (tools/minreproj_bench.py's setup and conventions: B = 8, 352 x 1216, the previous and the next frame
at 1 m of forward motion each way; HIP events around each call, 10 warm-up calls, the median of 150 calls taken as
three alternating blocks of 50 per variant; each variant also as a hipGraph of 20 back-to-back calls, per call =
replay / 20).

    python tools/consistency_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

  check_fused   DepthFuser(S=2): nconv_depth_consistency, one launch; fused and count written
  check_torch   per source the projection, F.grid_sample of the depth and of its validity, the way back by a
                matrix product, the thresholds, and the masked mean, all from torch ops
  check_copy    one copy of 8.5 B/px: 17 B/px moved against the 4 (depth) + 8 (two source planes, each tap's cache
                line shared by its neighbours) bytes read and the 4 + 1 bytes of fused and count written
  loss_fused    GeometryConsistency + backward: nconv_geo_consistency_loss_fwd (two launches) and _bwd (one)
  loss_torch    the projection, F.grid_sample, the masked mean of |c - zs| / (c + zs) and autograd
  loss_copy     one copy of 10 B/px: 20 B/px moved against the 4 + 4 bytes read by the forward and again by the
                backward and the 4 bytes of g_depth written
The torch compositions differ from ours in the last bits and wherever a decision falls the other way, so they are
compared by the share of pixels that differ. One run each: a record, not a gate."""
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

PX_TOL, REL_TOL, Z_MIN = 1.0, 0.01, 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    mod = nconv_pkg.load()
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(B, 1, 6, 20, generator=g) * 55 + 5
    depth0 = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).to(dev)
    k = torch.tensor([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]], device=dev)
    srcs, ms, mbs = [], [], []
    for yaw, tz in ((0.01, -1.0), (-0.01, 1.0)):  # the car moved 1 m forward / was 1 m behind
        pose = torch.tensor([[np.cos(yaw), 0.0, np.sin(yaw), 0.05], [0.0, 1.0, 0.0, -0.02],
                             [-np.sin(yaw), 0.0, np.cos(yaw), tz]], device=dev)
        ms.append(mod.warp_projection(k, pose).expand(B, 3, 4).contiguous())
        mbs.append(mod.warp_projection(k, mod.inverse_pose(pose)).expand(B, 3, 4).contiguous())
        # the neighbour's depth: the same smooth scene moved by tz, with its own percent of relief
        srcs.append((depth0 + tz) * (1 + 0.02 * (torch.rand(B, 1, H, W, generator=g).to(dev) - 0.5)))
    ks = [k, k]
    fuser = mod.DepthFuser((H, W), S=2, B=B, device=dev, px_tol=PX_TOL, rel_tol=REL_TOL)
    geo = mod.GeometryConsistency((H, W), B=B, device=dev)
    seed = torch.ones((), device=dev)
    jj = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ii = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)

    def leaf():
        return depth0.detach().requires_grad_(True)  # a fresh leaf per call (warp_bench.py says why)

    def project(z, m):
        x = (jj - k[0, 2]) * z / k[0, 0]
        y = (ii - k[1, 2]) * z / k[1, 1]
        mm = m.view(B, 3, 4, 1, 1)
        a_, b_, c_ = (mm[:, r, 0] * x + mm[:, r, 1] * y + mm[:, r, 2] * z + mm[:, r, 3] for r in range(3))
        u, v = a_ / c_, b_ / c_
        valid = (z > Z_MIN) & (c_ > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        grid = torch.stack((2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1), dim=-1)
        return u, v, c_, valid, torch.where(valid[..., None], grid, torch.zeros_like(grid))

    def sample(src, grid):
        zs = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
        tv = F.grid_sample((src > Z_MIN).float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
        return zs, tv > 0.999

    def check_fused():
        return fuser(depth0, k, srcs, ks, ms, mbs)

    def check_torch():
        with torch.no_grad():
            z = depth0[:, 0]
            acc, n = z.clone(), torch.zeros_like(z)
            for src, m, mb in zip(srcs, ms, mbs):
                u, v, _, valid, grid = project(z, m)
                zs, tv = sample(src, grid)
                xs, ys = (u - k[0, 2]) * zs / k[0, 0], (v - k[1, 2]) * zs / k[1, 1]
                mm = mb.view(B, 3, 4, 1, 1)
                a2, b2, c2 = (mm[:, r, 0] * xs + mm[:, r, 1] * ys + mm[:, r, 2] * zs + mm[:, r, 3] for r in range(3))
                d2 = (a2 / c2 - jj) ** 2 + (b2 / c2 - ii) ** 2
                cons = valid & tv & (c2 > 0) & (d2 <= PX_TOL * PX_TOL) & ((c2 - z).abs() <= REL_TOL * z)
                acc = torch.where(cons, acc + c2, acc)
                n = n + cons
            fused = torch.where((z > Z_MIN) & (n >= 1), acc / (n + 1), torch.zeros_like(acc))
            return fused[:, None], n.to(torch.uint8)

    def loss_fused():
        depth = leaf()
        return torch.autograd.grad(geo(depth, k, srcs[0], ms[0]), depth, seed)[0]

    def loss_torch():
        depth = leaf()
        _, _, c, valid, grid = project(depth[:, 0], ms[0])
        zs, tv = sample(srcs[0], grid)
        ok = valid & tv
        diff = torch.where(ok, (c - zs).abs() / (c + zs), torch.zeros_like(c))
        return torch.autograd.grad(diff.sum() / ok.sum().clamp_min(1), depth, seed)[0]

    npx = B * H * W
    bytes_check, bytes_loss = torch.empty(npx * 17 // 2, dtype=torch.uint8, device=dev), \
        torch.empty(npx * 10, dtype=torch.uint8, device=dev)
    out_check, out_loss = torch.empty_like(bytes_check), torch.empty_like(bytes_loss)

    def check_copy():
        return out_check.copy_(bytes_check)

    def loss_copy():
        return out_loss.copy_(bytes_loss)

    fused, count = (t.clone() for t in check_fused())
    fused_t, count_t = check_torch()
    ours = loss_fused().clone()
    scale = float(ours.abs().max())
    differ_g = float(((ours - loss_torch()).abs() > 1e-3 * scale).float().mean())
    _, n_g = geo(depth0, k, srcs[0], ms[0], return_count=True)
    variants = {"check_fused": check_fused, "check_torch": check_torch, "check_copy": check_copy,
                "loss_fused": loss_fused, "loss_torch": loss_torch, "loss_copy": loss_copy}
    res = measure(variants, graphable=tuple(variants))
    for q, base in (("check_torch", "check_fused"), ("check_copy", "check_fused"), ("loss_torch", "loss_fused"),
                    ("loss_copy", "loss_fused")):
        res[q]["graph_over_" + base + "_graph"] = round(res[q]["graph_us"] / res[base]["graph_us"], 2)
    record = {"shape": [B, H, W], "sources": 2, "px_tol": PX_TOL, "rel_tol": REL_TOL,
              "consistent_share": [round(float((count >= n).float().mean()), 4) for n in (1, 2)],
              "counted_share": round(int(n_g) / npx, 4),
              "torch_count_share_differing": float(f"{float((count != count_t).float().mean()):.3g}"),
              "torch_gradient_share_differing": float(f"{differ_g:.3g}"), **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
