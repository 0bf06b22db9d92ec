"""Timing record of the fused smoothness loss (smooth.smoothness_loss, forward + backward, both orders,
with and without edge weights) and of smooth.edge_weights against the same terms composed from torch ops
with autograd and against a plain copy of the bytes each must touch, on the same device tensors in the
same process (tools/warp_bench.py's conventions: HIP events around each call, 10 warm-up calls, the median
of 150 calls taken as three alternating blocks of 50 per variant; each variant also as a hipGraph of 20
back-to-back calls, per call = replay / 20, which takes the host's launch gap out).

    python tools/smooth_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

The frames are seeded and synthetic: a smoothly varying depth of 5 - 60 m with a little noise, a random
8-bit-valued frame, alpha = 1 / 255.
  smooth_o<k>[_w]        Smoother + backward: nconv_smooth_loss_fwd (two launches) and _bwd (one)
  smooth_o<k>[_w]_torch  slices, abs, (minimum,) multiply, two means, and autograd's backward
  edge_w / edge_w_torch  nconv_edge_weights (one launch) / slices, abs, mean, exp, two pads
  copy_<n>B              one copy that reads and writes n B/px in all: what the fused calls must move --
                         12 B/px without weights (depth read by the forward and by the backward, g_depth
                         written), 28 B/px with them (both weight planes read twice), 20 B/px for the edge
                         weights (three channels read, two planes written)
The torch gradient differs from ours in the last bits (another order of the same sums), so the two are
compared by their largest difference relative to the gradient's scale. A record, not a gate."""
import argparse
import json
import os
import sys

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
    B, H, W = a.batch, a.height, a.width
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(B, 1, 6, 20, generator=g) * 55 + 5
    depth0 = (F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
              + torch.rand(B, 1, H, W, generator=g) * 0.02).to(dev)
    rgb = torch.randint(0, 256, (B, 3, H, W), generator=g).float().to(dev)
    alpha = 1.0 / 255.0
    w_kept = torch.empty(B, 2, H, W, device=dev)
    weights = mod.edge_weights(rgb, alpha).clone()
    seed = torch.ones((), device=dev)

    def leaf():
        """The depth as a fresh leaf per call (tools/warp_bench.py's note on AccumulateGrad and capture)."""
        return depth0.detach().requires_grad_(True)

    def fused(order, w):
        sm = mod.Smoother((H, W), B=B, order=order, device=dev)

        def call():
            depth = leaf()
            return torch.autograd.grad(sm(depth, w), depth, seed)[0]
        return call

    def composed(order, w):
        def call():
            depth = leaf()
            d = depth[:, 0]
            if order == 1:
                tx, ty = d[:, :, 1:] - d[:, :, :-1], d[:, 1:, :] - d[:, :-1, :]
                wx = None if w is None else w[:, 0, :, :-1]
                wy = None if w is None else w[:, 1, :-1, :]
            else:
                tx = d[:, :, :-2] + d[:, :, 2:] - 2 * d[:, :, 1:-1]
                ty = d[:, :-2, :] + d[:, 2:, :] - 2 * d[:, 1:-1, :]
                wx = None if w is None else torch.minimum(w[:, 0, :, :-2], w[:, 0, :, 1:-1])
                wy = None if w is None else torch.minimum(w[:, 1, :-2, :], w[:, 1, 1:-1, :])
            ex, ey = tx.abs(), ty.abs()
            loss = (ex if wx is None else wx * ex).mean() + (ey if wy is None else wy * ey).mean()
            return torch.autograd.grad(loss, depth, seed)[0]
        return call

    def edge_w():
        return mod.edge_weights(rgb, alpha, out=w_kept)

    def edge_w_torch():
        wx = torch.exp(-alpha * (rgb[..., :, 1:] - rgb[..., :, :-1]).abs().mean(1))
        wy = torch.exp(-alpha * (rgb[..., 1:, :] - rgb[..., :-1, :]).abs().mean(1))
        return torch.stack((F.pad(wx, (0, 1), value=1.0), F.pad(wy, (0, 0, 0, 1), value=1.0)), 1)

    def copy_of(bytes_per_px):
        src = torch.rand(px * bytes_per_px // 8, generator=g).to(dev)
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)

    variants, diffs = {}, {}
    for order in (1, 2):
        for tag, w in (("", None), ("_w", weights)):
            name = f"smooth_o{order}{tag}"
            variants[name], variants[name + "_torch"] = fused(order, w), composed(order, w)
            ours, theirs = variants[name]().clone(), variants[name + "_torch"]()
            diffs[name] = float(f"{float((ours - theirs).abs().max()) / float(ours.abs().max()):.3g}")
    variants["edge_w"], variants["edge_w_torch"] = edge_w, edge_w_torch
    diffs["edge_w"] = float(f"{float((edge_w() - edge_w_torch()).abs().max()):.3g}")
    floors = {"smooth_o1": 12, "smooth_o2": 12, "smooth_o1_w": 28, "smooth_o2_w": 28, "edge_w": 20}
    for n in sorted(set(floors.values())):
        variants[f"copy_{n}B"] = copy_of(n)
    res = measure(variants, graphable=tuple(variants))
    for name, n in floors.items():
        r = res[name]
        r["over_copy_floor_graph"] = round(r["graph_us"] / res[f"copy_{n}B"]["graph_us"], 2)
        r["fraction_of_hbm_roof"] = round(n * px / (r["graph_us"] * 1e-6) / HBM_BPS, 3)
        r["torch_graph_over_fused_graph"] = round(res[name + "_torch"]["graph_us"] / r["graph_us"], 2)
        r["torch_max_diff_over_scale"] = diffs[name]
    line = json.dumps({"shape": [B, H, W], **res})
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
