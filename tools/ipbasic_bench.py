"""Timing record of ipbasic.ipbasic_fill against the copy floor of the same planes (4 bytes read and 4
written per pixel, times the plane passes of the launches: one without extrapolate, two with it) and
against the same pipeline composed from torch ops, on the same device tensors in the same process
(DESIGN.md section 5's conventions, as tools/occlusion_bench.py: HIP events around each call, 10 warm-up
calls, the median of 150 calls taken as three alternating blocks of 50 per variant; each variant also as
a hipGraph of 20 back-to-back calls, per call = replay / 20, which takes the host's launch gap out).

    python tools/ipbasic_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

The plane holds a depth in 1..80 at 5 % of its pixels, none in the top 100 rows (a KITTI plane). Both
extrapolate settings, the other options at their defaults. The torch composition is what a user would
write today: max_pool2d for the dilations (the first one as a full 5 x 5: max_pool2d has no diamond, and
a max over thirteen shifted slices would be slower still), -max_pool2d(-x) for the erosion, unfold +
median for the 5 x 5 median (replicate padding), conv2d on a reflect-padded plane for the blur, argmax +
gather for the column extrapolation. It is the reference for speed, not the code under test, and does
not have to match bit for bit; the share of pixels on which it agrees with ours to 1e-3 m is recorded.
A record, not a gate: if the fused call does not beat the composition the record says so
("fused_beats_torch": false)."""
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

T = 0.1


def torch_ipbasic(src, max_depth, extrapolate, w5):
    """fill_in_fast from torch ops on (B, 1, H, W)."""
    zero = torch.zeros((), device=src.device)
    v = torch.where((src > T) & (max_depth - src > T), max_depth - src, zero)
    v = F.max_pool2d(v, 5, 1, 2)                       # the custom kernel, as a full 5 x 5
    v = F.max_pool2d(v, 5, 1, 2)                       # close
    v = -F.max_pool2d(-v, 5, 1, 2)
    v = torch.where(v < T, F.max_pool2d(v, 7, 1, 3), v)
    if extrapolate:
        ok = v > T
        top = torch.where(ok.any(dim=2, keepdim=True), ok.int().argmax(dim=2, keepdim=True), 0)
        rows = torch.arange(v.shape[2], device=v.device).view(1, 1, -1, 1)
        v = torch.where(rows < top, torch.gather(v, 2, top.expand(-1, -1, 1, -1)), v)
        v = torch.where(v < T, F.max_pool2d(v, 31, 1, 15), v)
    B, _, H, W = v.shape
    win = F.unfold(F.pad(v, (2, 2, 2, 2), mode="replicate"), 5)             # (B, 25, H * W)
    v = win.median(dim=1).values.view(B, 1, H, W)
    blurred = F.conv2d(F.pad(v, (2, 2, 2, 2), mode="reflect"), w5)
    v = torch.where(v > T, blurred, v)
    return torch.where(v > T, max_depth - v, zero)


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
    src = (torch.rand(B, 1, H, W, generator=g) * 79 + 1) * (torch.rand(B, 1, H, W, generator=g) < 0.05)
    src[:, :, :min(100, H // 3)] = 0
    src = src.to(dev)
    out = {"depth": torch.empty(B, 1, H, W, device=dev), "work": torch.empty(B, H, W, device=dev),
           "top": torch.empty(B, W, dtype=torch.int32, device=dev)}
    copy_dst = torch.empty(B, 1, H, W, device=dev)
    k1 = torch.tensor([0.0625, 0.25, 0.375, 0.25, 0.0625], device=dev)
    w5 = (k1[:, None] * k1[None, :]).view(1, 1, 5, 5)

    variants = {"copy": lambda: copy_dst.copy_(src)}
    agree = {}
    for ex in (False, True):
        name = "extrapolate" if ex else "plain"
        variants[f"ours_{name}"] = lambda ex=ex: mod.ipbasic_fill(src, extrapolate=ex, out=out)
        variants[f"torch_{name}"] = lambda ex=ex: torch_ipbasic(src, 100.0, ex, w5)
        ours = mod.ipbasic_fill(src, extrapolate=ex).clone()
        theirs = torch_ipbasic(src, 100.0, ex, w5)
        agree[name] = round(float(((ours - theirs).abs() <= 1e-3).float().mean()), 4)

    res = measure(variants, graphable=tuple(variants))
    for ex, passes in ((False, 1), (True, 2)):
        name = "extrapolate" if ex else "plain"
        q, t = res[f"ours_{name}"], res[f"torch_{name}"]
        q["copy_floor_us"] = round(passes * res["copy"]["graph_us"], 2)
        q["bytes"] = 8 * px * passes
        q["graph_over_copy_floor"] = round(q["graph_us"] / q["copy_floor_us"], 2)
        q["fraction_of_hbm_roof"] = round(q["bytes"] / (q["graph_us"] * 1e-6) / HBM_BPS, 3)
        q["torch_eager_over_ours_eager"] = round(t["eager_us"] / q["eager_us"], 2)
        q["torch_graph_over_ours_graph"] = round(t["graph_us"] / q["graph_us"], 2)
        q["fused_beats_torch"] = bool(q["eager_us"] < t["eager_us"] and q["graph_us"] < t["graph_us"])
    record = {"shape": [B, H, W], "valid_share": round(float((src > 0).float().mean()), 4),
              "share_within_1mm_of_torch": agree, **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
