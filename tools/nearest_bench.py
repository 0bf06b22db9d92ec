"""Timing record of nearest.nearest_sample against the copy floor of the same plane (4 bytes read and 4
written per pixel) on the same device tensors in the same process (DESIGN.md section 5's conventions, as
tools/ipbasic_bench.py: HIP events around each call, 10 warm-up calls, the median of 150 calls taken as
three alternating blocks of 50 per variant; each variant also as a hipGraph of 20 back-to-back calls, per
call = replay / 20, which takes the host's launch gap out).

    python tools/nearest_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

Three cases:
    kitti    the IP-Basic bench's plane: a depth in 1..80 at 5 % of the pixels, none in the top 100 rows;
             the fill alone (kitti_fill) and with index, dist2 and dist as well (kitti_all)
    single   one sample per image, in the bottom left corner: every pixel searches its whole row, the
             worst case of the row pass
    copy     a plain copy of the plane: the traffic floor of one pass
The bytes of a call are the source read once per pass, the int32 workspace written and read, and the
outputs written: a count from the shapes, not a measurement. A record, not a gate."""
import argparse
import json
import os
import sys

import torch

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
    kitti = (torch.rand(B, 1, H, W, generator=g) * 79 + 1) * (torch.rand(B, 1, H, W, generator=g) < 0.05)
    kitti[:, :, :min(100, H // 3)] = 0
    kitti = kitti.to(dev)
    single = torch.zeros(B, 1, H, W, device=dev)
    single[:, :, H - 1, 0] = 41.5
    out = {"depth": torch.empty(B, 1, H, W, device=dev), "work": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "index": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "dist2": torch.empty(B, H, W, dtype=torch.int32, device=dev), "dist": torch.empty(B, H, W, device=dev)}
    every = dict(return_index=True, return_dist2=True, return_dist=True)
    copy_dst = torch.empty(B, 1, H, W, device=dev)

    variants = {"copy": lambda: copy_dst.copy_(kitti),
                "kitti_fill": lambda: mod.nearest_sample(kitti, out=out),
                "kitti_all": lambda: mod.nearest_sample(kitti, out=out, **every),
                "single_fill": lambda: mod.nearest_sample(single, out=out),
                "single_all": lambda: mod.nearest_sample(single, out=out, **every)}
    res = measure(variants, graphable=tuple(variants))
    for name, planes_out in (("kitti_fill", 1), ("kitti_all", 4), ("single_fill", 1), ("single_all", 4)):
        q = res[name]
        q["bytes"] = 4 * px * (1 + 2 + planes_out)  # source, workspace out and back, outputs
        q["graph_over_copy"] = round(q["graph_us"] / res["copy"]["graph_us"], 2)
        q["fraction_of_hbm_roof"] = round(q["bytes"] / (q["graph_us"] * 1e-6) / HBM_BPS, 4)
    _, d2 = mod.nearest_sample(kitti, return_dist2=True)
    record = {"shape": [B, H, W], "kitti_valid_share": round(float((kitti > 0).float().mean()), 4),
              "kitti_mean_distance_px": round(float(d2.float().sqrt().mean()), 2),
              "kitti_max_distance_px": round(float(d2.max()) ** 0.5, 2), **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
