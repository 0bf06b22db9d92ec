"""Timing record of occlusion.remove_occluded against a plain copy of the same plane (the traffic floor: 4
bytes read and 4 written per pixel) and against the min_support = 1 rule composed from torch ops, on the
same device tensors in the same process (DESIGN.md section 5's conventions, as tools/colorize_bench.py:
HIP events around each call, 10 warm-up calls, the median of 150 calls taken as three alternating
blocks of 50 per variant; each variant also as a hipGraph of 20 back-to-back calls, per call =
replay / 20, which takes the host's launch gap out).

    python tools/occlusion_bench.py [--batch 8] [--height 256] [--width 1216] [--json out.json]

The plane holds a depth in 1..80 at 5 % of its pixels. Windows (3, 3) and (16, 16), min_support 1 and 4,
jump_abs 1 m. The torch composition of the min_support = 1 rule: the plane with +inf at its empty pixels,
the window minimum as -max_pool2d of its negation (max_pool2d pads with -inf, so the border is clipped as
the rule asks), then valid & (v > min + 1) and a where(). The window minimum includes the centre, which
changes nothing for positive depths. Its result is compared with ours (it must be equal: one add and
comparisons). min_support = 4 has no cheap composition and is timed on our side only. A record, not a
gate: if the fused call does not beat the composition the record says so ("fused_beats_torch": false)."""
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

WINDOWS = ((3, 3), (16, 16))
SUPPORTS = (1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    mod = nconv_pkg.load()
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    src = ((torch.rand(B, 1, H, W, generator=g) * 79 + 1) * (torch.rand(B, 1, H, W, generator=g) < 0.05)).to(dev)
    out = {"depth": torch.empty(B, 1, H, W, device=dev)}
    copy_dst = torch.empty(B, 1, H, W, device=dev)
    inf = torch.tensor(float("inf"), device=dev)
    zero = torch.zeros((), device=dev)

    def torch_rule(rh, rw):
        valid = src > 0
        cand = torch.where(valid, src, inf)
        lo = -F.max_pool2d(-cand, (2 * rh + 1, 2 * rw + 1), 1, (rh, rw))
        return torch.where(valid & ~(src > lo + 1.0), src, zero)

    variants = {"copy": lambda: copy_dst.copy_(src)}
    removed = {}
    for rh, rw in WINDOWS:
        for ms in SUPPORTS:
            variants[f"ours_{rh}x{rw}_ms{ms}"] = (lambda rh=rh, rw=rw, ms=ms:
                                                 mod.remove_occluded(src, (rh, rw), min_support=ms, out=out))
            r = mod.remove_occluded(src, (rh, rw), min_support=ms, return_counts=True)[1].sum(0).tolist()
            removed[f"{rh}x{rw}_ms{ms}"] = {"valid": r[0], "removed": r[1]}
        variants[f"torch_{rh}x{rw}_ms1"] = lambda rh=rh, rw=rw: torch_rule(rh, rw)
        ours = mod.remove_occluded(src, (rh, rw), min_support=1)
        assert torch.equal(ours.view(torch.int32), torch_rule(rh, rw).view(torch.int32)), (rh, rw)

    res = measure(variants, graphable=tuple(variants))
    for rh, rw in WINDOWS:
        q, t = f"ours_{rh}x{rw}_ms1", f"torch_{rh}x{rw}_ms1"
        res[q]["torch_eager_over_ours_eager"] = round(res[t]["eager_us"] / res[q]["eager_us"], 2)
        res[q]["torch_graph_over_ours_graph"] = round(res[t]["graph_us"] / res[q]["graph_us"], 2)
        res[q]["fused_beats_torch"] = bool(res[q]["eager_us"] < res[t]["eager_us"] and res[q]["graph_us"] < res[t]["graph_us"])
    for k in res:
        if k.startswith("ours") or k == "copy":
            res[k]["bytes"] = 8 * px
            res[k]["fraction_of_hbm_roof"] = round(8 * px / (res[k]["graph_us"] * 1e-6) / HBM_BPS, 3)
            res[k]["graph_over_copy_graph"] = round(res[k]["graph_us"] / res["copy"]["graph_us"], 2)
    record = {"shape": [B, H, W], "valid_share": round(float((src > 0).float().mean()), 4), "counts": removed, **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
