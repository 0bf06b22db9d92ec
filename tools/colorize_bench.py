"""Timing record of visualize.colorize against the same picture composed from torch ops on the same
device tensors in the same process, and against today's host path (DESIGN.md section 5's conventions,
as tools/lidar_bench.py: HIP events around each call, 10 warm-up calls, the median of 150 calls taken as
three alternating blocks of 50 per variant; each device variant also as a hipGraph of 20 back-to-back
calls, per call = replay / 20, which takes the host's launch gap out).

    python tools/colorize_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

Three forms: a fixed range; the per-image range; the per-image range with radius 1 over a camera image
(overlay of a 5 % dense plane). The torch composition of each is amin / amax (per-image range),
normalise, round, clamp, long, a gather of the table and, for the overlay, a 3 x 3 min pooling of the
plane with its empty pixels at +inf and a where() against the background. Its pictures are compared with
ours by the share of equal bytes (round(x * s) in torch is the same arithmetic; the composition is not
held bit for bit). The host path is what compat save_depth did before for a device tensor: .cpu(), then
its float64 arithmetic, without the PNG write; it is timed with a host clock, one image at a time.
Bytes: 4 read + 3 written per pixel, 4 more read per pixel for the range pass, 3 more read for a
background; the roof is 8 TB/s. A record, not a gate: if the fused call does not beat the composition
the record says so ("fused_beats_torch": false)."""
import argparse
import json
import os
import statistics
import sys
import time

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
    V = mod.visualize
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    dense = (torch.rand(B, 1, H, W, generator=g) * 79 + 1).to(dev)
    sparse = (dense.cpu() * (torch.rand(B, 1, H, W, generator=g) < 0.05)).to(dev)
    rgb = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    table = torch.from_numpy(np.array(mod.COLORMAPS["inferno"])).to(dev)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    ws = torch.empty(V.workspace_bytes(B), dtype=torch.uint8, device=dev)
    inf = torch.tensor(float("inf"), device=dev)

    def torch_index(v, lo, s):
        return torch.round((v - lo) * s).clamp_(0, 255).long()

    def torch_fixed():
        return table[torch_index(dense[:, 0], 1.0, 255.0 / 79.0)]

    def torch_auto():
        v = dense[:, 0]
        lo, hi = v.amin(dim=(1, 2), keepdim=True), v.amax(dim=(1, 2), keepdim=True)
        return table[torch_index(v, lo, 255.0 / (hi - lo))]

    def torch_overlay():
        v = sparse[:, 0]
        ok = v > 0
        cand = torch.where(ok, v, inf)
        lo = cand.amin(dim=(1, 2), keepdim=True)
        hi = torch.where(ok, v, -inf).amax(dim=(1, 2), keepdim=True)
        shown = -F.max_pool2d(-cand[:, None], 3, 1, 1)[:, 0]
        has = shown < inf
        idx = torch_index(torch.where(has, shown, lo), lo, 255.0 / (hi - lo))
        return torch.where(has[..., None], table[idx], rgb)

    ours = {
        "colorize_fixed": lambda: V.colorize(dense, vmin=1.0, vmax=80.0, out=out),
        "colorize_auto": lambda: V.colorize(dense, out=out, workspace=ws),
        "colorize_overlay": lambda: V.overlay(sparse, rgb, out=out, workspace=ws),
    }
    theirs = {"torch_fixed": torch_fixed, "torch_auto": torch_auto, "torch_overlay": torch_overlay}
    pairs = (("colorize_fixed", "torch_fixed"), ("colorize_auto", "torch_auto"), ("colorize_overlay", "torch_overlay"))
    agree = {q: round(float((ours[q]().clone() == theirs[t]()).float().mean()), 5) for q, t in pairs}
    assert min(agree.values()) > 0.99, agree

    variants = {**ours, **theirs}
    res = measure(variants, graphable=tuple(variants))
    nbytes = {"colorize_fixed": 7 * px, "colorize_auto": 11 * px, "colorize_overlay": 14 * px}
    for q, t in pairs:
        res[q]["bytes"] = nbytes[q]
        res[q]["fraction_of_hbm_roof"] = round(nbytes[q] / (res[q]["graph_us"] * 1e-6) / HBM_BPS, 3)
        res[q]["torch_eager_over_ours_eager"] = round(res[t]["eager_us"] / res[q]["eager_us"], 2)
        res[q]["torch_graph_over_ours_graph"] = round(res[t]["graph_us"] / res[q]["graph_us"], 2)
        res[q]["fused_beats_torch"] = bool(res[q]["eager_us"] < res[t]["eager_us"] and res[q]["graph_us"] < res[t]["graph_us"])

    def host_path():  # one image, as save_depth took it: .cpu(), float64 min-max normalise, round half up
        d = np.asarray(dense[0, 0].cpu(), dtype=np.float64)
        lo, hi = float(d.min()), float(d.max())
        return ((d - lo) / (hi - lo) * 255.0 + 0.5).astype(np.uint8)

    host_path()
    times = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_path()
        times.append((time.perf_counter() - t0) * 1e6)
    record = {"shape": [B, H, W], "equal_byte_share_vs_torch": agree, **res,
              "host_path_one_image_us": round(statistics.median(times), 1),
              "host_path_batch_us": round(statistics.median(times) * B, 1)}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
