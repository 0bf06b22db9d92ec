"""Timing record of augment (nconv_frame_augment, one launch) against a straightforward PyTorch
composition of the same result, with tools/frames_bench.py's conventions (HIP events around each call,
10 warm-up calls, the median of 150 calls taken as three alternating blocks of 50 per variant; each
variant that can be captured is also timed as a hipGraph of 20 back-to-back calls, per call = replay
/ 20).

    python tools/augment_bench.py [--batch 8] [--height 352] [--width 1216] [--out-height 256]
                                  [--out-width 1216] [--json out.json]

The batch is rgb + depth + gt + k. The PyTorch composition draws its parameters with torch.rand on the
device, brings them to the host (the round trip a user's code makes: slicing needs Python integers),
slices and flips image by image, and applies the jitter as elementwise ops; it cannot be captured.
`torch_fixed` is the same composition with the parameters already on the host (no draw, no round
trip), which can be captured: the floor of what the composition costs on the device. Traffic floor at
the default shape (8 TB/s): 5 planes of 256 x 1216 read and written, 99.6 MB. A record, not a gate."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import nconv_pkg  # noqa: E402
from frames_bench import HBM_BPS, _eager_block, measure  # noqa: E402

AMP = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--out-height", type=int, default=256)
    ap.add_argument("--out-width", type=int, default=1216)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    m = nconv_pkg.load()
    dev = torch.device("cuda:0")
    B, H, W, h, w = a.batch, a.height, a.width, a.out_height, a.out_width
    g = torch.Generator().manual_seed(0)
    rgb = (torch.rand(B, 3, H, W, generator=g) * 255).to(dev)
    gt = (torch.rand(B, 1, H, W, generator=g) * 80).to(dev)
    depth = gt * (torch.rand(B, 1, H, W, generator=g) < 0.05).to(dev)
    k = torch.eye(3).repeat(B, 1, 1).to(dev)
    k[:, 0, 2], k[:, 1, 2] = W / 2, H / 2
    au = m.Augmenter((H, W), (h, w), B=B, seed=1, brightness=AMP, contrast=AMP, color=AMP)

    def compose(y0, x0, flip, gains, fy, fx, ft):
        """The result for host lists of parameters, a (B, 5) device tensor of gains and the parameters
        as device tensors (fp32 offsets, bool flips) for the intrinsics."""
        outs = {"rgb": [], "depth": [], "gt": []}
        for b in range(B):
            for n, t in (("rgb", rgb), ("depth", depth), ("gt", gt)):
                v = t[b, :, y0[b]:y0[b] + h, x0[b]:x0[b] + w]
                outs[n].append(v.flip(-1) if flip[b] else v)
        r = torch.stack(outs["rgb"])
        gb, gc, gch = gains[:, 0].view(B, 1, 1, 1), gains[:, 1].view(B, 1, 1, 1), gains[:, 2:].view(B, 3, 1, 1)
        r = (((r * gb) * gch - 127.5) * gc + 127.5).clamp(0.0, 255.0)
        ko = k.clone()
        cx = k[:, 0, 2] - fx
        ko[:, 0, 2] = torch.where(ft, (w - 1) - cx, cx)
        ko[:, 1, 2] = k[:, 1, 2] - fy
        return r, torch.stack(outs["depth"]), torch.stack(outs["gt"]), ko

    def torch_augment():
        u = torch.rand(B, 8, device=dev)
        fy, fx, ft = (u[:, 0] * (H - h + 1)).floor(), (u[:, 1] * (W - w + 1)).floor(), u[:, 2] < 0.5
        p = torch.stack((fy, fx, ft.float()), 1).cpu()  # the round trip: the slices below need Python integers
        y0, x0, flip = p[:, 0].long().tolist(), p[:, 1].long().tolist(), p[:, 2].bool().tolist()
        return compose(y0, x0, flip, 1 + AMP * (2 * u[:, 3:] - 1), fy, fx, ft)

    # the same composition on the parameters the kernel drew: the two agree bit for bit where no
    # fused multiply-add is formed by torch's elementwise kernels (reported, not asserted)
    ours = {n: t.clone() for n, t in au(rgb=rgb, depth=depth, gt=gt, k=k).items()}
    par, gains = ours["params"].cpu(), ours["gains"]
    fixed = (par[:, 0].tolist(), par[:, 1].tolist(), [bool(v) for v in par[:, 2].tolist()], gains,
             ours["params"][:, 0].float(), ours["params"][:, 1].float(), ours["params"][:, 2] != 0)
    ref = compose(*fixed)
    assert torch.equal(ours["depth"], ref[1]) and torch.equal(ours["gt"], ref[2]) and torch.equal(ours["k"], ref[3])
    rgb_diff = float((ours["rgb"] - ref[0]).abs().max())
    assert rgb_diff < 1e-3, rgb_diff

    res = measure({
        "augment": lambda: au(rgb=rgb, depth=depth, gt=gt, k=k),
        "torch_fixed": lambda: compose(*fixed),
    })
    # the composition with its draw and round trip cannot be captured: eager only
    for _ in range(10):
        torch_augment()
    times = [t for _ in range(3) for t in _eager_block(torch_augment, 50)]
    res["torch_augment"] = {"eager_us": round(statistics.median(times), 2)}
    floor = 2 * 5 * 4 * B * h * w / HBM_BPS * 1e6
    res["augment"]["floor_us"] = round(floor, 2)
    res["augment"]["graph_over_floor"] = round(res["augment"]["graph_us"] / floor, 2)
    res["ratio_torch_fixed_over_ours_graph"] = round(res["torch_fixed"]["graph_us"] / res["augment"]["graph_us"], 2)
    res["ratio_torch_augment_over_ours_eager"] = round(res["torch_augment"]["eager_us"] / res["augment"]["eager_us"], 2)
    res["rgb_max_abs_diff_vs_torch"] = rgb_diff
    res["shape"] = [B, H, W, h, w]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
