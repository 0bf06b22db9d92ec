"""Timing record of the graphed config-4b training step (B = 8, 352 x 1216, generalized crop, fused
capturable AdamW, as bench.py's make_train_step) with train.ConfidenceLoss on forward_with_confidence,
against the same step with calculate_loss, on the same device in the same process.

    python tools/conf_train_bench.py [--batch 8] [--height 352] [--width 1216] [--blocks 5] [--steps 20]

Both steps are captured once; then `blocks` alternating blocks of `steps` replays each (depth, conf, depth,
conf, ...), HIP events around each block, after 10 warm-up replays of each. Reported per variant: the
median, minimum and maximum of the block means (ms per step), and the difference of the medians. The
confidence step reads one more plane in two backward kernels (nconv6's input gradient and its matrix-core
weight gradient, both with nconv7's backward fused in) and runs a loss of three launches over three planes
instead of three launches over two planes with a Sobel window. A record, not a gate."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nconv_pkg  # noqa: E402


def sparse_depth(g, B, H, W, dev, density=0.05):
    d = torch.rand(B, 1, H, W, generator=g) * 79 + 1
    return (d * (torch.rand(B, 1, H, W, generator=g) < density)).to(dev)


def make_step(m, dev, B, H, W, conf):
    torch.manual_seed(0)
    net = m.SETP1_NCONV(crop="generalized").to(dev)
    opt = m.train.get_optimizer(net, "adam", 1e-2, 1e-7, capturable=True, fused=True)
    g = torch.Generator().manual_seed(2000)
    S, gt = sparse_depth(g, B, H, W, dev), sparse_depth(g, B, H, W, dev)
    net.train()
    if conf:
        loss = m.ConfidenceLoss(p=1.0).to(dev)
        fn = lambda model, s, t: loss(model.forward_with_confidence(s), t)  # noqa: E731
    else:
        fn = lambda model, s, t: m.train.calculate_loss(model(s), t, True)  # noqa: E731
    return m.train.GraphedTrainStep(net, opt, fn, (S, gt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    m = nconv_pkg.load()
    dev = torch.device("cuda:0")
    steps = {"calculate_loss": make_step(m, dev, a.batch, a.height, a.width, False),
             "confidence_loss": make_step(m, dev, a.batch, a.height, a.width, True)}
    for s in steps.values():
        for _ in range(10):
            s()
    torch.cuda.synchronize()
    means = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, s in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                s()
            e1.record()
            e1.synchronize()
            means[k].append(e0.elapsed_time(e1) / a.steps)
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "height": a.height, "width": a.width,
           "blocks": a.blocks, "steps_per_block": a.steps}
    for k, v in means.items():
        out[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    out["difference_ms"] = round(out["confidence_loss"]["median_ms"] - out["calculate_loss"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
