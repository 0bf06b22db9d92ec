"""Timing record of sparsification (nconv_depth_sparsification, twelve launches) against a plain PyTorch
statement of the same figures, with tools/frames_bench.py's conventions (HIP events around each call, 10
warm-up calls, the median of 150 calls taken as three alternating blocks of 50 per variant; the library
call is also timed as a hipGraph of 20 back-to-back calls, per call = replay / 20).

    python tools/sparsification_bench.py [--batch 8] [--height 352] [--width 1216] [--steps 100]
                                         [--valid 0.3] [--json out.json]

KITTI-like validity: about 30 % of gt is valid. The PyTorch statement is batched and free of host round
trips: invalid pixels get the key +inf and zero terms, torch.sort(stable=True)
orders each image's H * W keys (twice: confidence and -|e|), the suffix sums are a flipped float64 cumsum,
and the curve points are gathered at k_j. Its counts must equal the library's and its sums agree to 1e-9
(another summation order). A record, not a gate."""
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
from frames_bench import GRAPH_CALLS, _eager_block, _graph_of  # noqa: E402

LAUNCHES = 12  # csrc/sparsification.hip: fixed, whatever the data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--valid", type=float, default=0.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    m = nconv_pkg.load()
    mod = sys.modules[m.sparsification.__module__]
    dev = torch.device("cuda:0")
    B, H, W, J = a.batch, a.height, a.width, a.steps
    g = torch.Generator().manual_seed(0)
    gt = ((torch.rand(B, 1, H, W, generator=g) * 79 + 1) * (torch.rand(B, 1, H, W, generator=g) < a.valid)).to(dev)
    pred = (gt + torch.randn(B, 1, H, W, generator=g).to(dev) * 2).contiguous()
    conf = torch.rand(B, 1, H, W, generator=g).to(dev)
    bounds = (0.0, 80.0, 0.0, 0.0)

    keep = {}

    def ours():
        keep["curves"], _, keep["ws"] = mod._launch(pred, gt, conf, J, bounds, False, keep.get("curves"), False,
                                                    keep.get("ws"))
        return keep["curves"]

    j = torch.arange(J, device=dev)
    inf = torch.tensor(float("inf"), device=dev)
    zero = torch.zeros((), device=dev)

    def torch_curves():
        p, t, c = pred.view(B, -1), gt.view(B, -1), conf.view(B, -1)
        valid = (t > 0) & (t <= 80.0)
        e = p - t
        a_, q_ = torch.where(valid, e.abs(), zero), torch.where(valid, e * e, zero)
        n = valid.sum(1)
        k = (j[None, :] * n[:, None]) // J
        out = []
        for key in (torch.where(valid, c, inf), torch.where(valid, -a_, inf)):
            idx = torch.sort(key, dim=1, stable=True).indices
            sa = a_.double().gather(1, idx).flip(1).cumsum(1).flip(1)
            sq = q_.double().gather(1, idx).flip(1).cumsum(1).flip(1)
            out.append(torch.stack(((n[:, None] - k).double(), sa.gather(1, k), sq.gather(1, k)), -1))
        return torch.stack(out, 1)

    mine, ref = ours().clone(), torch_curves()
    torch.cuda.synchronize()
    assert torch.equal(mine[..., 0], ref[..., 0])
    rel = float(((mine - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    assert rel < 1e-9, rel

    variants = {"sparsification": ours, "torch_sort_cumsum": torch_curves}
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    eager = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            eager[k] += _eager_block(fn, 50)
    res = {k: {"eager_us": round(statistics.median(v), 2)} for k, v in eager.items()}
    # the library call as a hipGraph; torch.sort's temporaries are the framework's business, so the PyTorch
    # statement is timed eagerly only
    graph = _graph_of(ours)
    times = [t / GRAPH_CALLS for _ in range(3) for t in _eager_block(graph.replay, 10)]
    res["sparsification"]["graph_us"] = round(statistics.median(times), 2)
    res["launches"] = LAUNCHES
    res["ratio_torch_over_ours_eager"] = round(res["torch_sort_cumsum"]["eager_us"] / res["sparsification"]["eager_us"], 2)
    res["max_rel_diff_vs_torch"] = rel
    res["valid_share"] = round(float((gt > 0).float().mean()), 4)
    res["workspace_mb"] = round(keep["ws"].numel() / 2 ** 20, 1)
    res["shape"] = [B, H, W, J]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
