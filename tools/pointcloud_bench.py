"""Timing record of pointcloud.backproject (with and without colour) and backproject_map against the
torch-op formulation on the same device tensors in the same process (DESIGN.md section 5's
conventions, as tools/frames_bench.py: HIP events around each call, 10 warm-up calls, the median of
150 calls taken as three alternating blocks of 50 per variant; ours also as a hipGraph of 20
back-to-back calls, per call = replay / 20, which takes the host's launch gap out).

    python tools/pointcloud_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

At 5 %, 40 % and 100 % valid pixels. The torch formulation is a meshgrid, the elementwise passes, a
boolean mask and xyz[mask]; the mask index synchronises with the host to learn the point count, so it
cannot be captured in a graph and is timed eagerly only (its event time includes that wait, which is
part of its cost). Effective traffic counts what the result needs once: 4 B/px of depth read, 12 B per
point written (+ 3 B read and 3 B written per point with uint8 colour); the map form 4 B/px read and
12 B/px written. The roof is 8 TB/s. A record, not a gate."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nconv_pkg  # noqa: E402
from frames_bench import GRAPH_CALLS, HBM_BPS, _eager_block, _graph_of  # noqa: E402


def measure(variants, graphable, blocks=3, per_block=50, warmup=10):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    eager = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            eager[k] += _eager_block(fn, per_block)
    res = {k: {"eager_us": round(statistics.median(eager[k]), 2)} for k in variants}
    graphs = {k: _graph_of(variants[k]) for k in graphable}
    graph = {k: [] for k in graphable}
    for _ in range(blocks):
        for k, g in graphs.items():
            graph[k] += [t / GRAPH_CALLS for t in _eager_block(g.replay, per_block // 5)]
    for k in graphable:
        res[k]["graph_us"] = round(statistics.median(graph[k]), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    m = nconv_pkg.load()
    P = m.pointcloud
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    k = torch.tensor([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]], device=dev)
    rgb = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    out = {"xyz": torch.empty(px, 3, device=dev), "rgb": torch.empty(px, 3, dtype=torch.uint8, device=dev),
           "offsets": torch.empty(B + 1, dtype=torch.int32, device=dev),
           "workspace": torch.empty(P.workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)}
    m_out = torch.empty(B, 3, H, W, device=dev)
    jj, ii = torch.arange(W, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32)
    record = {"shape": [B, H, W]}
    for frac in (0.05, 0.4, 1.0):
        depth = (torch.rand(B, 1, H, W, generator=g) * 79 + 1) * (torch.rand(B, 1, H, W, generator=g) < frac)
        depth = depth.to(dev)

        def torch_points(color=False):
            v, u = torch.meshgrid(ii, jj, indexing="ij")
            z = depth[:, 0]
            x = (u - k[0, 2]) * z / k[0, 0]
            y = (v - k[1, 2]) * z / k[1, 1]
            mask = z > 0
            xyz = torch.stack((x, y, z), dim=-1)[mask]
            return (xyz, rgb[mask]) if color else xyz

        def torch_map():
            v, u = torch.meshgrid(ii, jj, indexing="ij")
            z = depth[:, 0]
            nan = torch.full_like(z, float("nan"))
            ok = z > 0
            return torch.stack((torch.where(ok, (u - k[0, 2]) * z / k[0, 0], nan),
                                torch.where(ok, (v - k[1, 2]) * z / k[1, 1], nan), torch.where(ok, z, nan)), dim=1)

        pc = P.backproject(depth, k, color=rgb, out=out)
        n = pc.count()
        ref_xyz, ref_rgb = torch_points(True)
        assert n == ref_xyz.shape[0] and torch.equal(pc.xyz[:n], ref_xyz) and torch.equal(pc.rgb[:n], ref_rgb)
        assert torch.equal(torch.nan_to_num(P.backproject_map(depth, k, out=m_out), nan=-1.0),
                           torch.nan_to_num(torch_map(), nan=-1.0))
        out_plain = {q: out[q] for q in ("xyz", "offsets", "workspace")}
        res = measure({
            "points": lambda: P.backproject(depth, k, out=out_plain),
            "points_rgb": lambda: P.backproject(depth, k, color=rgb, out=out),
            "map": lambda: P.backproject_map(depth, k, out=m_out),
            "torch_points": torch_points,
            "torch_points_rgb": lambda: torch_points(True),
            "torch_map": torch_map,
        }, graphable=("points", "points_rgb", "map"))
        useful = {"points": 4 * px + 12 * n, "points_rgb": 4 * px + 18 * n, "map": 16 * px}
        for q, nbytes in useful.items():
            gbps = nbytes / (res[q]["graph_us"] * 1e-6) / 1e9
            res[q]["effective_GBps"] = round(gbps, 1)
            res[q]["fraction_of_hbm_roof"] = round(gbps * 1e9 / HBM_BPS, 3)
            t = "torch_" + q
            res[q]["torch_eager_over_ours_eager"] = round(res[t]["eager_us"] / res[q]["eager_us"], 2)
            res[q]["torch_eager_over_ours_graph"] = round(res[t]["eager_us"] / res[q]["graph_us"], 2)
        res["points_valid"] = n
        record[f"valid_{int(frac * 100)}pct"] = res
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
