"""Timing record of frames.ingest / frames.export_depth16 against the device-side torch-op
equivalents (DESIGN.md section 5's conventions: HIP events around each call, 10 warm-up calls, the
median of 150 calls taken as three alternating blocks of 50 per variant, same device tensors in the
same process). Each variant is also timed as a hipGraph of 20 back-to-back calls (per call = replay
/ 20), which takes the host's launch gap out.

    python tools/frames_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

Traffic floors at the default shape (8 TB/s): ingest rgb + depth + gt reads 24.0 MB and writes
68.5 MB, export reads 13.7 MB and writes 6.8 MB. A record, not a gate."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nconv_pkg  # noqa: E402

HBM_BPS = 8e12
GRAPH_CALLS = 20


def _eager_block(fn, n):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]


def _graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    return g


def measure(variants, blocks=3, per_block=50, warmup=10):
    """{name: {'eager_us': median, 'graph_us': median per call}} with the variants' blocks alternating."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    eager = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            eager[k] += _eager_block(fn, per_block)
    graphs = {k: _graph_of(fn) for k, fn in variants.items()}
    graph = {k: [] for k in variants}
    for _ in range(blocks):
        for k, g in graphs.items():
            graph[k] += [t / GRAPH_CALLS for t in _eager_block(g.replay, per_block // 5)]
    return {k: {"eager_us": round(statistics.median(eager[k]), 2), "graph_us": round(statistics.median(graph[k]), 2)}
            for k in variants}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    m = nconv_pkg.load()
    dev = torch.device("cuda:0")
    B, h, w = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(0)
    rgb = torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    as16 = lambda t: t.to(torch.int16).view(torch.uint16)
    depth = as16(torch.randint(-32768, 32768, (B, h, w), generator=g)).to(dev)
    gt = as16(torch.randint(-32768, 32768, (B, h, w), generator=g)).to(dev)
    pred = (torch.rand(B, 1, h, w, generator=g) * 90).to(dev)
    out = {"rgb": torch.empty(B, 3, h, w, device=dev), "depth": torch.empty(B, 1, h, w, device=dev),
           "gt": torch.empty(B, 1, h, w, device=dev)}
    out16 = m.export_depth16(pred)
    # where this torch build has no uint16 shift / cast kernels on the device the baseline reads the
    # planes as int32 copies made beforehand and exports to int32 (both favour the baseline)
    try:
        (depth[:1] >> 8).float()
        (pred[:1] * 256).round().clamp(0, 65535).to(torch.uint16)
        torch.cuda.synchronize()
        native16 = True
    except (RuntimeError, NotImplementedError):
        native16 = False
    d_src = depth if native16 else depth.view(torch.int16).to(torch.int32).bitwise_and_(0xFFFF)
    g_src = gt if native16 else gt.view(torch.int16).to(torch.int32).bitwise_and_(0xFFFF)

    def torch_ingest():
        r = rgb.to(torch.float32).flip(-1).permute(0, 3, 1, 2).contiguous()
        d = (d_src >> 8).float() / 256
        t = (g_src >> 8).float() / 256
        return r, d, t

    def torch_export():
        return (pred * 256).round().clamp(0, 65535).to(torch.uint16 if native16 else torch.int32)

    ours = m.ingest(rgb=rgb, depth=depth, gt=gt, out=out)
    ref = torch_ingest()
    assert torch.equal(ours["rgb"], ref[0]) and torch.equal(ours["depth"][:, 0], ref[1])
    assert torch.equal(out16.cpu().to(torch.int32), torch_export().cpu().to(torch.int32))
    res = measure({
        "ingest": lambda: m.ingest(rgb=rgb, depth=depth, gt=gt, out=out),
        "ingest_depth_only": lambda: m.ingest(depth=depth, out={"depth": out["depth"]}),
        "torch_ingest": torch_ingest,
        "export": lambda: m.export_depth16(pred, out=out16),
        "torch_export": torch_export,
    })
    px = B * h * w
    floors = {"ingest": (7 + 20) * px / HBM_BPS * 1e6, "ingest_depth_only": (2 + 4) * px / HBM_BPS * 1e6,
              "export": (4 + 2) * px / HBM_BPS * 1e6}
    for k, f in floors.items():
        res[k]["floor_us"] = round(f, 2)
        res[k]["graph_over_floor"] = round(res[k]["graph_us"] / f, 2)
    res["ratio_ingest_torch_over_ours"] = round(res["torch_ingest"]["graph_us"] / res["ingest"]["graph_us"], 2)
    res["ratio_export_torch_over_ours"] = round(res["torch_export"]["graph_us"] / res["export"]["graph_us"], 2)
    res["shape"] = [B, h, w]
    res["torch_uint16_kernels"] = native16
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
