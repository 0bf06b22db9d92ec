"""Timing record of sparsify.sparsify against the host path it replaces, DataLoader_NYU.preprocess_depth,
on the same machine (DESIGN.md section 5's conventions, as tools/colorize_bench.py: HIP events around
each call, 10 warm-up calls, the median of 150 calls taken as three alternating blocks of 50 per
variant; each device variant also as a hipGraph of 20 back-to-back calls, per call = replay / 20, which
takes the host's launch gap out).

    python tools/sparsify_bench.py [--json out.json] [--only B H W --calls N]

The device call at 480 x 640 (NYU) and 352 x 1216 (KITTI) with B = 1 and B = 8, in two forms: 500 random
samples of the valid pixels ("n500"), and the reference's NYU rule with noise ("nyu": every pixel a
candidate, a per-image count from device memory, +-10 % noise on a tenth). The host path is timed with a
host clock on one 480 x 640 sample (it is hard-wired to that size) read from a synthetic directory, with
and without noise, mask file and ground truth in the page cache; times B for a batch from one worker.
--only runs N eager calls of the "nyu" form at one shape and nothing else: the run to put under a kernel
profiler for the per-kernel split. A record, not a gate."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nconv_pkg  # noqa: E402
from pointcloud_bench import measure  # noqa: E402


def device_forms(mod, dev, B, H, W):
    g = torch.Generator().manual_seed(0)
    depth = ((torch.rand(B, 1, H, W, generator=g) * 9 + 1) * (torch.rand(B, 1, H, W, generator=g) < 0.7)).to(dev)
    S = sys.modules[mod.sparsify.__module__]
    out = {"depth": torch.empty(B, 1, H, W, device=dev), "kept": torch.empty(B, dtype=torch.int32, device=dev),
           "workspace": torch.empty(S.workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)}
    state = S.make_state(1234, 0, dev)
    n_keep = torch.full((B,), int(0.9 * H * W), dtype=torch.int32, device=dev)
    return {
        "n500": lambda: mod.sparsify(depth, 500, state=state, out=out),
        "nyu": lambda: mod.sparsify(depth, n_keep, floor=None, noise_frac=0.1, noise_amp=0.1, state=state, out=out),
    }


def host_path(mod):
    """Median microseconds of preprocess_depth on one sample, (without, with) noise."""
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        for sub in ("train/gt", "train/depth", "train/img", "mask"):
            os.makedirs(os.path.join(d, sub))
        np.save(os.path.join(d, "train/gt/000.npy"), (rng.random((480, 640)) * 10).astype(np.float32))
        np.save(os.path.join(d, "mask/m0.npy"), (rng.random((480, 640)) < 0.9).astype(np.uint8))
        res = []
        for noise in (False, True):
            ds = mod.data.DataLoader_NYU(d, "train", use_mask=False, add_noise=noise)
            random.seed(0), torch.manual_seed(0)
            times = []
            for it in range(25):
                t0 = time.perf_counter()
                ds.preprocess_depth(ds.depths[0], False, noise)
                if it >= 5:
                    times.append((time.perf_counter() - t0) * 1e6)
            res.append(round(statistics.median(times), 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", type=int, nargs=3, default=None, metavar=("B", "H", "W"))
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    mod = nconv_pkg.load()
    dev = torch.device("cuda:0")
    if a.only:
        fn = device_forms(mod, dev, *a.only)["nyu"]
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"only": a.only, "calls": a.calls}))
        return
    record = {"threads": torch.get_num_threads()}
    for H, W in ((480, 640), (352, 1216)):
        for B in (1, 8):
            forms = device_forms(mod, dev, B, H, W)
            res = measure(forms, graphable=tuple(forms))
            for k, r in res.items():
                r["pixels_per_us_graph"] = round(B * H * W / r["graph_us"], 1)
            record[f"{B}x{H}x{W}"] = res
    plain, noisy = host_path(mod)
    record["host_preprocess_depth_one_sample_us"] = {"no_noise": plain, "noise": noisy}
    record["host_preprocess_depth_batch8_us"] = {"no_noise": round(8 * plain, 1), "noise": round(8 * noisy, 1)}
    dev8 = record["8x480x640"]["nyu"]["graph_us"]
    record["host_noise_batch8_over_device_nyu_8x480x640"] = round(8 * noisy / dev8, 1)
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
