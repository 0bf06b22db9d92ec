"""Timing record of pointcloud.normals / normal_image / backproject(normals=True) against the same
definition composed from torch ops on the same device tensors in the same process (DESIGN.md section
5's conventions, as tools/colorize_bench.py: HIP events around each call, the median of 150 calls taken
as three alternating blocks of 50 per variant; each variant also as a hipGraph of 20 back-to-back
calls, per call = replay / 20). Before the timed blocks every variant runs for --warm-seconds (time
based, so the clocks have settled whatever a call costs), and the record carries the clocks rocm-smi
reports before and after.

    python tools/normals_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

All pixels are valid (a smooth random surface, every neighbour inside the gate). The torch composition
is backproject_map, four shifted slices with their masks, two where() chains for the one-sided
differences, a cross product, a norm and a division; the picture adds the scale, round and byte cast,
the packed form a boolean gather. It is not defined bit for bit (torch fuses nothing and rounds the
same way, but the record does not rely on it): the share of pixels whose three components agree
bitwise with ours is reported, not asserted. Bytes: 4 read + 12 written per pixel for the map, 4 + 3
for the picture, and for the fourth launch of the packed form 4 (index) + 4 (depth, its neighbours come
from cache) + 12; the roof is 8 TB/s. A record, not a gate."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nconv_pkg  # noqa: E402
from frames_bench import HBM_BPS  # noqa: E402
from pointcloud_bench import measure  # noqa: E402


def clocks():
    """What rocm-smi reports for the first device's clocks (read only), or why it could not be asked."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else f"rocm-smi exit {r.returncode}"
    except Exception as e:  # noqa: BLE001
        return f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--warm-seconds", type=float, default=0.5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    mod = nconv_pkg.load()
    P = mod.pointcloud
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    k = torch.tensor([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]], device=dev)
    ii = torch.arange(H, dtype=torch.float32).reshape(1, 1, H, 1)
    jj = torch.arange(W, dtype=torch.float32).reshape(1, 1, 1, W)
    depth = (20.0 + 5.0 * torch.sin(ii / 40.0) * torch.cos(jj / 60.0) + 0.01 * torch.rand(B, 1, H, W, generator=g)).to(dev)
    rel = 0.1
    m_out = torch.empty(B, 3, H, W, device=dev)
    i_out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    cloud = {"xyz": torch.empty(px, 3, device=dev), "index": torch.empty(px, dtype=torch.int32, device=dev),
             "normals": torch.empty(px, 3, device=dev), "offsets": torch.empty(B + 1, dtype=torch.int32, device=dev),
             "workspace": torch.empty(P.workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)}
    nan = torch.tensor(float("nan"), device=dev)

    def torch_map():
        p = P.backproject_map(depth, k)
        z = p[:, 2:3]
        ok = ~torch.isnan(z)
        tol = rel * z

        def shifted(t, di, dj, fill):
            s = torch.full_like(t, fill)
            src = t[..., max(di, 0):H + min(di, 0), max(dj, 0):W + min(dj, 0)]
            s[..., max(-di, 0):H + min(-di, 0), max(-dj, 0):W + min(-dj, 0)] = src
            return s

        def tangent(lo, hi):
            pl, ph = shifted(p, *lo, 0.0), shifted(p, *hi, 0.0)
            ul = shifted(ok, *lo, False) & ((pl[:, 2:3] - z).abs() <= tol)
            uh = shifted(ok, *hi, False) & ((ph[:, 2:3] - z).abs() <= tol)
            return torch.where(uh, ph, p) - torch.where(ul, pl, p), ul | uh

        tu, has_u = tangent((0, -1), (0, 1))
        tv, has_v = tangent((-1, 0), (1, 0))
        c = torch.cross(tv, tu, dim=1)
        c = torch.where((c * p).sum(1, keepdim=True) > 0, -c, c)
        l = c.norm(dim=1, keepdim=True)
        return torch.where(ok & has_u & has_v & (l > 0) & (l < float("inf")), c / l, nan)

    def torch_image():
        n = torch_map()
        t = torch.stack([n[:, 0], -n[:, 1], -n[:, 2]], dim=-1)
        return torch.round((t * 0.5 + 0.5) * 255.0).nan_to_num_(0.0).clamp_(0, 255).to(torch.uint8)

    def torch_points():
        n = torch_map().permute(0, 2, 3, 1)
        xyz = P.backproject_map(depth, k).permute(0, 2, 3, 1)
        ok = ~torch.isnan(xyz[..., 2])
        return xyz[ok], n[ok].nan_to_num_(0.0)

    ours = {"normals_map": lambda: P.normals(depth, k, jump_rel=rel, out=m_out),
            "normals_image": lambda: P.normal_image(depth, k, jump_rel=rel, out=i_out),
            "normals_points": lambda: P.backproject(depth, k, normals=True, jump_rel=rel, out=cloud),
            "points_without_normals": lambda: P.backproject(depth, k, with_index=True, out=cloud)}
    theirs = {"torch_map": torch_map, "torch_image": torch_image, "torch_points": torch_points}
    got, want = ours["normals_map"]().clone(), torch_map()
    same = (got.view(torch.int32) == want.view(torch.int32)).all(dim=1)
    agree = {"map_pixels_bitwise_equal": round(float(same.float().mean()), 5),
             "map_max_abs_difference": float((got - want).abs().nan_to_num_(0.0).max()),
             "pixels_with_a_normal": round(float((~torch.isnan(got[:, 0])).float().mean()), 5),
             "image_bytes_equal": round(float((ours["normals_image"]() == torch_image()).float().mean()), 5)}
    pc = ours["normals_points"]()
    agree["points_rows_bitwise_equal"] = round(float(
        (pc.normals.view(torch.int32) == torch_points()[1].view(torch.int32)).all(dim=1).float().mean()), 5)
    assert pc.count() == px

    before = clocks()
    variants = {**ours, **theirs}
    for fn in variants.values():  # time-based warm-up
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.warm_seconds:
            fn()
            torch.cuda.synchronize()
    # the boolean gather of torch_points synchronises with the host: it cannot be captured
    res = measure(variants, graphable=tuple(q for q in variants if q != "torch_points"))
    after = clocks()
    res["normals_points_fourth_launch"] = {q: round(res["normals_points"][q] - res["points_without_normals"][q], 2)
                                           for q in ("eager_us", "graph_us")}
    nbytes = {"normals_map": 16 * px, "normals_image": 7 * px, "normals_points_fourth_launch": 20 * px}
    for q, t in (("normals_map", "torch_map"), ("normals_image", "torch_image"), ("normals_points", "torch_points")):
        res[q]["torch_eager_over_ours_eager"] = round(res[t]["eager_us"] / res[q]["eager_us"], 2)
        if "graph_us" in res[t]:
            res[q]["torch_graph_over_ours_graph"] = round(res[t]["graph_us"] / res[q]["graph_us"], 2)
    for q, n in nbytes.items():
        res[q]["bytes"] = n
        res[q]["fraction_of_hbm_roof"] = round(n / (res[q]["graph_us"] * 1e-6) / HBM_BPS, 3)
    record = {"shape": [B, H, W], "jump_rel": rel, "agreement_with_torch": agree, **res,
              "warm_seconds_per_variant": a.warm_seconds, "clocks_before": before, "clocks_after": after}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
