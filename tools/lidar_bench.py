"""Timing record of lidar.project_points (with and without index) against the torch-op formulation on
the same device tensors in the same process (DESIGN.md section 5's conventions, as
tools/pointcloud_bench.py: HIP events around each call, 10 warm-up calls, the median of 150 calls taken
as three alternating blocks of 50 per variant; each variant also as a hipGraph of 20 back-to-back calls,
per call = replay / 20, which takes the host's launch gap out).

    python tools/lidar_bench.py [--batch 8] [--height 352] [--width 1216] [--rows 120000] [--json out.json]

The scan is seeded and synthetic: per image `rows` 4-float KITTI-layout rows (x, y, z, intensity), a
64-beam sweep of 360 degrees at 3 - 80 m, projected with KITTI's camera-2 matrix and the loaders' bottom
crop, so that about a fifth of the rows land in the image. The torch formulation is a batched matmul,
the elementwise passes and the boolean mask, a scatter_reduce_(amin) of the masked rows and the fix-up
of the empty pixels; the mask index waits for the host to learn the count, so it cannot be captured and
is timed eagerly only, that wait included (it is part of its cost). A second torch variant avoids the
wait by sending the rows that are not valid to one dump element behind the plane; it can be captured,
but every such row then contends for that element. Neither has an index or a defined winner between
ties. The matmul fuses and reorders the sums, so the planes are compared by the share of equal pixels.
Fill + resolve move 12 B per pixel without the index (4 written, 4 read, 4 written) and 24 B with it;
the roof is 8 TB/s. A record, not a gate."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nconv_pkg  # noqa: E402
from frames_bench import HBM_BPS  # noqa: E402
from pointcloud_bench import measure  # noqa: E402

# KITTI 2011_09_26: P_rect_02 and the velodyne pose (R_rect_00 taken as the identity)
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04], [1.480249e-02, 7.280733e-04, -9.998902e-01],
              [9.998621e-01, 7.523790e-03, 1.480755e-02]])
T = np.array([-4.069766e-03, -7.631618e-02, -2.717806e-01])


def synthetic_scan(rng, rows):
    az = rng.uniform(-math.pi, math.pi, rows)
    el = np.deg2rad(rng.uniform(-17.0, 2.0, rows))
    r = rng.uniform(3.0, 80.0, rows)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el),
                     rng.random(rows)], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    mod = nconv_pkg.load()
    Ld = mod.lidar
    dev = torch.device("cuda:0")
    B, H, W, rows = a.batch, a.height, a.width, a.rows
    px = B * H * W
    rng = np.random.default_rng(0)
    tr = np.eye(4)
    tr[:3, :3], tr[:3, 3] = R, T
    m64 = P2 @ tr
    m64[1] -= (375 - H) * m64[2]  # the loaders' bottom crop of a 375-row frame
    m = torch.from_numpy(m64.astype(np.float32)).to(dev)
    pts = torch.from_numpy(np.concatenate([synthetic_scan(rng, rows) for _ in range(B)])).to(dev)
    off = torch.arange(B + 1, dtype=torch.int32, device=dev) * rows
    out = {"depth": torch.empty(B, 1, H, W, device=dev), "index": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "workspace": torch.empty(Ld.workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)}
    out_plain = {"depth": torch.empty(B, 1, H, W, device=dev)}

    xyz = pts.view(B, rows, 4)[:, :, :3]
    mt, m3 = m[:, :3].t().contiguous().expand(B, 3, 3), m[:, 3].expand(B, 1, 3)
    first = (torch.arange(B, device=dev) * (H * W)).view(B, 1)
    plane = torch.empty(px + 1, device=dev)

    def torch_terms():
        p = torch.baddbmm(m3, xyz, mt)
        c = p[..., 2]
        u, v = torch.round(p[..., 0] / c), torch.round(p[..., 1] / c)
        ok = (c > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        return c, u, v, ok

    def torch_finish(pix, c):
        plane.fill_(float("inf"))
        plane.scatter_reduce_(0, pix, c, "amin")
        z = plane[:px]
        return torch.where(torch.isinf(z), 0.0, z).view(B, 1, H, W)

    def torch_project():  # boolean mask: a host synchronisation for the count
        c, u, v, ok = torch_terms()
        return torch_finish((first + v.long() * W + u.long())[ok], c[ok])

    def torch_project_nosync():  # rows that are not valid go to the dump element plane[px]
        c, u, v, ok = torch_terms()
        return torch_finish(torch.where(ok, first + v.long() * W + u.long(), px).view(-1), c.reshape(-1))

    d, ix = Ld.project_points(pts, off, m, (H, W), return_index=True, out=out)
    d0 = Ld.project_points(pts, off, m, (H, W), out=out_plain)
    assert torch.equal(d.view(torch.int32), d0.view(torch.int32))
    valid = int((ix >= 0).sum())
    won = ix[ix >= 0].long()
    assert bool((won // rows == torch.arange(B, device=dev).view(B, 1, 1).expand(B, H, W)[ix >= 0]).all())
    agree = float((torch_project() == d).float().mean())
    assert agree > 0.98 and torch.equal(torch_project(), torch_project_nosync()), agree
    variants = {
        "project": lambda: Ld.project_points(pts, off, m, (H, W), out=out_plain),
        "project_index": lambda: Ld.project_points(pts, off, m, (H, W), return_index=True, out=out),
        "torch_project": torch_project,
        "torch_project_nosync": torch_project_nosync,
    }
    res = measure(variants, graphable=("project", "project_index", "torch_project_nosync"))
    sweep = {"project": 12 * px, "project_index": 24 * px}
    for q, nbytes in sweep.items():
        res[q]["fill_resolve_fraction_of_hbm_roof"] = round(nbytes / (res[q]["graph_us"] * 1e-6) / HBM_BPS, 3)
        res[q]["torch_eager_over_ours_eager"] = round(res["torch_project"]["eager_us"] / res[q]["eager_us"], 2)
        res[q]["torch_eager_over_ours_graph"] = round(res["torch_project"]["eager_us"] / res[q]["graph_us"], 2)
        res[q]["torch_nosync_graph_over_ours_graph"] = round(res["torch_project_nosync"]["graph_us"] / res[q]["graph_us"], 2)
    record = {"shape": [B, H, W], "rows_per_image": rows, "pixels_hit": valid, "pixels_hit_share": round(valid / px, 4),
              "rows_in_image_share": round(float(torch_terms()[3].float().mean()), 4),
              "torch_equal_pixel_share": round(agree, 5), **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
