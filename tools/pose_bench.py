"""Timing record of the pose alignment (pose.py: nconv_pose_normal_eq + nconv_pose_update) against the same
Gauss-Newton iteration composed from torch ops and against a plain copy of the planes one iteration must touch,
on the same device tensors in the same process (tools/pointcloud_bench.py's measure: HIP events around each
call, 10 warm-up calls, the median of 150 calls taken as three alternating blocks of 50 per variant; each
graphable variant also as a hipGraph of 20 back-to-back calls, per call = replay / 20).

    python tools/pose_bench.py [--batch 8] [--height 352] [--width 1216] [--json out.json]

B = 8, C = 3, 352 x 1216; the sparse plane has 5 % of the pixels below row 100 (the IP-Basic bench's plane); the
source is a smooth random frame and the target its own warp (view_warp) by a dense depth and 1 m of forward
motion, so that the alignment has something to find.

  pose_iteration   one Gauss-Newton iteration: the two launches
  estimate_pose    PoseEstimator(levels = 3, iters = 8): 54 launches plus the pyramid's torch ops
  torch_iteration  the same iteration from torch ops: the projection, F.grid_sample for the value and for the two
                   slopes (central taps of the bilinear blend), the explicit 1 x 6 Jacobian, the masked sums as
                   matrix products in double and torch.linalg.solve (eager only: the solve synchronises)
  copy_floor       one copy of a (B, 7, H, W) fp32 tensor: depth, three target and three source planes, the
                   28 B/px an iteration must read at full density (the sparse plane lets the kernel skip most taps)
A record, not a gate."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nconv_pkg  # noqa: E402
from pointcloud_bench import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    mod = nconv_pkg.load()
    P = mod.pose
    dev = torch.device("cuda:0")
    B, H, W, C = a.batch, a.height, a.width, 3
    g = torch.Generator().manual_seed(0)
    coarse = torch.rand(B, 1, 6, 20, generator=g) * 55 + 5
    dense = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).to(dev)
    src = F.interpolate(torch.rand(B, C, 12, 40, generator=g) * 255, size=(H, W), mode="bicubic",
                        align_corners=True).clamp(0, 255).to(dev)
    k = torch.tensor([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]], device=dev)
    yaw = 0.01
    true = torch.tensor([[np.cos(yaw), 0.0, np.sin(yaw), 0.05], [0.0, 1.0, 0.0, -0.02],
                         [-np.sin(yaw), 0.0, np.cos(yaw), -1.0]], device=dev)  # the car moved 1 m forward
    m_true = mod.warp_projection(k, true).expand(B, 3, 4).contiguous()
    tgt = mod.view_warp(dense, k, src, m_true).contiguous()
    keep = torch.rand(B, 1, H, W, generator=g).to(dev) < 0.05
    keep[:, :, :100] = False
    depth = torch.where(keep, dense, torch.zeros_like(dense))

    # one iteration: the two launches on kept buffers
    buf = P._Buffers(B, H, W, 1, 1, dev)
    buf.state.copy_(torch.eye(3, 4, dtype=torch.float64, device=dev).expand(B, 3, 4))
    buf.pose.copy_(buf.state)
    buf.m[0].copy_(P.pose_projection(k, buf.state))
    opts = P._options(P.HUBER_DEFAULT, 1e-4, P.MIN_POINTS_DEFAULT)
    lv = dict(depth=depth, k=k, tgt=tgt, src=src, k_src=k, mask=None)
    d, _keep = P._descriptor(lv, buf, 0, *opts, 1e-3, None)
    lib, ws = mod._lib.lib(), mod._lib.ptr(buf.ws)

    def pose_iteration():
        st = mod._lib.stream_handle(dev)
        mod._lib.check(lib.nconv_pose_normal_eq(ctypes.byref(d), ws, buf.nbytes, st), "nconv_pose_normal_eq")
        mod._lib.check(lib.nconv_pose_update(ctypes.byref(d), ws, buf.nbytes, 0, 1, st), "nconv_pose_update")
        return buf.pose

    est = mod.PoseEstimator((H, W), B=B, C=C, levels=3, iters=8, device=dev)

    def estimate_pose():
        return est(depth, k, tgt, src)[0]

    jj = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ii = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    state = torch.eye(3, 4, device=dev).expand(B, 3, 4).contiguous()

    def torch_iteration():
        z = depth[:, 0]
        x = (jj - k[0, 2]) * z / k[0, 0]
        y = (ii - k[1, 2]) * z / k[1, 1]
        pp = state.view(B, 3, 4, 1, 1)
        X, Y, Z = (pp[:, r, 0] * x + pp[:, r, 1] * y + pp[:, r, 2] * z + pp[:, r, 3] for r in range(3))
        xn, yn, iz = X / Z, Y / Z, 1 / Z
        u, v = k[0, 0] * xn + k[0, 2], k[1, 1] * yn + k[1, 2]
        valid = (z > 1e-3) & (Z > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)

        def sample(du, dv):
            grid = torch.stack((2 * (u + du) / (W - 1) - 1, 2 * (v + dv) / (H - 1) - 1), dim=-1)
            grid = torch.where(valid[..., None], grid, torch.zeros_like(grid))
            return F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=True)

        s = sample(0, 0)
        dIu = (sample(0.5, 0) - sample(-0.5, 0))
        dIv = (sample(0, 0.5) - sample(0, -0.5))
        o = torch.zeros_like(xn)
        Ju = k[0, 0] * torch.stack((iz, o, -xn * iz, -xn * yn, 1 + xn * xn, -yn), dim=1)
        Jv = k[1, 1] * torch.stack((o, iz, -yn * iz, -(1 + yn * yn), xn * yn, xn), dim=1)
        J = dIu[:, :, None] * Ju[:, None] + dIv[:, :, None] * Jv[:, None]            # (B, C, 6, H, W)
        r = s - tgt
        ar = r.abs()
        w = torch.where(ar <= P.HUBER_DEFAULT, torch.ones_like(ar), P.HUBER_DEFAULT / ar) * valid[:, None]
        Jm = J.permute(0, 2, 1, 3, 4).reshape(B, 6, -1).double()
        wr = (w * r).reshape(B, 1, -1).double()
        Hm = (Jm * w.reshape(B, 1, -1).double()) @ Jm.transpose(1, 2)
        b = (Jm * wr).sum(dim=2)
        Hm = Hm + 1e-4 * torch.diag_embed(torch.diagonal(Hm, dim1=1, dim2=2))
        return torch.linalg.solve(Hm, -b)

    planes = torch.rand(B, 7, H, W, generator=g).to(dev)
    planes_out = torch.empty_like(planes)

    def copy_floor():
        return planes_out.copy_(planes)

    pose = est(depth, k, tgt, src)[0].clone()
    torch.cuda.synchronize()
    err_t = (pose[:, :, 3].double() - true[:, 3].double()).norm(dim=1)
    variants = {"pose_iteration": pose_iteration, "estimate_pose": estimate_pose, "torch_iteration": torch_iteration,
                "copy_floor": copy_floor}
    res = measure(variants, graphable=("pose_iteration", "estimate_pose", "copy_floor"))
    res["torch_iteration"]["eager_over_pose_iteration_eager"] = round(
        res["torch_iteration"]["eager_us"] / res["pose_iteration"]["eager_us"], 2)
    res["copy_floor"]["graph_over_pose_iteration_graph"] = round(
        res["copy_floor"]["graph_us"] / res["pose_iteration"]["graph_us"], 2)
    record = {"shape": [B, C, H, W], "samples_per_image": int(est.info["n"][0, :, -1].float().mean()),
              "status": est.info["status"].cpu().numpy().tolist(),
              "translation_error_m_after_estimate": [float(f"{e:.3g}") for e in err_t.cpu().numpy()],
              "cost_first_last": [float(f"{float(est.info['cost'][-1, 0, 0]):.4g}"),
                                  float(f"{float(est.info['cost'][0, 0, -1]):.4g}")], **res}
    line = json.dumps(record)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
