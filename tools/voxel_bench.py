"""Timing record of voxel_merge (nconv_voxel_merge, 5 + 2 P launches) against the torch composition of the same
map (torch.unique(return_inverse=True) + index_add_) and against a plain device copy of the bytes the merge
must touch, with tools/frames_bench.py's conventions (HIP events around each call, 10 warm-up calls, the median
of three alternating blocks per variant; the library call is also timed as a hipGraph of 20 back-to-back calls,
per call = replay / 20).

    python tools/voxel_bench.py [--batch 8] [--height 352] [--width 1216] [--voxel 0.1] [--json out.json]

B clouds from backproject (colours and normals) of a synthetic street: a road plane, two facades and a far wall,
with centimetre noise; one pose per image, 1 m apart along the driving direction. The torch composition is timed
eagerly only, its synchronisation included (the size of its result depends on the data: that is part of its
cost); it uses float atomics, so its sums differ from run to run, and it is compared with a tolerance. The copy
moves inputs + outputs bytes once (N * 27 read, n_voxels * 35 written in the merge). A record, not a gate."""
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


def street(B, H, W, k, dev, g):
    """Depth (B, 1, H, W) of a road 1.6 m below the camera, facades 6 m left and right, a wall 45 m ahead."""
    j = torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
    i = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
    rx, ry = (j - k[0, 2]) / k[0, 0], (i - k[1, 2]) / k[1, 1]
    inf = torch.full((H, W), 1e9)
    z = torch.minimum(torch.where(ry > 1e-3, 1.6 / ry, inf), torch.where(rx.abs() > 1e-3, 6.0 / rx.abs(), inf))
    z = torch.minimum(z, torch.full((H, W), 45.0))
    z = z[None, None] + torch.randn(B, 1, H, W, generator=g) * 0.01
    return z.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    m = nconv_pkg.load()
    dev = torch.device("cuda:0")
    B, H, W, voxel = a.batch, a.height, a.width, a.voxel
    g = torch.Generator().manual_seed(0)
    k = torch.tensor([[721.5, 0.0, W / 2 - 0.5], [0.0, 721.5, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    depth = street(B, H, W, k, dev, g)
    color = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    pc = m.backproject(depth, k.to(dev), color=color, normals=True, z_max=60.0)
    poses = torch.eye(3, 4)[None].repeat(B, 1, 1)
    poses[:, 2, 3] = torch.arange(B, dtype=torch.float32)  # 1 m apart
    poses = poses.to(dev)
    origin, extent = (-8.0, -4.0, 0.0), (16.0, 8.0, 56.0)
    dims = tuple(int(round(e / voxel)) for e in extent)
    N = pc.capacity
    merger = m.VoxelMerger(N, dims, voxel=voxel, origin=origin, max_voxels=N, rgb=True, normals=True, device=dev)

    def ours():
        return merger(pc, poses=poses)

    o = torch.tensor(origin, device=dev)
    nd = torch.tensor(dims, device=dev)
    vox = torch.full((1,), voxel, device=dev)  # a device divisor: a true division, not a product with 1 / voxel
    rows = torch.arange(N, device=dev, dtype=torch.int32)
    seg = torch.bucketize(rows, pc.offsets[1:], right=True).clamp_(max=B - 1)

    def torch_merge():
        R, t = poses[seg, :, :3], poses[seg, :, 3]
        p = torch.einsum("nij,nj->ni", R, pc.xyz) + t
        f = torch.floor((p - o) / vox)
        inside = ((f >= 0) & (f < nd)).all(1) & (rows < pc.offsets[B])  # rows past the count are not points
        p, c = p[inside], f[inside].long()
        key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
        uniq, inv = torch.unique(key, return_inverse=True)  # synchronises: the size depends on the data
        cnt = torch.zeros(len(uniq), device=dev).index_add_(0, inv, torch.ones(len(inv), device=dev))
        xyz = torch.zeros(len(uniq), 3, device=dev).index_add_(0, inv, p) / cnt[:, None]
        rgb = torch.zeros(len(uniq), 3, device=dev).index_add_(0, inv, pc.rgb[inside].float()) / cnt[:, None]
        nrm = torch.zeros(len(uniq), 3, device=dev).index_add_(0, inv, torch.einsum("nij,nj->ni", R, pc.normals)[inside])
        return uniq, xyz, rgb, nrm, cnt

    vm = ours()
    uniq, xyz_t, _, _, cnt_t = torch_merge()
    torch.cuda.synchronize()
    nv, n_in, n_drop, _ = vm.host_stats()
    same = nv == len(uniq) and torch.equal(vm.key[:nv].long(), uniq) and torch.equal(vm.count[:nv].float(), cnt_t)
    diff = float((vm.xyz[:nv] - xyz_t).abs().max()) if same else None  # recorded, not asserted: a record, not a gate

    nbytes = N * 27 + nv * 35
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def copy():
        dst.copy_(src)

    variants = {"voxel_merge": ours, "torch_unique_index_add": torch_merge, "copy": copy}
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    eager = {name: [] for name in variants}
    for _ in range(3):
        for name, fn in variants.items():
            eager[name] += _eager_block(fn, 20)
    res = {name: {"eager_us": round(statistics.median(v), 2)} for name, v in eager.items()}
    for name in ("voxel_merge", "copy"):  # the torch composition synchronises: it cannot be captured
        graph = _graph_of(variants[name])
        times = [t / GRAPH_CALLS for _ in range(3) for t in _eager_block(graph.replay, 10)]
        res[name]["graph_us"] = round(statistics.median(times), 2)
    res["launches"] = m.voxelmap.launches(dims)
    res["ratio_torch_eager_over_ours_graph"] = round(res["torch_unique_index_add"]["eager_us"] / res["voxel_merge"]["graph_us"], 2)
    res["ratio_ours_graph_over_copy_graph"] = round(res["voxel_merge"]["graph_us"] / res["copy"]["graph_us"], 2)
    res["keys_and_counts_equal_torch"], res["max_abs_diff_vs_torch_m"] = bool(same), diff
    res["points"], res["n_inside"], res["n_dropped"], res["n_voxels"] = N, n_in, n_drop, nv
    res["copy_bytes"] = nbytes
    res["workspace_mb"] = round(merger.out["workspace"].numel() / 2 ** 20, 1)
    res["shape"], res["dims"], res["voxel"] = [B, H, W], list(dims), voxel
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
