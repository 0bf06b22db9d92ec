"""GPU: nconv_voxel_merge bit for bit (torch.equal on every output, stats included) against the numpy restatement
of its rule (tests/voxel_cases.py). The shapes are the smallest at which each mechanism can go wrong, relative
to the kernel's constants: sort tile T, chunk C, the compaction tile, one and four radix passes."""
import numpy as np
import pytest
import torch

import voxel_cases as VC

pytestmark = pytest.mark.gpu

SENTINEL = {"xyz": -777.0, "normals": -777.0, "rgb": 77, "count": -7, "key": -7}
PER_POINT = ("rgb", "normals", "weights", "offsets", "poses")


def _dev(gpu, kw):
    """The case's arrays as device tensors (copies: the shared cases are read-only) and its grid."""
    t = {k: torch.tensor(np.asarray(kw[k])).to(gpu) for k in PER_POINT if kw.get(k) is not None}
    return torch.tensor(kw["xyz"]).to(gpu), t, dict(voxel=kw["voxel"], origin=kw["origin"], dims=kw["dims"])


def _out(gpu, cap, kw):
    out = {"xyz": torch.full((cap, 3), SENTINEL["xyz"], device=gpu), "count": torch.full((cap,), -7, dtype=torch.int32, device=gpu),
           "key": torch.full((cap,), -7, dtype=torch.int32, device=gpu)}
    if kw.get("rgb") is not None:
        out["rgb"] = torch.full((cap, 3), 77, dtype=torch.uint8, device=gpu)
    if kw.get("normals") is not None:
        out["normals"] = torch.full((cap, 3), SENTINEL["normals"], device=gpu)
    return out


def _equal(vm, want, cap):
    """Every output of the VoxelMap against the restatement's rows, and the rows past them untouched."""
    torch.cuda.synchronize()
    assert torch.equal(vm.stats.cpu(), torch.tensor(want["stats"]))
    kept = len(want["key"])
    assert kept == min(int(want["stats"][0]), cap)
    for name in ("xyz", "rgb", "normals", "count", "key"):
        got = getattr(vm, name)
        if want[name] is None:
            assert got is None
            continue
        assert got.shape[0] == cap
        g = got.cpu()
        assert torch.equal(g[:kept], torch.tensor(want[name])), name
        assert (g[kept:] == SENTINEL[name]).all(), f"{name}: rows past n_voxels were written"


def _check(nconv_amd, gpu, kw, max_voxels=None):
    xyz, t, grid = _dev(gpu, kw)
    n = xyz.shape[0]
    cap = min(n, int(np.prod(kw["dims"]))) if max_voxels is None else max_voxels
    want = VC.voxel_merge_ref(**{**kw, "max_voxels": cap})
    vm = nconv_amd.voxel_merge(xyz, t.get("offsets"), t.get("poses"), rgb=t.get("rgb"), normals=t.get("normals"),
                               weights=t.get("weights"), max_voxels=cap, out=_out(gpu, cap, kw), **grid)
    _equal(vm, want, cap)
    return vm, want


def test_no_point(nconv_amd, gpu):
    kw = dict(xyz=np.zeros((0, 3), np.float32), voxel=0.5, origin=(0.0, 0.0, 0.0), dims=(4, 4, 4))
    vm, _ = _check(nconv_amd, gpu, kw, max_voxels=3)
    assert vm.n_voxels() == 0 and not vm.truncated() and vm.points()[0].shape == (0, 3)
    _check(nconv_amd, gpu, kw)  # capacity 0 as well


def test_one_point(nconv_amd, gpu):
    kw = dict(xyz=np.array([[0.6, 1.2, 1.9]], np.float32), voxel=0.5, origin=(0.0, 0.0, 0.0), dims=(4, 4, 4),
              rgb=np.array([[1, 2, 3]], np.uint8), normals=np.array([[0, 0.6, -0.8]], np.float32))
    vm, want = _check(nconv_amd, gpu, kw)
    assert want["key"].tolist() == [(3 * 4 + 2) * 4 + 1] and vm.n_voxels() == 1


def test_all_points_outside(nconv_amd, gpu):
    kw = dict(VC.random_case(VC.T + 5, (7, 5, 3), seed=5))
    kw["origin"] = (100.0, 100.0, 100.0)
    _, want = _check(nconv_amd, gpu, kw)
    assert want["stats"].tolist() == [0, 0, VC.T + 5, 0]


@pytest.mark.parametrize("dims", [(7, 5, 3), (300, 300, 300), (1, 1, 1), (256, 1, 1), (257, 1, 1)],
                         ids=["one_pass_many_ties", "four_passes_singletons", "no_pass", "eight_bits", "nine_bits"])
def test_random_points_across_tiles_and_chunks(nconv_amd, gpu, dims):
    """N = 3 T + 7: runs that cross sort-tile and chunk boundaries; dims picks the number of radix passes."""
    _, want = _check(nconv_amd, gpu, VC.random_case(3 * VC.T + 7, dims))
    assert want["stats"][1] > 2 * VC.T


def test_more_rows_than_one_compaction_tile(nconv_amd, gpu):
    _check(nconv_amd, gpu, VC.random_case(2 * VC.PREP + 11, (16, 16, 4), seed=6))


def test_every_point_in_one_voxel_spans_chunks(nconv_amd, gpu):
    _, want = _check(nconv_amd, gpu, VC.one_voxel_case(5 * VC.C + 3))
    assert want["stats"].tolist() == [1, 5 * VC.C + 3, 0, 0]


def test_runs_that_end_exactly_on_a_chunk_boundary(nconv_amd, gpu):
    """Two cells of exactly C and 2 C points: heads at positions 0 and C, the second run through two whole chunks."""
    n = 3 * VC.C
    xyz = np.full((n, 3), 0.25, np.float32)
    xyz[VC.C:, 0] = 1.25
    xyz += np.random.default_rng(8).uniform(0, 0.5, size=(n, 3)).astype(np.float32)
    kw = dict(xyz=xyz, voxel=1.0, origin=(0.0, 0.0, 0.0), dims=(2, 1, 1))
    _, want = _check(nconv_amd, gpu, kw)
    assert want["count"].tolist() == [VC.C, 2 * VC.C]


def test_faces_negative_floor_nan_inf_and_weights(nconv_amd, gpu):
    _, want = _check(nconv_amd, gpu, VC.edge_case())
    assert want["stats"][2] == 14 and VC.INT32_MAX in want["count"].tolist()


@pytest.mark.parametrize("case", [VC.segment_case, VC.truncated_segment_case], ids=["rows_beyond", "truncated"])
def test_three_segments_with_poses(nconv_amd, gpu, case):
    _, want = _check(nconv_amd, gpu, case())
    assert want["stats"][0] > 100 and want["stats"][1] > 2 * VC.T  # tests/test_voxel_cpu.py: both segments land inside


def test_rgb_half_way_means_round_to_even(nconv_amd, gpu):
    vm, _ = _check(nconv_amd, gpu, VC.half_case())
    assert vm.rgb.cpu().tolist() == [[0] * 3, [2] * 3, [255] * 3]


def test_normals_cancel_and_ignore_missing_ones(nconv_amd, gpu):
    vm, _ = _check(nconv_amd, gpu, VC.normals_case())
    n = vm.normals.cpu()
    assert n[0].tolist() == [0, 0, 0] and torch.equal(n[1], torch.tensor(VC.normals_case()["normals"][3]))


def test_capacity_below_the_number_of_voxels(nconv_amd, gpu):
    kw = VC.random_case(3 * VC.T + 7, (7, 5, 3))
    vm, want = _check(nconv_amd, gpu, kw, max_voxels=40)
    assert want["stats"][0] > 40 and vm.truncated() and vm.n_voxels() == want["stats"][0]
    assert vm.points()[0].shape == (40, 3)


def test_strided_rows(nconv_amd, gpu):
    """xyz, rgb and normals as column slices of wider buffers."""
    kw = VC.random_case(VC.T + 9, (7, 5, 3), seed=9)
    xyz, t, grid = _dev(gpu, kw)
    n = xyz.shape[0]
    wide = torch.zeros(n, 7, device=gpu)
    wide[:, 1:4] = xyz
    wn = torch.zeros(n, 5, device=gpu)
    wn[:, 2:5] = t["normals"]
    wc = torch.zeros(n, 4, dtype=torch.uint8, device=gpu)
    wc[:, :3] = t["rgb"]
    vm = nconv_amd.voxel_merge(wide[:, 1:4], rgb=wc[:, :3], normals=wn[:, 2:5], weights=t["weights"], **grid)
    cap = vm.capacity
    want = VC.voxel_merge_ref(**kw)
    torch.cuda.synchronize()
    k = len(want["key"])
    assert torch.equal(vm.stats.cpu(), torch.tensor(want["stats"]))
    for name in ("xyz", "rgb", "normals", "count", "key"):
        assert torch.equal(getattr(vm, name).cpu()[:k], torch.tensor(want[name])), name
    assert cap == min(n, 7 * 5 * 3)


@pytest.mark.parametrize("case", [VC.segment_case, lambda: VC.one_voxel_case(5 * VC.C + 3)], ids=["segments", "one_voxel"])
def test_two_runs_give_identical_outputs(nconv_amd, gpu, case):
    """Many ties and runs across chunks (105 cells for 664 points), and one run through six chunks."""
    kw = case()
    xyz, t, grid = _dev(gpu, kw)
    runs = []
    for _ in range(2):
        vm = nconv_amd.voxel_merge(xyz, t.get("offsets"), t.get("poses"), rgb=t["rgb"], normals=t["normals"],
                                   weights=t["weights"], max_voxels=105, out=_out(gpu, 105, kw), **grid)
        torch.cuda.synchronize()
        runs.append([x.clone() for x in (vm.xyz, vm.rgb, vm.normals, vm.count, vm.key, vm.stats)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert int(runs[0][5][0]) > 0 and int(runs[0][5][1]) > 2 * VC.T  # there was something to sort and to sum


def test_merger_under_torch_cuda_graph(nconv_amd, gpu):
    n, dims = 3 * VC.T + 7, (7, 5, 3)
    cases = [VC.random_case(n, dims, seed=s) for s in (11, 12)]
    _, t0, grid = _dev(gpu, cases[0])
    merger = nconv_amd.VoxelMerger(n, dims, voxel=grid["voxel"], origin=grid["origin"], rgb=True, normals=True, device=gpu)
    xyz = torch.zeros(n, 3, device=gpu)
    rgb, nrm, w = torch.zeros_like(t0["rgb"]), torch.zeros_like(t0["normals"]), torch.ones_like(t0["weights"])
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        merger(xyz, rgb=rgb, normals=nrm, weights=w)  # warm up outside the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vm = merger(xyz, rgb=rgb, normals=nrm, weights=w)
    for kw in cases:
        x, t, _ = _dev(gpu, kw)
        xyz.copy_(x), rgb.copy_(t["rgb"]), nrm.copy_(t["normals"]), w.copy_(t["weights"])
        graph.replay()
        torch.cuda.synchronize()
        eager = nconv_amd.voxel_merge(x, rgb=t["rgb"], normals=t["normals"], weights=t["weights"], **grid)
        torch.cuda.synchronize()
        k = int(eager.stats[0])
        assert torch.equal(vm.stats, eager.stats) and k > 0
        for name in ("xyz", "rgb", "normals", "count", "key"):
            assert torch.equal(getattr(vm, name)[:k], getattr(eager, name)[:k]), name
        want = VC.voxel_merge_ref(**kw)
        assert torch.equal(vm.xyz[:k].cpu(), torch.tensor(want["xyz"])) and torch.equal(vm.key[:k].cpu(), torch.tensor(want["key"]))


def test_add_is_the_rule_applied_twice(nconv_amd, gpu):
    kw = VC.random_case(3 * VC.T + 7, (7, 5, 3))
    first, second = VC.split_halves(kw)
    x1, t1, grid = _dev(gpu, first)
    x2, t2, _ = _dev(gpu, second)
    m1 = nconv_amd.voxel_merge(x1, rgb=t1["rgb"], normals=t1["normals"], weights=t1["weights"], **grid)
    cap = m1.capacity
    pc = nconv_amd.PointCloud(x2, t2["rgb"], None, torch.tensor([0, x2.shape[0]], dtype=torch.int32, device=gpu),
                              t2["normals"])
    m2 = m1.add(pc, weights=t2["weights"])
    want = VC.add_ref(VC.voxel_merge_ref(**first), cap, second)
    torch.cuda.synchronize()
    k = len(want["key"])
    assert torch.equal(m2.stats.cpu(), torch.tensor(want["stats"]))
    for name in ("xyz", "rgb", "normals", "count", "key"):
        assert torch.equal(getattr(m2, name).cpu()[:k], torch.tensor(want[name])), name
    # with poses: the identity for the map's segment, a real one for the cloud, given in that camera's frame
    pose = VC.segment_case()["poses"][2]
    moved = dict(second, xyz=VC.to_camera(second["xyz"], pose))
    pc = nconv_amd.PointCloud(torch.tensor(moved["xyz"]).to(gpu), t2["rgb"], None, pc.offsets, t2["normals"])
    m3 = m1.add(pc, torch.tensor(pose[None]).to(gpu), weights=t2["weights"])
    want = VC.add_ref(VC.voxel_merge_ref(**first), cap, moved, poses=pose[None])
    torch.cuda.synchronize()
    k = len(want["key"])
    assert want["stats"][1] > m1.n_voxels() + 0.8 * x2.shape[0]  # the cloud's points land in the map
    assert torch.equal(m3.stats.cpu(), torch.tensor(want["stats"]))
    for name in ("xyz", "rgb", "normals", "count", "key"):
        assert torch.equal(getattr(m3, name).cpu()[:k], torch.tensor(want[name])), name


def test_pointcloud_from_backproject_goes_straight_in(nconv_amd, gpu):
    rng = np.random.default_rng(13)
    B, H, W = 2, 24, 40
    depth = rng.uniform(2.0, 12.0, size=(B, 1, H, W)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.2] = 0
    color = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    k = np.array([[30.0, 0, 19.5], [0, 30.0, 11.5], [0, 0, 1]], np.float32)
    poses = np.stack([np.eye(3, 4, dtype=np.float32), VC._pose(rng, (1.0, 0.0, 0.0))])
    pc = nconv_amd.backproject(torch.tensor(depth).to(gpu), torch.tensor(k).to(gpu), color=torch.tensor(color).to(gpu),
                               normals=True)
    grid = dict(voxel=0.5, origin=(-10.0, -6.0, 0.0), dims=(40, 24, 26))
    vm = nconv_amd.voxel_merge(pc, poses=torch.tensor(poses).to(gpu), **grid)
    torch.cuda.synchronize()
    n = pc.count()
    assert 0 < n < B * H * W and vm.capacity == B * H * W
    want = VC.voxel_merge_ref(pc.xyz.cpu().numpy(), pc.offsets.cpu().numpy(), poses, rgb=pc.rgb.cpu().numpy(),
                              normals=pc.normals.cpu().numpy(), **grid)
    kept = len(want["key"])
    assert torch.equal(vm.stats.cpu(), torch.tensor(want["stats"])) and want["stats"][2] >= B * H * W - n
    assert 0 < kept < n
    for name in ("xyz", "rgb", "normals", "count", "key"):
        assert torch.equal(getattr(vm, name).cpu()[:kept], torch.tensor(want[name])), name
