"""CPU: the numpy restatement of the voxel-grid merge (tests/voxel_cases.py) against an independent brute-force
reference (a dict of cells, math.fsum of exact products, divided in float64); its properties; a merged map merged
again; VoxelMap.add restated; the Python argument checks; the two entry points exported, declared and bound with
the C struct's layout under an unchanged ABI number, and every malformed call refused on the host with -22."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import host_harness
import voxel_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
NEW = ("nconv_voxel_merge_workspace_bytes", "nconv_voxel_merge")
F32 = np.float32


# ---- the brute-force reference -----------------------------------------------------------------------
def brute(kw):
    """{key: (W, exact-sum means of xyz as float64, exact rgb means as Fractions, rows)} and the stats; the
    world point and the cell by scalar np.float32 steps of its own."""
    xyz, off, poses = kw["xyz"], kw.get("offsets"), kw.get("poses")
    w_all, rgb, nrm = kw.get("weights"), kw.get("rgb"), kw.get("normals")
    o, v, dims = [F32(t) for t in kw["origin"]], F32(kw["voxel"]), kw["dims"]
    cells, n_in = {}, 0
    for i in range(len(xyz)):
        s = 0
        if off is not None:
            s = -1
            for k in range(len(off) - 1):
                if off[k] <= i < off[k + 1]:
                    s = k
        w = 1 if w_all is None else int(w_all[i])
        x = [F32(t) for t in xyz[i]]
        nv = None if nrm is None else [F32(t) for t in nrm[i]]
        with np.errstate(all="ignore"):
            if poses is not None and s >= 0:
                m = poses[s]
                x = [((m[k, 0] * x[0] + m[k, 1] * x[1]) + m[k, 2] * x[2]) + m[k, 3] for k in range(3)]
                if nv is not None:
                    nv = [(m[k, 0] * nv[0] + m[k, 1] * nv[1]) + m[k, 2] * nv[2] for k in range(3)]
            f = [np.floor((x[a] - o[a]) / v) for a in range(3)]
        if s < 0 or w <= 0 or not all(f[a] >= 0 and f[a] < F32(dims[a]) for a in range(3)):
            continue
        n_in += 1
        key = (int(f[2]) * dims[1] + int(f[1])) * dims[0] + int(f[0])
        cells.setdefault(key, []).append((w, [float(t) for t in x], None if rgb is None else [int(c) for c in rgb[i]],
                                          None if nv is None else [float(t) for t in nv]))
    out = {}
    for key, pts in cells.items():
        W = sum(t[0] for t in pts)

        def exact(j, a):  # w = hi * 2^16 + lo: both products with an fp32 value are exact in double
            return math.fsum([(t[0] >> 16) * 65536.0 * t[j][a] for t in pts] + [(t[0] & 65535) * t[j][a] for t in pts])

        mean = [exact(1, a) / W for a in range(3)]
        col = None if rgb is None else [Fraction(sum(t[0] * t[2][a] for t in pts), W) for a in range(3)]
        nsum = None if nrm is None else ([exact(3, a) for a in range(3)],
                                         math.fsum(t[0] * abs(t[3][a]) for t in pts for a in range(3)))
        out[key] = (W, mean, col, len(pts), nsum)
    return out, [len(out), n_in, len(xyz) - n_in, 0]


def ulps(a, b):
    """The distance of two finite fp32 in units in the last place."""
    def lin(x):
        i = np.asarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(lin(a) - lin(b))


CASES = {"random_7x5x3": lambda: VC.random_case(3 * VC.T + 7, (7, 5, 3)),
         "random_300": lambda: VC.random_case(3 * VC.T + 7, (300, 300, 300)),
         "one_voxel": lambda: VC.one_voxel_case(5 * VC.C + 3), "edges": VC.edge_case, "segments": VC.segment_case,
         "truncated_segments": VC.truncated_segment_case, "halves": VC.half_case, "normals": VC.normals_case}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_brute_force_reference(name):
    """Keys, counts and stats equal; centroids within 1 fp32 ulp (a sequential double sum is off by at most
    n 2^-53 sum |w p|, which moves the fp32 rounding only next to a tie); rgb equal, the reference itself showing
    that no exact mean lies within n 2^-50 of a half other than the exact halves, which round to even; normals
    within 1e-6 per component of the exactly summed direction: the three roundings of the sums to fp32 and the
    five of the normalisation are each below 2^-24 of a unit vector's length (under 5e-7 together), and the double
    sums add at most n 2^-53 sum |w n| / length < 2e-10 where the length is above a thousandth of sum |w n|."""
    kw = CASES[name]()
    got = VC.voxel_merge_ref(**kw)
    cells, stats = brute(kw)
    assert got["stats"].tolist() == stats
    keys = sorted(cells)
    assert got["key"].tolist() == keys
    for m, key in enumerate(keys):
        W, mean, col, n, nsum = cells[key]
        if nsum is not None:
            # the direction of the exactly summed rotated normals; where they cancel to less than a thousandth of
            # their summed length the direction is rounding's and only an exact zero is checked
            length = math.sqrt(sum(t * t for t in nsum[0]))
            if length == 0:
                assert got["normals"][m].tolist() == [0, 0, 0], (name, key)
            elif length > 1e-3 * nsum[1]:
                assert np.abs(got["normals"][m] - np.asarray(nsum[0]) / length).max() < 1e-6, (name, key)
        assert got["count"][m] == min(W, VC.INT32_MAX)
        assert ulps(got["xyz"][m], np.asarray(mean).astype(F32)).max() <= 1, (name, key)
        if col is not None:
            for a in range(3):
                frac = col[a] - math.floor(col[a])
                d = abs(frac - Fraction(1, 2))
                assert d == 0 or d > Fraction(n, 2 ** 50), (name, key, "a colour mean next to a half")
                want = math.floor(col[a]) + (1 if frac > Fraction(1, 2) else 0)
                if d == 0:
                    want = math.floor(col[a]) + (math.floor(col[a]) & 1)  # half to even
                assert got["rgb"][m][a] == want, (name, key)


@pytest.mark.parametrize("name", sorted(CASES))
def test_properties(name):
    kw = CASES[name]()
    got = VC.voxel_merge_ref(**kw)
    inside = VC.classify(kw["xyz"], kw.get("offsets"), kw.get("poses"), kw.get("weights"), kw["voxel"], kw["origin"],
                         kw["dims"])[0]
    w = np.ones(len(kw["xyz"]), np.int64) if kw.get("weights") is None else kw["weights"].astype(np.int64)
    assert (np.diff(got["key"].astype(np.int64)) > 0).all()
    assert got["stats"][1] + got["stats"][2] == len(kw["xyz"]) and got["stats"][3] == 0
    assert got["stats"][0] == len(got["key"]) and got["stats"][1] == inside.sum()
    if name != "edges":  # its big weights saturate count
        assert got["count"].astype(np.int64).sum() == w[inside].sum()


def test_the_named_cases_hold_what_they_promise():
    e = VC.edge_case()
    inside = VC.classify(e["xyz"], None, None, e["weights"], e["voxel"], e["origin"], e["dims"])[0]
    assert inside.tolist() == [True, True] + [False] * 14 + [True] * 4
    got = VC.voxel_merge_ref(**e)
    assert got["key"][0] == 0 and got["count"][0] == 2 and VC.INT32_MAX in got["count"].tolist()
    assert got["key"][-1] == 4 * 3 * 2 - 1  # the last float below the far corner: the last cell
    h = VC.voxel_merge_ref(**VC.half_case())
    assert h["rgb"].tolist() == [[0] * 3, [2] * 3, [255] * 3]
    n = VC.voxel_merge_ref(**VC.normals_case())["normals"]
    assert n[0].tolist() == [0, 0, 0] and np.array_equal(n[1], VC.normals_case()["normals"][3])
    assert np.allclose(n[2], [math.sqrt(0.5), math.sqrt(0.5), 0], atol=1e-7)
    s, t = VC.segment_case(), VC.truncated_segment_case()
    assert s["offsets"][1] == s["offsets"][2] and s["offsets"][3] < len(s["xyz"]) < t["offsets"][3]
    for case, none in ((s, 40), (t, 0)):
        inside, key, _, seg = VC.classify(case["xyz"], case["offsets"], case["poses"], case["weights"], case["voxel"],
                                          case["origin"], case["dims"])
        assert (seg == -1).sum() == none and (seg == 1).sum() == 0 and not inside[seg == -1].any()
        for k in (0, 2):  # every non-empty segment brings most of its points into the box
            assert inside[seg == k].sum() > 0.8 * (seg == k).sum() > 0
        assert len(set(key[inside & (seg == 0)]) & set(key[inside & (seg == 2)])) > 50  # cells that mix segments
        # the poses matter: with segment 2's pose on segment 0's rows nothing of them comes back
        wrong = dict(case, poses=case["poses"][[2, 1, 0]])
        assert VC.voxel_merge_ref(**wrong)["stats"][1] < 0.2 * inside.sum()
    assert VC.voxel_merge_ref(**t)["stats"][1] > VC.voxel_merge_ref(**s)["stats"][1]  # the 40 last rows count now
    one = VC.voxel_merge_ref(**VC.one_voxel_case(5 * VC.C + 3))
    assert one["stats"].tolist() == [1, 5 * VC.C + 3, 0, 0]
    r = VC.voxel_merge_ref(**VC.random_case(3 * VC.T + 7, (300, 300, 300)))
    assert VC.passes((300, 300, 300)) == 4 and VC.passes((7, 5, 3)) == 1 and VC.passes((1, 1, 1)) == 0
    assert r["stats"][0] > 0.95 * r["stats"][1]  # mostly singleton runs
    assert 3 * VC.T + 7 > VC.PREP // 2 and (VC.T, VC.C, VC.DIGIT, VC.BLOCKS) == (256, 256, 8, 256)


def test_tree_is_chunks_then_pieces():
    """A run across three chunks of 4: ((t0 + t1 + t2 from 0) is not what the tree gives where rounding shows."""
    terms = np.array([[1e16], [1.0], [1.0], [1.0], [1.0], [1.0], [-1e16]])
    assert VC._tree_sum(terms, 0, 7, 4)[0] == ((((0.0 + 1e16) + 1.0) + 1.0) + 1.0) + (((0.0 + 1.0) + 1.0) + -1e16)
    assert VC._tree_sum(terms, 1, 6, 4)[0] == 5.0 and VC._tree_sum(terms, 3, 5, 4)[0] == 2.0


def test_merging_a_merged_map_keeps_keys_and_counts():
    kw = VC.random_case(3 * VC.T + 7, (7, 5, 3))
    a = VC.voxel_merge_ref(**kw)
    b = VC.voxel_merge_ref(a["xyz"], voxel=kw["voxel"], origin=kw["origin"], dims=kw["dims"], rgb=a["rgb"],
                           normals=a["normals"], weights=a["count"])
    assert np.array_equal(a["key"], b["key"]) and np.array_equal(a["count"], b["count"])
    assert b["stats"].tolist() == [len(a["key"])] * 2 + [0, 0]
    assert np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["rgb"], b["rgb"])  # w x / w of one point


def test_add_in_two_halves_is_the_rule_applied_twice():
    kw = VC.random_case(3 * VC.T + 7, (7, 5, 3))
    first, second = VC.split_halves(kw)
    m1 = VC.voxel_merge_ref(**first)
    cap = min(len(first["xyz"]), 7 * 5 * 3)
    both = VC.add_ref(m1, cap, second)
    whole = VC.voxel_merge_ref(**kw)
    assert np.array_equal(both["key"], whole["key"]) and np.array_equal(both["count"], whole["count"])
    assert both["stats"][2] == whole["stats"][2] - first["xyz"].shape[0] + m1["stats"][1] + cap - len(m1["key"])
    assert np.abs(both["xyz"] - whole["xyz"]).max() < 1e-5  # close, and in general not equal
    assert np.abs(both["rgb"].astype(int) - whole["rgb"].astype(int)).max() <= 1


def test_add_with_a_pose_brings_the_cloud_into_the_map():
    kw = VC.random_case(3 * VC.T + 7, (7, 5, 3))
    first, second = VC.split_halves(kw)
    pose = VC.segment_case()["poses"][2]
    second = dict(second, xyz=VC.to_camera(second["xyz"], pose))
    m1 = VC.voxel_merge_ref(**first)
    both = VC.add_ref(m1, 105, second, poses=pose[None])
    assert both["stats"][1] > len(m1["key"]) + 0.8 * len(second["xyz"])
    assert both["count"].astype(np.int64).sum() > m1["count"].astype(np.int64).sum() + 0.8 * len(second["xyz"])
    assert VC.add_ref(m1, 105, second)["stats"][1] < len(m1["key"]) + 0.2 * len(second["xyz"])  # without it: lost


# ---- the Python layer ---------------------------------------------------------------------------------
def test_python_refuses_bad_arguments(nconv_amd):
    vm = nconv_amd.voxel_merge
    g = dict(voxel=0.1, origin=(0, 0, 0), dims=(4, 4, 4))
    x = torch.zeros(8, 3)
    with pytest.raises(TypeError, match="xyz: expected torch.float32"):
        vm(x.double(), **g)
    with pytest.raises(TypeError, match="rgb: expected torch.uint8"):
        vm(x, rgb=x, **g)
    with pytest.raises(TypeError, match="weights: expected torch.int32"):
        vm(x, weights=torch.ones(8), **g)
    with pytest.raises(TypeError, match="offsets: expected torch.int32"):
        vm(x, torch.tensor([0, 8]), **g)
    with pytest.raises(ValueError, match=r"xyz must be \(N, 3\)"):
        vm(torch.zeros(8, 4), **g)
    with pytest.raises(ValueError, match="normals has 7 rows, xyz 8"):
        vm(x, normals=torch.zeros(7, 3), **g)
    with pytest.raises(ValueError, match="no unit innermost stride"):
        vm(torch.zeros(3, 8).t(), **g)
    with pytest.raises(ValueError, match="no unit innermost stride"):
        vm(torch.zeros(8, 6)[:, ::2], **g)
    with pytest.raises(ValueError, match="weights must be a contiguous"):
        vm(x, weights=torch.ones(16, dtype=torch.int32)[::2], **g)
    with pytest.raises(ValueError, match="2\\^31 cells"):
        vm(x, voxel=0.1, origin=(0, 0, 0), dims=(2048, 1024, 1024))
    with pytest.raises(ValueError, match="dims must be three values >= 1"):
        vm(x, voxel=0.1, origin=(0, 0, 0), dims=(4, 0, 4))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel = .* must be > 0"):
            vm(x, voxel=bad, origin=(0, 0, 0), dims=(4, 4, 4))
    with pytest.raises(ValueError, match="origin must be three finite"):
        vm(x, voxel=0.1, origin=(0, float("nan"), 0), dims=(4, 4, 4))
    off = torch.tensor([0, 4, 8], dtype=torch.int32)
    with pytest.raises(ValueError, match=r"poses must be \(2, 3, 4\)"):
        vm(x, off, torch.zeros(3, 3, 4), **g)
    with pytest.raises(ValueError, match=r"poses must be \(1, 3, 4\)"):
        vm(x, None, torch.zeros(2, 3, 4), **g)
    with pytest.raises(ValueError, match="offsets must be a contiguous"):
        vm(x, torch.zeros(1, dtype=torch.int32), **g)
    with pytest.raises(ValueError, match="max_voxels"):
        vm(x, max_voxels=-1, **g)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        vm(x, **g)
    pc = nconv_amd.PointCloud(x, None, None, off)
    with pytest.raises(ValueError, match="a PointCloud supplies offsets"):
        vm(pc, off, **g)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        vm(pc, **g)
    with pytest.raises(ValueError, match="too large"):
        nconv_amd.voxelmap.workspace_bytes(2 ** 31, (4, 4, 4))
    assert nconv_amd.voxelmap.launches((1, 1, 1)) == 5 and nconv_amd.voxelmap.launches((7, 5, 3)) == 7
    assert nconv_amd.voxelmap.launches((300, 300, 300)) == 13 and nconv_amd.voxelmap.launches((2, 1, 1)) == 7
    assert nconv_amd.voxelmap.launches((256, 1, 1)) == 7 and nconv_amd.voxelmap.launches((257, 1, 1)) == 9
    for name in ("VoxelMap", "VoxelMerger", "voxel_merge"):
        assert name in nconv_amd.__all__ and hasattr(nconv_amd, name)


def test_voxelmap_host_helpers(nconv_amd):
    xyz = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    m = nconv_amd.VoxelMap(xyz, None, None, torch.ones(5, dtype=torch.int32), torch.arange(5, dtype=torch.int32),
                           torch.tensor([7, 9, 1, 0], dtype=torch.int32), 0.1, (0.0, 0.0, 0.0), (4, 4, 4))
    assert m.capacity == 5 and m.n_voxels() == 7 and m.truncated() and m.points()[0].shape == (5, 3)
    m = nconv_amd.VoxelMap(xyz, None, xyz, m.count, m.key, torch.tensor([3, 3, 0, 0], dtype=torch.int32), 0.1,
                           (0.0, 0.0, 0.0), (4, 4, 4))
    p = m.points()
    assert not m.truncated() and p[0].shape == (3, 3) and p[1] is None and p[2].shape == (3, 3)


# ---- the C boundary -----------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(nconv_amd):
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", open(HEADER).read(), re.M))
    for name in NEW:
        assert name in declared and name in nconv_amd._lib.EXPORTED and hasattr(nconv_amd._lib.lib(), name)
    assert nconv_amd._lib.ABI_VERSION == 27


@pytest.fixture(scope="module")
def host(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "voxel_host")


def test_ctypes_layout_matches_the_header(host, nconv_amd):
    want = host_harness.ctypes_layout(nconv_amd._lib.NconvVoxelMerge, "nconv_voxel_merge_args")
    assert {k: v for k, v in host.items() if k.startswith("nconv_voxel_merge_args")} == want
    assert host["abi"] == [27, 27]


REASON = {"null_descriptor": "null descriptor", "n_points": "n_points must be in", "max_voxels": "max_voxels must be in",
          "null_stats": "null stats", "null_xyz": "null xyz", "xyz_row_stride": "xyz: row stride smaller than 3",
          "rgb_row_stride": "rgb: row stride smaller than 3", "normals_row_stride": "normals: row stride smaller than 3",
          "n_segments": "n_segments must be >= 1", "segments_without_offsets": "n_segments must be 1 without offsets",
          "nx": "dims:", "ny": "dims:", "nz": "dims:", "cells": "nx * ny * nz < 2^31", "voxel": "voxel must be > 0",
          "origin": "origin must be finite", "null_out_rgb": "null out_rgb with rgb",
          "null_out_normals": "null out_normals with normals", "null_out": "null out_xyz, out_count or out_key",
          "workspace_misaligned": "workspace not 8-byte aligned", "workspace": "workspace too small"}


def test_c_boundary_refuses_every_invalid_call(host):
    calls = {k[3:]: v for k, v in host.items() if k.startswith("rc_")}
    assert len(calls) == 40
    for name, (rc, text) in calls.items():
        assert rc == -22, (name, rc, text)
        assert text.startswith("nconv_voxel_merge: "), (name, text)
        if name.endswith("_misaligned") and name != "workspace_misaligned":
            assert "aligned" in text and name.split("_misaligned")[0].replace("out_", "out_") in text, (name, text)
            continue
        reason = next(r for k, r in REASON.items() if name.startswith(k))
        assert reason in text, (name, text)


def test_workspace_bytes_is_monotone_and_refuses_the_impossible(host, nconv_amd):
    ws = host["workspace_bytes"]
    assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:])) and ws[0] == ws[1] and ws[2] < ws[4]
    assert host["workspace_refused"] == [0] * 5
    wb = nconv_amd.voxelmap.workspace_bytes
    sizes = [wb(n, (100, 80, 20)) for n in (0, 1, 255, 256, 257, 1000, 1024, 1025, 65536, 65537, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[5] == ws[5]
    assert all(s % 8 == 0 for s in sizes)
