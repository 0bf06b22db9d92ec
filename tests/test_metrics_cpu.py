"""CPU: the depth-metrics entry points are exported with the header's ABI version and validate their
arguments on the host; DepthMetrics' host logic (compute, unit conversions, merge, per_image,
from_sums, all_reduce over gloo) is plain tensor arithmetic on hand-made sums."""
import ctypes
import math
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")


def test_metrics_symbols_and_abi(nconv_amd):
    L = nconv_amd._lib
    lib = L.lib()
    src = open(HEADER).read()
    for name in ("nconv_depth_metrics_workspace_bytes", "nconv_depth_metrics"):
        assert name in L.EXPORTED
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    v = int(re.search(r"#define NCONV_ABI_VERSION (\d+)", src).group(1))
    assert lib.nconv_abi_version() == v == L.ABI_VERSION and v >= 24
    assert int(re.search(r"#define NCONV_DEPTH_METRICS_SUMS (\d+)", src).group(1)) == L.DEPTH_METRICS_SUMS == 12
    assert nconv_amd.DepthMetrics is nconv_amd.metrics.DepthMetrics
    assert nconv_amd.depth_metric_sums is nconv_amd.metrics.depth_metric_sums


def test_metrics_workspace_size(nconv_amd):
    ws = nconv_amd._lib.lib().nconv_depth_metrics_workspace_bytes
    assert ws(1, 1, 1) > 0
    assert ws(0, 5, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 5, 0) == 0
    # one fp32 partial row per 1,024-pixel tile and one double row per image, at the least
    assert ws(8, 352, 1216) >= 8 * 12 * 8 + 8 * (352 * 1216 // 1024) * 12 * 4
    base = (2, 33, 130)
    for axis in range(3):
        prev = 0
        for n in (1, 2, 15, 16, 17, 63, 64, 65, 130, 400):
            dims = list(base)
            dims[axis] = n
            cur = ws(*dims)
            assert cur >= prev > -1 and cur > 0, (dims, cur, prev)
            prev = cur


def test_metrics_validation_is_host_only(nconv_amd):
    """Every malformed call fails with -22 and a message before any launch (fake pointers, no GPU)."""
    lib = nconv_amd._lib.lib()
    p = ctypes.c_void_p(0x1000)
    big = lib.nconv_depth_metrics_workspace_bytes(2, 4, 8)
    nan = float("nan")

    def call(pred=p, pbs=32, prs=8, gt=p, gbs=32, grs=8, B=1, H=4, W=8, gt_min=0.0, gt_max=0.0, lo=0.0, hi=0.0,
             sums=p, accum=p, ws=p, ws_bytes=big):
        return lib.nconv_depth_metrics(pred, pbs, prs, gt, gbs, grs, B, H, W, gt_min, gt_max, lo, hi, sums, accum,
                                       ws, ws_bytes, None)

    cases = [
        (dict(pred=None), "null plane"),
        (dict(gt=None), "null plane"),
        (dict(sums=None, accum=None), "null sums and accum"),
        (dict(B=0), "non-positive"),
        (dict(H=0), "non-positive"),
        (dict(W=-1), "non-positive"),
        (dict(prs=7), "row stride"),
        (dict(grs=7), "row stride"),
        (dict(B=2, pbs=31), "image stride"),
        (dict(B=2, gbs=31), "image stride"),
        (dict(ws_bytes=8), "workspace too small"),
        (dict(B=2, ws_bytes=big - 4), "workspace too small"),
        (dict(ws=None), "workspace too small"),
        (dict(gt_min=-1.0), "negative or NaN"),
        (dict(gt_max=nan), "negative or NaN"),
        (dict(lo=-0.5), "negative or NaN"),
        (dict(hi=nan), "negative or NaN"),
        (dict(gt_min=5.0, gt_max=2.0), "gt_min > gt_max"),
        (dict(lo=5.0, hi=2.0), "clamp_lo > clamp_hi"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -22, (kw, msg)
        err = lib.nconv_last_error().decode()
        assert msg in err and err.startswith("nconv_depth_metrics:"), (kw, err)


def _hand_sums():
    # 4 valid pixels, 3 of them positive
    return torch.tensor([4.0, 3.0, 6.0, 16.0, 0.5, 1.0, 0.03, 0.0012, 0.27, 1.0, 2.0, 3.0], dtype=torch.float64)


def test_compute_on_hand_made_sums(nconv_amd):
    DM = nconv_amd.DepthMetrics
    m = DM.from_sums(_hand_sums())
    assert m.state.device.type == "cpu" and m.state.dtype == torch.float64
    r = m.compute()
    want = {"n": 4.0, "n_pos": 3.0, "mae": 1.5, "rmse": 2.0, "rel": 0.125, "sqrel": 0.25, "imae": 0.01,
            "irmse": 0.02, "rmse_log": 0.3, "d1": 1 / 3, "d2": 2 / 3, "d3": 1.0,
            "mae_mm": 1500.0, "rmse_mm": 2000.0, "imae_1/km": 10.0, "irmse_1/km": 20.0}
    assert set(r) == set(want)
    for k, v in want.items():
        assert isinstance(r[k], float) and r[k] == pytest.approx(v, rel=1e-12), k
    # KITTI's 16-bit PNG unit: 1/256 m
    q = m.compute(unit_m=1 / 256)
    for k in ("n", "n_pos", "mae", "rmse", "rel", "sqrel", "imae", "irmse", "rmse_log", "d1", "d2", "d3"):
        assert q[k] == r[k], k
    assert q["rmse_mm"] == pytest.approx(1000 * q["rmse"] / 256, rel=1e-12)
    assert q["mae_mm"] == pytest.approx(r["mae_mm"] / 256, rel=1e-12)
    assert q["imae_1/km"] == pytest.approx(r["imae_1/km"] * 256, rel=1e-12)
    assert q["irmse_1/km"] == pytest.approx(1000 * q["irmse"] * 256, rel=1e-12)


def test_compute_empty_state_is_nan(nconv_amd):
    m = nconv_amd.DepthMetrics(device="cpu")
    r = m.compute()
    assert r["n"] == 0.0 and r["n_pos"] == 0.0
    for k, v in r.items():
        if k not in ("n", "n_pos"):
            assert math.isnan(v), k
    # valid pixels, none positive: the error means exist, the inverse / log / delta means do not
    s = _hand_sums()
    s[1] = 0
    s[6:] = 0
    r = nconv_amd.DepthMetrics.from_sums(s).compute()
    assert r["mae"] == 1.5 and math.isnan(r["imae"]) and math.isnan(r["d1"]) and math.isnan(r["rmse_log"])
    m = nconv_amd.DepthMetrics.from_sums(_hand_sums())
    assert m.reset() is m and not m.state.any()


def test_merge_equals_concatenated_sums(nconv_amd):
    DM = nconv_amd.DepthMetrics
    pred, gt, ref, _ = MC.case(3, 33, 130, 1)
    a, b = DM.from_sums(ref[:1]), DM.from_sums(ref[1:])
    whole = DM.from_sums(ref)
    a.merge(b)
    torch.testing.assert_close(a.state, whole.state, rtol=1e-13, atol=0)
    assert torch.equal(a.state[[0, 1, 9, 10, 11]], ref[:, [0, 1, 9, 10, 11]].sum(0))
    ra, rw = a.compute(), whole.compute()
    for k in rw:
        assert ra[k] == pytest.approx(rw[k], rel=1e-12), k


def test_per_image_agrees_with_compute(nconv_amd):
    DM = nconv_amd.DepthMetrics
    _, _, ref, _ = MC.case(1, 17, 65, 2)
    one = DM.per_image(ref, unit_m=0.5)
    all_ = DM.from_sums(ref).compute(unit_m=0.5)
    assert set(one) == set(all_)
    for k, v in one.items():
        assert isinstance(v, list) and len(v) == 1 and v[0] == all_[k], k
    _, _, ref3, _ = MC.case(3, 33, 130, 1)
    many = DM.per_image(ref3)
    assert all(len(v) == 3 for v in many.values())
    assert many["rmse"][2] == math.sqrt(ref3[2, 3].item() / ref3[2, 0].item())


def test_update_refuses_cpu_and_non_fp32(nconv_amd):
    pred, gt, _, _ = MC.case(1, 7, 3, 3)
    m = nconv_amd.DepthMetrics(device="cpu")
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        m.update(pred, gt)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        nconv_amd.depth_metric_sums(pred, gt)
    assert not m.state.any()
    with pytest.raises(ValueError):
        nconv_amd.DepthMetrics(gt_min=-1.0, device="cpu")
    with pytest.raises(ValueError):
        nconv_amd.DepthMetrics(clamp=(5.0, 2.0), device="cpu")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nconv_pkg
    import metrics_cases
    m = nconv_pkg.load()
    _, _, ref, _ = metrics_cases.case(4, 17, 65, 5)
    dm = m.DepthMetrics.from_sums(ref[2 * rank:2 * rank + 2])
    dm.all_reduce()
    q.put((rank, dm.state.numpy().copy()))  # by value: see test_dp_gloo.py
    dist.destroy_process_group()


def test_all_reduce_over_gloo_gives_every_rank_the_whole_case(nconv_amd):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _, _, ref, _ = MC.case(4, 17, 65, 5)
    whole = nconv_amd.DepthMetrics.from_sums(ref).state
    for rank in range(world):
        got = torch.from_numpy(res[rank])
        torch.testing.assert_close(got, whole, rtol=1e-13, atol=0)
        assert torch.equal(got[[0, 1, 9, 10, 11]], whole[[0, 1, 9, 10, 11]])
    assert torch.equal(torch.from_numpy(res[0]), torch.from_numpy(res[1]))
