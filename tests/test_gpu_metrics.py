"""GPU: the fused depth-metrics kernels (nconv_depth_metrics) against the float64 reference of
metrics_cases: sums 2..8 within the a-priori budget, counts exact; bounds, empty images,
non-positive and NaN predictions, determinism, hipGraph capture and compat.utils.get_metrics."""
import importlib.util
import os
import sys

import pytest
import torch

import metrics_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [0, 1, 9, 10, 11]


def _place(x, dev, layout):
    """x on the device: 'plain' contiguous; 'cropped' the [1:1+H, 1:1+W] view of a larger tensor
    (row-strided, first element not 16-byte aligned); 'padded' the [:H, :W] view of a tensor whose
    rows are a multiple of four wide (aligned rows with a ragged last group of four)."""
    B, _, H, W = x.shape
    if layout == "plain":
        return x.to(dev)
    if layout == "cropped":
        wide = W + 2 if (W + 3) % 4 else W + 3  # element (1, 1) off the 16-byte grid
        big = torch.full((B, 1, H + 2, wide), 7.0, device=dev)
        v = big[:, :, 1:1 + H, 1:1 + W]
    else:
        big = torch.full((B, 1, H + 1, (W + 3) // 4 * 4 + 4), 7.0, device=dev)
        v = big[:, :, :H, :W]
    v.copy_(x)
    return v


# the issue's cases, then aligned rows with a ragged last group of four (W % 4 != 0, row stride % 4 == 0)
CASES = [(1, 1, 5, "plain"), (1, 7, 3, "plain"), (1, 16, 64, "plain"), (1, 17, 65, "plain"),
         (3, 33, 130, "cropped"), (2, 352, 1216, "cropped"), (2, 18, 70, "padded"),
         # the widths at which the shared loader (plane_io.h) changes path, on every alignment: image
         # strides that are no multiple of 4 (B = 2 plain with odd H * W), bases one element off the
         # 16-byte grid and row strides that are no multiple of 4 (cropped), aligned rows with a ragged
         # last group (padded), fully aligned (plain with W % 4 == 0); H no multiple of the 16 tile rows
         (2, 5, 1, "plain"), (2, 3, 3, "cropped"), (1, 9, 4, "plain"), (2, 4, 4, "cropped"), (1, 17, 5, "padded"),
         (2, 17, 255, "padded"), (2, 3, 255, "plain"), (1, 20, 256, "plain"), (2, 18, 256, "cropped"),
         (2, 5, 257, "plain"), (2, 17, 257, "padded"), (2, 17, 261, "padded"), (2, 3, 261, "cropped")]


@pytest.mark.parametrize("B,H,W,layout", CASES)
def test_sums_within_budget_counts_exact(nconv_amd, gpu, B, H, W, layout):
    pred, gt, ref, bound = MC.case(B, H, W, 11)
    p = _place(pred, gpu, layout)
    g = _place(gt, gpu, "padded" if layout == "padded" else "plain")
    if layout == "cropped":
        assert p.data_ptr() % 16 != 0 and p.stride(-2) > W
    acc = torch.zeros(12, dtype=torch.float64, device=gpu)
    got = nconv_amd.depth_metric_sums(p, g, accum=acc)
    assert got.shape == (B, 12) and got.dtype == torch.float64 and got.device == p.device
    MC.check_rows(got, ref, bound, "rows")
    # accum: the in-order float64 sum of the rows
    want = torch.zeros(12, dtype=torch.float64)
    mine = torch.zeros(12, dtype=torch.float64)
    for b in range(B):
        want = want + ref[b]
        mine = mine + got[b].cpu()
    MC.check_rows(acc[None], want[None], bound.sum(0, keepdim=True), "accum")
    assert torch.equal(acc.cpu(), mine)
    # a second call adds to accum
    nconv_amd.depth_metric_sums(p, g, accum=acc)
    for b in range(B):
        mine = mine + got[b].cpu()
    assert torch.equal(acc.cpu(), mine)
    if B == 1:  # (H, W) and (1, H, W) operands are the same plane
        assert torch.equal(nconv_amd.depth_metric_sums(p[0, 0], g[0, 0]), got)
        assert torch.equal(nconv_amd.depth_metric_sums(p[0], g[0]), got)


def test_bounds_select_and_clamp(nconv_amd, gpu):
    kw = dict(gt_min=2.0, gt_max=40.0, clamp=(1.0, 60.0))
    pred, gt, ref, bound = MC.case(3, 33, 130, 12, **kw)
    free = MC.reference_sums(pred, gt)
    assert (ref[:, 0] < free[:, 0]).all() and (ref[:, 0] > 0).all()  # the window drops pixels
    assert (MC._clamped(pred, kw["clamp"]) != pred)[MC._valid(gt, 2.0, 40.0)].any()  # the clamp acts
    got = nconv_amd.depth_metric_sums(_place(pred, gpu, "cropped"), gt.to(gpu), **kw)
    MC.check_rows(got, ref, bound)
    m = nconv_amd.DepthMetrics(device=gpu, **kw).update(pred.to(gpu), gt.to(gpu))
    MC.check_rows(m.state[None], ref.sum(0, keepdim=True), bound.sum(0, keepdim=True))
    # each bound on its own
    for one in (dict(gt_min=2.0), dict(gt_max=40.0), dict(clamp=(1.0, None)), dict(clamp=(None, 60.0))):
        p1, g1, r1, b1 = MC.case(1, 17, 65, 13, **one)
        MC.check_rows(nconv_amd.depth_metric_sums(p1.to(gpu), g1.to(gpu), **one), r1, b1, one)


def test_empty_image_gives_zero_row_and_nan_figures(nconv_amd, gpu):
    pred, gt, ref, bound = MC.case(1, 17, 65, 2)
    gt2 = torch.cat([torch.zeros_like(gt), gt])
    pred2 = torch.cat([pred + 1, pred])
    got = nconv_amd.depth_metric_sums(pred2.to(gpu), gt2.to(gpu))
    assert torch.equal(got[0].cpu(), torch.zeros(12, dtype=torch.float64))
    assert torch.equal(got[1:], nconv_amd.depth_metric_sums(pred.to(gpu), gt.to(gpu)))
    MC.check_rows(got[1:], ref, bound)
    fig = nconv_amd.DepthMetrics.per_image(got)
    for k, v in fig.items():
        if k in ("n", "n_pos"):
            assert v[0] == 0.0 and v[1] > 0
        else:
            assert v[0] != v[0] and v[1] == v[1], k


def test_non_positive_predictions(nconv_amd, gpu):
    pred, gt, _, _ = MC.case(2, 17, 65, 4)
    pred = pred.clone()
    valid = gt > 0
    idx = valid.flatten().nonzero().flatten()
    pred.view(-1)[idx[0::7]] = -3.5
    pred.view(-1)[idx[1::7]] = 0.0
    pred.view(-1)[idx[2::7]] = -0.0
    ref, bound = MC.reference_sums(pred, gt), MC.budget(pred, gt)
    assert (ref[:, 1] < ref[:, 0]).all() and (ref[:, 1] > 0).all()
    got = nconv_amd.depth_metric_sums(pred.to(gpu), gt.to(gpu))
    MC.check_rows(got, ref, bound)
    assert torch.isfinite(got).all()
    # the e sums include those pixels: they differ from the sums over the positive pixels alone
    only_pos = MC.reference_sums(pred, gt * (pred > 0))
    assert ((got[:, 2].cpu() - only_pos[:, 2]) > 1.0).all()
    # with a lower clamp they become positive
    both = nconv_amd.depth_metric_sums(pred.to(gpu), gt.to(gpu), clamp=(0.5, None))
    assert torch.equal(both[:, 0], both[:, 1])


def test_nan_prediction_is_not_hidden(nconv_amd, gpu):
    pred, gt, ref, bound = MC.case(2, 17, 65, 4)
    bad = pred.clone()
    k = (gt[0] > 0).flatten().nonzero().flatten()[3]
    bad[0].view(-1)[k] = float("nan")
    for kw in (dict(), dict(clamp=(1.0, 60.0))):
        clean = nconv_amd.depth_metric_sums(pred.to(gpu), gt.to(gpu), **kw).cpu()
        got = nconv_amd.depth_metric_sums(bad.to(gpu), gt.to(gpu), **kw).cpu()
        assert torch.isnan(got[0, 2:6]).all()
        assert got[0, 0] == clean[0, 0] and got[0, 1] == clean[0, 1] - 1
        assert torch.isfinite(got[0, 6:]).all()
        assert torch.equal(got[1], clean[1])
    # a NaN where the target is invalid is not seen
    k0 = (gt[0] == 0).flatten().nonzero().flatten()[0]
    off = pred.clone()
    off[0].view(-1)[k0] = float("nan")
    MC.check_rows(nconv_amd.depth_metric_sums(off.to(gpu), gt.to(gpu)), ref, bound)


def test_deterministic(nconv_amd, gpu):
    pred, gt, _, _ = MC.case(3, 33, 130, 11)
    p, g = _place(pred, gpu, "cropped"), gt.to(gpu)
    a = nconv_amd.depth_metric_sums(p, g)
    b = nconv_amd.depth_metric_sums(p, g)
    assert torch.equal(a, b)
    # the operand's alignment picks the load width, not the arithmetic
    assert torch.equal(a, nconv_amd.depth_metric_sums(pred.to(gpu), g))


def test_update_in_hipgraph(nconv_amd, gpu):
    cases = [MC.case(2, 17, 65, s)[:2] for s in (4, 6, 7)]
    sp, sg = (torch.zeros(2, 1, 17, 65, device=gpu) for _ in range(2))
    eager = nconv_amd.DepthMetrics(device=gpu)
    for pred, gt in cases:
        sp.copy_(pred)
        sg.copy_(gt)
        eager.update(sp, sg)
    m = nconv_amd.DepthMetrics(device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.update(sp, sg)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(sp, sg)
    for pred, gt in cases:
        sp.copy_(pred)
        sg.copy_(gt)
        graph.replay()
    torch.cuda.synchronize()
    assert m.state[0].item() > 0
    assert torch.equal(m.state, eager.state)


def _compat_utils():
    compat = os.path.join(ROOT, "compat")
    sys.path.insert(0, compat)
    try:
        spec = importlib.util.spec_from_file_location("nconv_compat_utils", os.path.join(compat, "utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(compat)
    return mod


def test_compat_get_metrics_end_to_end(nconv_amd, gpu):
    utils = _compat_utils()
    torch.manual_seed(0)
    net = nconv_amd.DNET(32, crop="generalized")
    loader = []
    for seed in (21, 22):
        _, gt, _, _ = MC.case(2, 64, 96, seed)
        g = torch.Generator().manual_seed(seed)
        depth = gt * (torch.rand(gt.shape, generator=g) < 0.5)
        loader.append({"depth": depth, "gt": gt})
    kw = dict(gt_max=70.0, clamp=(1.0, 80.0))
    got = utils.get_metrics(net, loader, "cuda", unit_m=0.5, **kw)
    assert not net.training
    hand = nconv_amd.DepthMetrics(device=gpu, **kw)
    with torch.no_grad():
        for data in loader:
            est = net(data["depth"].to(gpu))
            assert est.shape == data["gt"].shape
            hand.update(est, data["gt"].to(gpu))
    want = hand.compute(unit_m=0.5)
    assert got == want
    assert got["n"] == sum(float(((d["gt"] > 0) & (d["gt"] <= 70.0)).sum()) for d in loader)
    assert got["n_pos"] == got["n"] and got["rmse"] > 0 and got["rmse_mm"] == 500.0 * got["rmse"]
