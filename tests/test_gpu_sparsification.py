"""GPU: nconv_depth_sparsification against the numpy reference (tests/sparsification_cases.py): order bit for
bit, counts exactly, every sum within the bound of any summation order of n_b non-negative doubles. Shapes
sized from the kernel's constants, the key patterns that stress a stable radix sort, cropped views, steps,
guard bands, determinism, torch.cuda.graph, SparsificationCurves, and one DNET end-to-end run."""
import ctypes

import numpy as np
import pytest
import torch

import sparsification_cases as SC

pytestmark = pytest.mark.gpu

F32 = np.float32


def _dev(gpu, *arrays):
    return [torch.tensor(np.asarray(x)).to(gpu)[:, None] for x in arrays]  # a copy: the shared cases are read-only


def _run(nconv_amd, gpu, pred, gt, conf, **kw):
    curves, order = nconv_amd.sparsification(*_dev(gpu, pred, gt, conf), return_order=True, **kw)
    torch.cuda.synchronize()
    return curves.cpu().numpy(), order.cpu().numpy()


def _check(nconv_amd, gpu, shape, pattern, seed=0, steps=100):
    pred, gt, conf, want, order, n = SC.case(shape, pattern, seed, steps)
    got, got_order = _run(nconv_amd, gpu, pred, gt, conf, steps=steps)
    assert got_order.dtype == np.int32 and np.array_equal(got_order, order)
    SC.assert_curves(got, want, n)
    return got


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_key_patterns_on_the_multi_tile_shape(nconv_amd, gpu, pattern):
    got = _check(nconv_amd, gpu, SC.MULTI, pattern)
    n = SC.case(SC.MULTI, pattern)[5]
    assert n[0] == SC.MULTI[1] * SC.MULTI[2] and n[0] % SC.SORT_TILE and len(set(n.tolist())) == 3
    assert got.shape == (3, 2, 100, 3)


def test_equal_confidence_is_raster_order(nconv_amd, gpu):
    pred, gt, conf, _, _, n = SC.case(SC.MULTI, "equal")
    _, order = _run(nconv_amd, gpu, pred, gt, conf)
    for b in range(SC.MULTI[0]):
        assert np.array_equal(order[b, 0, :n[b]], np.flatnonzero(gt[b].reshape(-1) > 0))


@pytest.mark.parametrize("shape", [SC.SMALL, SC.WIDE], ids=["small", "wide"])
def test_one_small_plane_and_more_chunks_than_threads(nconv_amd, gpu, shape):
    _check(nconv_amd, gpu, shape, "random", seed=1, steps=7)
    _check(nconv_amd, gpu, shape, "four", seed=2, steps=7)


def _counts_case():
    """B = 3: about half of the pixels, none, and exactly one (the last pixel)."""
    B, H, W = 3, 67, 131
    pred, gt, conf = (x.copy() for x in SC.case((B, H, W), "four", seed=7, steps=7)[:3])
    gt[0][np.random.default_rng(7).random((H, W)) < 0.5] = 0
    gt[1] = 0
    gt[2] = 0
    gt[2, H - 1, W - 1] = 3.5
    return pred, gt, conf


def test_three_valid_counts_zero_and_one(nconv_amd, gpu):
    pred, gt, conf = _counts_case()
    for steps in (1, 7, 100, 1024):
        want, order, n = SC.sparsification_ref(pred, gt, conf, steps) if steps <= 100 else (None, None, None)
        got, got_order = _run(nconv_amd, gpu, pred, gt, conf, steps=steps)
        if want is not None:
            assert n[1] == 0 and n[2] == 1 and n[0] > 2 * SC.SORT_TILE
            assert np.array_equal(got_order, order)
            SC.assert_curves(got, want, n)
        assert not got[1].any() and (got_order[1] == -1).all()
        # one pixel, n_b < steps: every k_j is 0, the one term exactly
        a, q = SC.terms(pred[2, -1, -1], gt[2, -1, -1])
        assert (got[2] == np.array([1.0, float(a), float(q)])).all()
        assert got_order[2, :, 0].tolist() == [67 * 131 - 1] * 2 and (got_order[2, :, 1:] == -1).all()


@pytest.mark.parametrize("steps", [1, 7, 100, 1024])
def test_steps(nconv_amd, gpu, steps):
    shape = (2, 23, 37)  # n_b = 851 and about 425: below 1024 steps
    _check(nconv_amd, gpu, shape, "random", seed=3, steps=steps)


def test_bounds_clamp_and_uncertainty(nconv_amd, gpu):
    pred, gt, conf = SC.case(SC.MULTI, "four", seed=4)[:3]
    kw = dict(gt_min=5.0, gt_max=60.0, clamp=(2.0, 55.0))
    for unc in (False, True):
        want, order, n = SC.sparsification_ref(pred, gt, conf, 13, uncertainty=unc, **kw)
        got, got_order = _run(nconv_amd, gpu, pred, gt, conf, steps=13, uncertainty=unc, **kw)
        assert np.array_equal(got_order, order)
        SC.assert_curves(got, want, n)


def test_nan_prediction_and_nan_confidence_order_only(nconv_amd, gpu):
    pred, gt, conf = (x.copy() for x in SC.case(SC.MULTI, "random", seed=5)[:3])
    rng = np.random.default_rng(5)
    pred.reshape(-1)[rng.choice(pred.size, 40, replace=False)] = np.nan
    pred.reshape(-1)[rng.choice(pred.size, 10, replace=False)] = np.inf
    conf.reshape(-1)[rng.choice(conf.size, 40, replace=False)] = np.nan
    conf.reshape(-1)[rng.choice(conf.size, 20, replace=False)] = -np.nan
    for unc in (False, True):
        want, order, n = SC.sparsification_ref(pred, gt, conf, 5, uncertainty=unc, sums=False)
        got, got_order = _run(nconv_amd, gpu, pred, gt, conf, steps=5, uncertainty=unc)
        assert np.array_equal(got_order, order)
        assert np.array_equal(got[..., 0], want[..., 0])


def _cropped(gpu, x, lead, top, left):
    """x (B, H, W) as a (B, 1, H, W) window of a larger buffer of other values, the base `lead` elements in."""
    B, H, W = x.shape
    hh, ww = H + top + 2, W + left + 3
    whole = torch.full((B * hh * ww + lead + 3,), float("nan"), device=gpu)
    big = whole[lead:lead + B * hh * ww].view(B, 1, hh, ww)
    v = big[:, :, top:top + H, left:left + W]
    v.copy_(torch.tensor(np.asarray(x))[:, None])
    return v


def test_cropped_views_with_odd_offsets(nconv_amd, gpu):
    pred, gt, conf, want, order, n = SC.case(SC.MULTI, "four")
    views = [_cropped(gpu, pred, 1, 1, 2), _cropped(gpu, gt, 3, 2, 1), _cropped(gpu, conf, 2, 0, 3)]
    assert all(v.data_ptr() % 16 for v in views) and not any(v.is_contiguous() for v in views)
    curves, got_order = nconv_amd.sparsification(*views, return_order=True)
    torch.cuda.synchronize()
    assert np.array_equal(got_order.cpu().numpy(), order)
    SC.assert_curves(curves.cpu().numpy(), want, n)
    # (H, W) and (1, H, W) operands
    one = nconv_amd.sparsification(views[0][0, 0], views[1][0, 0], views[2][0], steps=100)
    assert tuple(one.shape) == (1, 2, 100, 3) and torch.equal(one[0], curves[0])


def test_guard_bands_through_the_c_abi(nconv_amd, gpu):
    """curves, order and the workspace written inside their extents only, at an offset base."""
    L = nconv_amd._lib
    lib = L.lib()
    pred, gt, conf, want, order, n = SC.case(SC.MULTI, "top_digit")
    B, H, W = SC.MULTI
    J = 100
    p, g, c = (t.contiguous() for t in _dev(gpu, pred, gt, conf))
    nws = lib.nconv_depth_sparsification_workspace_bytes(B, H, W, J)
    ws_all = torch.full((nws + 16,), 0x5A, dtype=torch.uint8, device=gpu)
    cur_all = torch.full((B * 2 * J * 3 + 2,), -7.0, dtype=torch.float64, device=gpu)
    ord_all = torch.full((B * 2 * H * W + 2,), -77, dtype=torch.int32, device=gpu)
    d = L.NconvDepthSparsification()
    d.B, d.H, d.W, d.steps = B, H, W, J
    d.pred, d.gt, d.conf = p.data_ptr(), g.data_ptr(), c.data_ptr()
    d.pred_image_stride = d.gt_image_stride = d.conf_image_stride = H * W
    d.pred_row_stride = d.gt_row_stride = d.conf_row_stride = W
    d.curves, d.order = cur_all[1:].data_ptr(), ord_all[1:].data_ptr()
    rc = lib.nconv_depth_sparsification(ctypes.byref(d), ctypes.c_void_p(ws_all[8:].data_ptr()), nws, L.stream_handle(gpu))
    L.check(rc, "nconv_depth_sparsification")
    torch.cuda.synchronize()
    assert (ws_all[:8] == 0x5A).all() and (ws_all[8 + nws:] == 0x5A).all()
    assert cur_all[0] == -7.0 and cur_all[-1] == -7.0 and ord_all[0] == -77 and ord_all[-1] == -77
    assert np.array_equal(ord_all[1:-1].view(B, 2, H * W).cpu().numpy(), order)
    SC.assert_curves(cur_all[1:-1].view(B, 2, J, 3).cpu().numpy(), want, n)


def test_same_bits_with_and_without_order_and_on_every_run(nconv_amd, gpu):
    pred, gt, conf = SC.case(SC.MULTI, "four")[:3]
    p, g, c = _dev(gpu, pred, gt, conf)
    first, order = nconv_amd.sparsification(p, g, c, return_order=True)
    again, order2 = nconv_amd.sparsification(p, g, c, return_order=True)
    plain = nconv_amd.sparsification(p, g, c)
    assert torch.equal(first.view(torch.int64), again.view(torch.int64)) and torch.equal(order, order2)
    assert torch.equal(first.view(torch.int64), plain.view(torch.int64))


def test_captured_update_replays_on_changed_input(nconv_amd, gpu):
    shape = SC.MULTI
    cases = [SC.case(shape, pat, seed) for pat, seed in (("four", 0), ("random", 8), ("specials", 9))]
    p, g, c = (t.clone() for t in _dev(gpu, *cases[0][:3]))
    acc = nconv_amd.SparsificationCurves(steps=100, gt_max=None, device=gpu)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        acc.update(p, g, c)  # warm-up: the workspace and the curves now exist
        acc.reset()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.graph
    gr = torch.cuda.CUDAGraph()
    with graph(gr):
        acc.update(p, g, c)
    curves = acc._buffers[(p.device, tuple(p.shape))][0]
    acc.reset()
    total = torch.zeros_like(acc.state)
    for pred, gt, conf, want, _, n in cases[1:]:
        for dst, src in zip((p, g, c), _dev(gpu, pred, gt, conf)):
            dst.copy_(src)
        gr.replay()
        torch.cuda.synchronize()
        eager = nconv_amd.sparsification(p, g, c)
        assert torch.equal(curves.view(torch.int64), eager.view(torch.int64))
        SC.assert_curves(curves.cpu().numpy(), want, n)
        total += nconv_amd.SparsificationCurves.normalised(eager).sum(1)
    assert torch.equal(acc.state, total) and int(acc.images) == 2 * shape[0]


def _curves_tolerance(n_max, scale):
    """A normalised curve point is a ratio of two means (RMSE: of their roots): each sum within
    sum_bound(n), two divisions and at most two roots of half an ulp each, then the mean over a few images."""
    return (4 * SC.sum_bound(n_max) + 16 * 2.0 ** -53) * scale


def test_sparsification_curves_over_two_batches(nconv_amd, gpu):
    a = SC.case(SC.MULTI, "random", seed=10)
    pred_b, gt_b, conf_b = _counts_case()  # holds an image without a valid pixel: left out of the mean
    want_b = SC.sparsification_ref(pred_b, gt_b, conf_b, 100, gt_max=80.0)[0]
    acc = nconv_amd.SparsificationCurves(steps=100, gt_max=80.0, device=gpu)
    acc.update(*_dev(gpu, *a[:3])).update(*_dev(gpu, pred_b, gt_b, conf_b))
    out = acc.compute()
    norm = np.concatenate((SC.normalised_ref(a[3]), SC.normalised_ref(want_b)), axis=1)  # (2, 6, 2, J)
    assert out["images"] == 5 and np.array_equal(out["fraction"].numpy(), np.arange(100) / 100)
    mean = norm.sum(1) / 5
    tol = _curves_tolerance(int(a[5].max()), np.abs(norm).max())
    for f, fig in enumerate(("mae", "rmse")):
        for o, rank in enumerate(("conf", "oracle")):
            err = np.abs(out[f"{fig}_{rank}"].numpy() - mean[f, o]).max()
            print(f"{fig}_{rank}: max abs err {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol
        ause = float((mean[f, 0] - mean[f, 1]).mean())
        assert abs(out[f"ause_{fig}"] - ause) <= 2 * tol and out[f"ause_{fig}"] > 0


def test_confidence_that_is_the_negated_error_has_zero_ause(nconv_amd, gpu):
    B, H, W = SC.MULTI
    rng = np.random.default_rng(11)
    gt = np.full(SC.MULTI, 7, dtype=F32)
    a = np.stack([rng.permutation(H * W).reshape(H, W) for _ in range(B)]).astype(F32) * F32(2.0 ** -10)
    pred = gt + a  # exact, so |pred - gt| is tie-free
    p, g = _dev(gpu, pred, gt)
    conf = -(p - g).abs()
    curves, order = nconv_amd.sparsification(p, g, conf, return_order=True)
    assert torch.equal(order[:, 0], order[:, 1]) and torch.equal(curves[:, 0], curves[:, 1])
    acc = nconv_amd.SparsificationCurves(steps=100, gt_max=None, device=gpu).update(p, g, conf)
    out = acc.compute()
    assert out["ause_mae"] == 0.0 and out["ause_rmse"] == 0.0 and out["images"] == B
    assert out["mae_conf"][0] == 1.0 and out["rmse_oracle"][0] == 1.0


def test_dnet_confidence_end_to_end(nconv_amd, gpu):
    torch.manual_seed(0)
    net = nconv_amd.DNET(32).to(gpu).eval()
    g = torch.Generator().manual_seed(0)
    dense = torch.rand(2, 1, 64, 96, generator=g) * 79 + 1
    sparse = (dense * (torch.rand(2, 1, 64, 96, generator=g) < 0.1)).to(gpu)
    with torch.no_grad():
        pred, conf = net.forward_with_confidence(sparse)  # cropped views of nconv7's grid
    gt = ((torch.rand(pred.shape, generator=g) * 79 + 1) * (torch.rand(pred.shape, generator=g) < 0.3)).to(gpu)
    curves, order = nconv_amd.sparsification(pred, gt, conf, steps=20, gt_max=80.0, return_order=True)
    want, want_order, n = SC.sparsification_ref(pred[:, 0].cpu().numpy(), gt[:, 0].cpu().numpy(),
                                                conf[:, 0].cpu().numpy(), 20, gt_max=80.0)
    assert (n > 100).all() and np.array_equal(order.cpu().numpy(), want_order)
    SC.assert_curves(curves.cpu().numpy(), want, n)
