"""The smoothness loss and the edge weights (smooth.smoothness_loss / edge_weights: nconv_smooth_loss_*,
nconv_edge_weights) on the GPU: bit for bit against the fp32 rule restated in numpy (smooth_cases.rule_fp32,
edge_weights_rule) including the loss's summation tree, cropped views inside sentinels, a pyramid level of
the view warp made with halve_intrinsics / halve_projection, Smoother under torch.cuda.graph, EdgeWeights
behind the prefetcher, and a captured training step with the whole self-supervised objective."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reduce_tree as RT
import smooth_cases as SC
import warp_cases as WC
from test_gpu_dnet import sparse_depth

pytestmark = pytest.mark.gpu
f32 = np.float32


def _run(nconv_amd, gpu, depth, weights, order, mask, gloss):
    """(L, counts, g_depth (B, H, W)) as numpy from the device."""
    d = torch.as_tensor(depth).to(gpu)[:, None].requires_grad_(True)
    w = None if weights is None else torch.as_tensor(weights).to(gpu)
    m = None if mask is None else torch.as_tensor(mask).to(gpu)[:, None]
    L, counts = nconv_amd.smoothness_loss(d, w, order, m, return_counts=True)
    L.backward(None if gloss is None else torch.tensor(gloss, device=gpu))
    torch.cuda.synchronize()
    assert counts.dtype == torch.int32 and d.grad.shape == d.shape
    return L.detach().cpu().numpy(), counts.cpu().numpy(), d.grad[:, 0].cpu().numpy()


def _same(a, b):
    return np.asarray(a, dtype=f32).tobytes() == np.asarray(b, dtype=f32).tobytes()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape", SC.GPU_SHAPES, ids=["x".join(map(str, s)) for s in SC.GPU_SHAPES])
def test_loss_counts_gradient_and_weights_match_rule(nconv_amd, gpu, shape, order):
    """L, n_x, n_y, g_depth and the weight planes bit for bit, without and with weights and mask, gloss 0.7;
    a second run gives the same bits."""
    B, _, H, W = shape
    x = SC.smooth_inputs(B, H, W, seed=H * W + order, with_w=True, with_mask=True)
    got_w = nconv_amd.edge_weights(torch.as_tensor(x["rgb"]).to(gpu)).cpu().numpy()
    assert got_w.shape == (B, 2, H, W) and np.array_equal(got_w.view(np.uint32), x["weights"].view(np.uint32))
    for weights in (None, x["weights"]):
        for mask in (None, x["mask"]):
            rule = SC.rule_fp32(x["depth"], weights, order, mask, SC.GLOSS)
            L, counts, g = _run(nconv_amd, gpu, x["depth"], weights, order, mask, SC.GLOSS)
            what = (shape, order, weights is not None, mask is not None)
            assert counts.tolist() == [rule["n_x"], rule["n_y"]], what
            assert _same(L, rule["L"]), (what, L, rule["L"])
            assert np.array_equal(g.view(np.uint32), rule["g_depth"].view(np.uint32)), what
            again = _run(nconv_amd, gpu, x["depth"], weights, order, mask, SC.GLOSS)
            assert _same(L, again[0]) and np.array_equal(counts, again[1]) and _same(g, again[2])


@pytest.mark.parametrize("C,alpha", [(1, 1.0 / 255.0), (3, 1.0), (3, 0.0)])
def test_edge_weights_match_rule_on_strided_frames(nconv_amd, gpu, C, alpha):
    """One and three channels, alpha 1 on values up to 255 (weights down to the flush to +0) and alpha 0
    (every weight exactly 1), the frame a crop of a larger buffer, the output a kept tensor."""
    g = torch.Generator().manual_seed(C)
    img = torch.randint(0, 256, (2, C, 33, 130), generator=g).float()
    big = torch.full((2, C + 1, 40, 140), 1e30, device=gpu)
    view = big[:, 1:, 3:36, 5:135]
    view.copy_(img)
    out = torch.empty(2, 2, 33, 130, device=gpu)
    got = nconv_amd.edge_weights(view, alpha, out=out)
    want = SC.edge_weights_rule(img.numpy(), alpha)
    assert got.data_ptr() == out.data_ptr() and not view.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if alpha == 1.0:
        assert (want == 0).any() and (want[:, 0, :, :-1] < 1).any()
    if alpha == 0.0:
        assert (want == 1).all()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape", [(3, 33, 70), (17, 17, 65)], ids=["3x33x70", "17x17x65"])
def test_smooth_loss_sum_is_the_stated_tree(nconv_amd, gpu, shape, order):
    """One huge x term among ones (wave 0, lane 0 of a tile in the middle of the batch) and a huge y term
    elsewhere: L bit for bit from the rule's fp32 terms summed in the order csrc/wave_ops.h states
    (reduce_tree.py, view_warp.hip's thread map), Sx and Sy apart; a sum in another order differs. Partial
    tiles in both directions, six or four tiles per image; seventeen images, so that a wave of the finalize stage
    takes a second one."""
    B, H, W = shape
    i = np.arange(H, dtype=f32)[:, None]
    j = np.arange(W, dtype=f32)[None, :]
    # first differences 1 in both directions (order 1); second differences 2 through i^2 + j^2 (order 2)
    d = np.broadcast_to(i + j if order == 1 else i * i + j * j, (B, H, W)).astype(f32).copy()
    b = B // 2
    d[b, 16, 0] += f32(2.0 ** 24)  # row 16, column 0: the first pixel of the tile below
    rule = SC.rule_fp32(d, None, order)
    L, counts, _ = _run(nconv_amd, gpu, d, None, order, None, None)
    naive = f32(np.float64(rule["sx"].sum(dtype=np.float64)) / rule["n_x"] + rule["sy"].sum(dtype=np.float64) / rule["n_y"])
    print(f"L {L:.9g} tree {rule['L']:.9g} plain float64 sum {naive:.9g}")
    assert counts.tolist() == [rule["n_x"], rule["n_y"]]
    assert _same(L, rule["L"])
    assert RT.tile_partials(rule["sx"], RT.ROWS).shape == (B, -(-H // 16) * 2)
    assert (rule["sx"] >= 2.0 ** 23).any() and (rule["sy"] >= 2.0 ** 23).any()


def test_cropped_strided_depth_view(nconv_amd, gpu):
    """depth a DNET-style crop of a larger buffer at an odd offset (NaN sentinels around the view: one read
    of them would poison L), the mask a crop of another with other strides, g_depth a kept tensor inside
    sentinels: the results are the contiguous ones, and nothing outside the outputs is written."""
    x = SC.smooth_inputs(2, 45, 67, seed=9, with_w=True, with_mask=True)
    for order in (1, 2):
        rule = SC.rule_fp32(x["depth"], x["weights"], order, x["mask"])
        big_d = torch.full((2, 1, 49, 71), float("nan"), device=gpu)
        big_m = torch.ones((2, 1, 46, 75), dtype=torch.uint8, device=gpu)
        dv, mv = big_d[:, :, 3:48, 1:68], big_m[:, :, 1:, 3:70]
        dv.copy_(torch.as_tensor(x["depth"])[:, None])
        mv.copy_(torch.as_tensor(x["mask"])[:, None])
        before = big_d.clone()
        guard = torch.full((2 * 45 * 67 + 128,), -7.0, device=gpu)
        kept = {"g_depth": guard[64:-64].view(2, 1, 45, 67)}
        d = dv.detach().requires_grad_(True)
        assert not d.is_contiguous() and not mv.is_contiguous()
        L, counts = nconv_amd.smoothness_loss(d, torch.as_tensor(x["weights"]).to(gpu), order, mv.view(torch.bool),
                                              return_counts=True, out=kept)
        L.backward()
        torch.cuda.synchronize()
        assert _same(L.item(), rule["L"]) and counts.tolist() == [rule["n_x"], rule["n_y"]]
        assert np.array_equal(kept["g_depth"][:, 0].cpu().numpy(), rule["g_depth"])
        assert np.array_equal(d.grad[:, 0].cpu().numpy(), rule["g_depth"])
        assert (guard[:64] == -7).all() and (guard[-64:] == -7).all()
        assert torch.equal(big_d.view(torch.int32), before.view(torch.int32))


def test_pyramid_level_of_the_view_warp(nconv_amd, gpu):
    """The "half a metre sideways is eight columns" construction one level down: a fronto-parallel plane at
    4 m, fx = fy = 64, t = (0.5, 0, 0), an integer-valued source. The warp of the 2 x 2 average-pooled
    frames with halve_intrinsics(k) and halve_projection(m) is the average pooling of the full-resolution
    warp exactly (u' = j' + 4) on the columns that stay inside the source; with k / 2 it is not."""
    B, C, H, W = 2, 3, 20, 72
    g = torch.Generator().manual_seed(8)
    src = torch.randint(0, 256, (B, C, H, W), generator=g).float().to(gpu)
    k = torch.tensor([[64.0, 0, 30], [0, 64.0, 9], [0, 0, 1]], device=gpu)
    d = torch.full((B, 1, H, W), 4.0, device=gpu)
    m = nconv_amd.warp_projection(k, torch.tensor(WC.rigid(t=(0.5, 0.0, 0.0)), device=gpu))
    full, valid = nconv_amd.view_warp(d, k, src, m, return_valid=True)
    assert valid[..., :W - 8].all() and torch.equal(full[..., :W - 8], src[..., 8:])
    want = F.avg_pool2d(full, 2)
    d2, src2 = F.avg_pool2d(d, 2), F.avg_pool2d(src, 2)
    half, valid2 = nconv_amd.view_warp(d2, nconv_amd.halve_intrinsics(k), src2, nconv_amd.halve_projection(m),
                                       return_valid=True)
    inner = W // 2 - 4
    assert valid2[..., :inner].all() and not valid2[..., inner:].any()
    assert torch.equal(half[..., :inner], want[..., :inner]) and torch.equal(half[..., :inner], src2[..., 4:])
    naive = nconv_amd.view_warp(d2, k / 2, src2, nconv_amd.halve_projection(m))
    assert not torch.equal(naive[..., :inner - 1], want[..., :inner - 1])


def test_smoother_keeps_its_buffers_and_replays(nconv_amd, gpu):
    """Smoother: no allocation after construction, so the loss with its backward is captured and replayed;
    refilling the depth and the weights in place changes the replay's results to the eager call's, bit for
    bit."""
    B, H, W = 2, 33, 130
    xs = [SC.smooth_inputs(B, H, W, seed=s, with_w=True) for s in (1, 2)]
    for order in (1, 2):
        sm = nconv_amd.Smoother((H, W), B=B, order=order, device=gpu)
        d = torch.as_tensor(xs[0]["depth"]).to(gpu)[:, None].clone().requires_grad_(True)
        w = torch.as_tensor(xs[0]["weights"]).to(gpu).clone()
        seed = torch.full((), 0.7, device=gpu)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sm(d, w).backward(seed)
        torch.cuda.current_stream().wait_stream(side)
        d.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            L, counts = sm(d, w, return_counts=True)
            L.backward(seed)
        assert L.data_ptr() == sm._out["loss"].data_ptr()
        seen = []
        for x in xs[::-1]:
            with torch.no_grad():
                d.copy_(torch.as_tensor(x["depth"])[:, None])
            w.copy_(torch.as_tensor(x["weights"]))
            graph.replay()
            torch.cuda.synchronize()
            got = (L.item(), counts.tolist(), d.grad.clone())
            e = d.detach().clone().requires_grad_(True)
            Le, ce = nconv_amd.smoothness_loss(e, w, order, return_counts=True)
            Le.backward(seed)
            rule = SC.rule_fp32(x["depth"], x["weights"], order, None, 0.7)
            assert _same(got[0], Le.item()) and got[1] == ce.tolist() and torch.equal(got[2], e.grad)
            assert _same(got[0], rule["L"]) and np.array_equal(got[2][:, 0].cpu().numpy(), rule["g_depth"])
            seen.append(got)
        assert seen[0][0] != seen[1][0] and not torch.equal(seen[0][2], seen[1][2])
        with pytest.raises(ValueError, match="Smoother was built for"):
            sm(d[:1], w[:1])


def test_edge_weights_stage_behind_the_prefetcher(nconv_amd, gpu):
    g = torch.Generator().manual_seed(4)
    batches = [{"rgb": torch.randint(0, 256, (2, 3, 17, 65), generator=g).float(), "depth": torch.rand(2, 1, 17, 65, generator=g),
                "name": n} for n in ("a", "b")]
    stage = nconv_amd.EdgeWeights()
    got = list(nconv_amd.data.DevicePrefetcher(batches, gpu, ingest=stage))
    torch.cuda.synchronize()
    assert len(got) == 2
    for raw, b in zip(batches, got):
        assert sorted(b) == ["depth", "edge_w", "name", "rgb"] and b["name"] == raw["name"]
        assert torch.equal(b["rgb"].cpu(), raw["rgb"]) and torch.equal(b["depth"].cpu(), raw["depth"])
        assert torch.equal(b["edge_w"], nconv_amd.edge_weights(b["rgb"]))
        assert np.array_equal(b["edge_w"].cpu().numpy(), SC.edge_weights_rule(raw["rgb"].numpy()))
    # a chain runs first; other keys and another alpha
    chain = lambda batch: {**batch, "img": batch["rgb"] / 255.0}  # noqa: E731
    b = nconv_amd.EdgeWeights(alpha=1.0, chain=chain, rgb_key="img", out_key="w")({"rgb": batches[0]["rgb"].to(gpu)})
    assert sorted(b) == ["img", "rgb", "w"] and torch.equal(b["w"], nconv_amd.edge_weights(b["img"], 1.0))


def test_gpu_argument_checks(nconv_amd, gpu):
    d = torch.ones(2, 1, 8, 16, device=gpu)
    w = torch.ones(2, 2, 8, 16, device=gpu)
    with pytest.raises(ValueError, match="weights requires a gradient"):
        nconv_amd.smoothness_loss(d, w.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.smoothness_loss(d.cpu(), w)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.smoothness_loss(d, w.cpu())
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.smoothness_loss(d, mask=torch.ones(2, 1, 8, 16, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.edge_weights(torch.ones(2, 3, 8, 16))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.Smoother((8, 16), B=2, device=gpu)(d.cpu())
    with pytest.raises(RuntimeError, match="out\\['weights'\\] on"):
        nconv_amd.edge_weights(torch.ones(2, 3, 8, 16, device=gpu), out=torch.empty(2, 2, 8, 16))


def test_graphed_step_with_the_self_supervised_objective(nconv_amd, gpu):
    """A GraphedTrainStep on a small DNET (2 x 64 x 96, test_graphed_step_with_photometric_term's shape) whose
    loss is calculate_loss + w1 photo(pred, k, rgb, rgb_near, m) + w2 smooth(pred, edge_w), replayed three
    times: the parameters and the loss are the eager steps' bit for bit, and edge weights refilled in place
    between replays change the step."""
    g = torch.Generator().manual_seed(6)
    S = sparse_depth(g, 2, 64, 96, density=0.1).to(gpu)
    gt = ((torch.rand(2, 1, 64, 96, generator=g) * 80) * (torch.rand(2, 1, 64, 96, generator=g) < 0.3)).to(gpu)
    rgb = torch.rand(2, 3, 64, 96, generator=g).to(gpu)
    near = torch.rand(2, 3, 64, 96, generator=g).to(gpu)
    k = torch.tensor(WC.intrinsics(64, 96, 80.0), dtype=torch.float32, device=gpu)
    pose = torch.tensor(np.stack([WC.rigid(0.004, -0.006, 0.003, (0.12, -0.04, 0.45))] * 2), device=gpu)
    m0 = nconv_amd.warp_projection(k, pose)
    e0 = nconv_amd.edge_weights(rgb, alpha=1.0)
    w1, w2 = 0.1, 0.05

    def setup(order):
        torch.manual_seed(0)
        net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu)
        net.train()
        opt = nconv_amd.train.get_optimizer(net, "adam", 1e-2, 1e-7, capturable=True)
        photo = nconv_amd.PhotometricLoss(z_min=1e-3)
        smooth = nconv_amd.SmoothnessLoss(order=order)

        def fn(model, s, t, a, b, m, e):
            pred = model(s)
            return nconv_amd.train.calculate_loss(pred, t, True) + w1 * photo(pred, k, a, b, m) + w2 * smooth(pred, e)
        return net, opt, fn

    net_e, opt_e, fn_e = setup(1)
    net_g, opt_g, fn_g = setup(1)
    net_r, opt_r, fn_r = setup(1)  # the control: three eager steps that keep e0
    step = nconv_amd.train.GraphedTrainStep(net_g, opt_g, fn_g, (S, gt, rgb, near, m0, e0))

    def eager(net, opt, fn, ee):
        opt.zero_grad(set_to_none=True)
        loss = fn(net, S, gt, rgb, near, m0, ee)
        loss.backward()
        opt.step()
        return loss.item()

    def both(ee):
        le = eager(net_e, opt_e, fn_e, ee)
        lg = step(S, gt, rgb, near, m0, ee)
        torch.cuda.synchronize()
        assert le == lg.item()
        for (n, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), n
        return le

    assert both(e0) == eager(net_r, opt_r, fn_r, e0)
    assert both(e0) == eager(net_r, opt_r, fn_r, e0)
    e1 = nconv_amd.edge_weights(rgb, alpha=8.0)
    step.static_inputs[5].copy_(e1)  # in place, in the step's own buffer
    l3, l3_kept = both(step.static_inputs[5]), eager(net_r, opt_r, fn_r, e0)
    assert np.isfinite(l3) and l3 != l3_kept
    assert any(not torch.equal(a, b) for a, b in zip(net_g.state_dict().values(), net_r.state_dict().values()))
