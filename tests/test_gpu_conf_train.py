"""Training the output confidence: DNET.forward_with_confidence under autograd, nconv7's cout gradient in
the fused tail backward (nconv_bwd_tail_conf) and in the unfused one, against the float64 oracle, against
each other, and in a captured training step. Every case B = 2."""
import numpy as np
import pytest
import torch

import confloss_cases as CC
from oracle import nconv_ref as R
from test_gpu_dnet import make_net, oracle_params, sparse_depth

pytestmark = pytest.mark.gpu


def _gt(g, shape):
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 80) * \
        (torch.rand(shape, generator=g, dtype=torch.float64) < 0.3)


def _snapshot(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("crop", ["literal", "generalized"])
@pytest.mark.parametrize("H,W", [(64, 96), (45, 67)])
def test_forward_with_confidence_under_grad(nconv_amd, gpu, H, W, crop):
    """In training mode under autograd the pair is differentiable and the depth is forward(S)'s bit for
    bit (the weights restored in between: a training forward applies EnforcePos to them); the confidence
    is the inference path's within the forward's bound (1e-4 |ref| + 1e-6, test_gpu_dnet.py)."""
    net = make_net(nconv_amd, crop, gpu)
    net.train()
    S = sparse_depth(torch.Generator().manual_seed(H + W), 2, H, W).to(gpu)
    sd = _snapshot(net)
    want = net(S)
    net.load_state_dict(sd)
    depth, conf = net.forward_with_confidence(S)
    assert depth.requires_grad and conf.requires_grad and depth.grad_fn is not None and conf.grad_fn is not None
    assert depth.shape == conf.shape == want.shape
    assert torch.equal(depth, want)
    (depth.sum() + conf.sum()).backward()
    for n, p in net.d_net.named_parameters():
        if "bnorm" not in n:  # (the nine NConv layers: every one is reached from the outputs)
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    net.eval()
    with torch.no_grad():
        _, conf_i = net.forward_with_confidence(S)  # (the weights are the drifted ones: what the pass above used)
    assert ((conf.detach() - conf_i).abs() <= 1e-4 * conf_i.abs() + 1e-6).all()
    with pytest.raises(RuntimeError, match="inference only"):  # eval mode under grad stays refused
        net.forward_with_confidence(S)


def _grads_vs_oracle(nconv_amd, gpu, H, W, crop, loss_gpu, loss_ref, seed=11):
    """The recipe of test_gpu_dnet._train_gradients_vs_oracle with forward_with_confidence: the fp64 oracle
    on the EnforcePos-drifted weights and on the GPU's pool winners; the normwise error of each of the 18
    parameter gradients."""
    net = make_net(nconv_amd, crop, gpu)
    net.train()
    g = torch.Generator().manual_seed(seed)
    S = sparse_depth(g, 2, H, W)
    params0 = oracle_params(net)
    net.d_net.capture = {}
    depth, conf = net.forward_with_confidence(S.to(gpu))
    cap, net.d_net.capture = net.d_net.capture, None
    idx = {k: tuple(torch.nn.functional.max_pool2d(t, 2, 2, return_indices=True)[1].cpu() for t in v)
           for k, v in cap.items()}
    params = {n: (R.softplus_pos(w).detach().requires_grad_(True), b.detach().requires_grad_(True))
              for n, (w, b) in params0.items()}
    rd, rc = CC.dnet_forward_with_confidence(S.double(), params, crop, pool_idx=idx)
    assert rd.shape == depth.shape
    gt = _gt(g, rd.shape)
    cot = torch.rand(rd.shape, generator=g, dtype=torch.float64) - 0.3
    loss_ref(rd, rc, gt, cot).backward()
    loss_gpu(depth, conf, gt.to(gpu, torch.float32), cot.to(gpu, torch.float32)).backward()
    torch.cuda.synchronize()
    named = dict(net.named_parameters())
    report = {}
    for n, (w, b) in params.items():
        for lab, ref_t in (("weight", w), ("bias", b)):
            got = named[f"d_net.{n}.{lab}"].grad.double().cpu()
            want = ref_t.grad if ref_t.grad is not None else torch.zeros_like(ref_t)  # (no path to the loss)
            report[f"{n}.{lab}"] = (((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item(),
                                    want.abs().max().item())
    return report


@pytest.mark.parametrize("crop", ["literal", "generalized"])
@pytest.mark.parametrize("H,W", [(64, 96), (45, 67)])
def test_confidence_loss_gradients_vs_oracle(nconv_amd, gpu, H, W, crop):
    """confidence_loss (lam = 1) on (depth, conf): all 18 parameter gradients normwise within 1e-3 of the
    float64 oracle. 64 x 96 takes the fused tail (generalized: the cropped one), 45 x 67 the unfused
    branch (odd: no exactly-2x upsample)."""
    rep = _grads_vs_oracle(
        nconv_amd, gpu, H, W, crop,
        lambda d, c, gt, cot: nconv_amd.confidence_loss(d, gt, c, 1.0),
        lambda d, c, gt, cot: CC.published_loss(d, c, gt, 1.0))
    print("\n".join(f"{k}: {v[0]:.2e}" for k, v in rep.items()))
    assert len(rep) == 18
    assert all(v[0] <= 1e-3 for v in rep.values()), rep


@pytest.mark.parametrize("H,W", [(64, 96), (45, 67)])
def test_confidence_only_gradients_vs_oracle(nconv_amd, gpu, H, W):
    """A loss on the confidence alone, (conf * cotangent).sum() with a fixed random cotangent, g9 = 0: the
    new term in isolation. The weight gradients are non-zero and within 1e-3 of the oracle; the confidence
    does not depend on any bias (cout = conv(c, w) / s), so the bias gradients are exactly 0 on both sides."""
    rep = _grads_vs_oracle(nconv_amd, gpu, H, W, "generalized",
                           lambda d, c, gt, cot: (c * cot).sum(), lambda d, c, gt, cot: (c * cot).sum())
    print("\n".join(f"{k}: {v[0]:.2e} (max |ref| {v[1]:.2e})" for k, v in rep.items()))
    assert len(rep) == 18
    assert all(v == (0.0, 0.0) for k, v in rep.items() if k.endswith(".bias")), rep
    assert all(v[1] > 0 and v[0] <= 1e-3 for k, v in rep.items() if k.endswith(".weight")), rep


@pytest.mark.parametrize("frozen", [(), ("nconv6.weight", "nconv6.bias"), ("nconv6.weight",), ("nconv6.bias",)])
def test_fused_tail_matches_unfused_with_confidence_gradient(nconv_amd, gpu, monkeypatch, frozen):
    """test_frozen_layers_fused_tail_matches_unfused with gc9 != 0 (confidence_loss, lam = 1): every
    trainable gradient of the fused tail backward within 1e-5 normwise of the unfused path's -- nconv7's
    weight in particular, which carries the normaliser term gs7."""
    g = torch.Generator().manual_seed(91)
    S = sparse_depth(g, 2, 64, 96).to(gpu)
    gt = _gt(g, (2, 1, 64, 96)).to(gpu, torch.float32)
    grads = {}
    for fused in (True, False):
        monkeypatch.setattr(nconv_amd.dnet, "FUSE_TAIL_BWD", fused)
        net = make_net(nconv_amd, "generalized", gpu)
        for n, p in net.d_net.named_parameters():
            p.requires_grad_(n not in frozen)
        net.train()
        depth, conf = net.forward_with_confidence(S)
        nconv_amd.confidence_loss(depth, gt, conf, 1.0).backward()
        torch.cuda.synchronize()
        grads[fused] = {n: (p.grad.detach().clone() if p.grad is not None else None)
                        for n, p in net.d_net.named_parameters() if "bnorm" not in n}
    for n, a in grads[True].items():
        b = grads[False][n]
        assert (a is None) == (b is None) == (n in frozen), n
        if a is None:
            continue
        assert torch.isfinite(a).all(), n
        rel = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
        assert rel <= 1e-5, f"{n}: {rel:.2e}"
    assert grads[True]["nconv7.weight"].abs().max() > 0


def _tail_case(nconv_amd, gpu, H, W, window):
    """nconv6 + nconv7 of a trained-like net on random inputs at H x W (even): the tensors and specs of
    the two layers' backward, nconv7's planes either its whole (H + 2) x (W + 2) grid or a window of it
    from row / column 1."""
    net = make_net(nconv_amd, "generalized", gpu).d_net
    N, lib = nconv_amd.nconv, nconv_amd._lib
    g = torch.Generator().manual_seed(H * W)
    rnd = lambda *s: torch.rand(*s, generator=g).to(gpu)  # noqa: E731
    x2, c2, x7, c7 = rnd(2, 8, H, W) * 40, rnd(2, 8, H, W), rnd(2, 8, H // 2, W // 2) * 40, rnd(2, 8, H // 2, W // 2)
    l6, l7 = net.nconv6, net.nconv7
    sp6, sp7 = l6.spec(lib.UPCAT_UP_FIRST), l7.spec()
    ws = [torch.empty(w.shape[0], device=gpu) for w in (l6.weight, l7.weight)]
    N.weight_prep([l6.weight.detach(), l7.weight.detach()], [False, False], ws)
    W6, W7 = (l6.weight.detach(), l6.bias.detach(), ws[0]), (l7.weight.detach(), l7.bias.detach(), ws[1])
    x8, c8 = N.layer_forward_raw(sp6, x2, c2, x7, c7, *W6)
    x9, c9 = N.layer_forward_raw(sp7, x8, c8, None, None, *W7)
    g9, gc9 = rnd(*x9.shape) - 0.5, rnd(*x9.shape) - 0.5
    if window is not None:  # gradient outside the window is 0
        h, w = window
        m = torch.zeros_like(g9)
        m[:, :, 1:1 + h, 1:1 + w] = 1
        g9, gc9 = g9 * m, gc9 * m
    return dict(sp6=sp6, sp7=sp7, W6=W6, W7=W7, x2=x2, c2=c2, x7=x7, c7=c7, x8=x8, c8=c8, x9=x9, c9=c9, g9=g9,
                gc9=gc9)


def _tail_fused(nconv_amd, gpu, k, window, gc9, conf_entry=True):
    N = nconv_amd.nconv
    e = torch.empty_like
    gin = N.InputGrads(e(k["x2"]), e(k["c2"]), e(k["x7"]), e(k["c7"]))
    gw6, gb6, gw7 = e(k["W6"][0]), e(k["W6"][1]), e(k["W7"][0])
    cut = (lambda t: t) if window is None else (lambda t: t[:, :, 1:1 + window[0], 1:1 + window[1]].contiguous())
    tail = N.TailBwd(k["sp7"], *k["W7"], cut(k["x9"]), cut(k["c9"]), cut(k["g9"]), gw7,
                     crop0=None if window is None else 1, gcout=None if gc9 is None else cut(gc9),
                     conf_entry=conf_entry)
    N.layer_backward(k["sp6"], N.Operands(k["x2"], k["c2"], k["x7"], k["c7"], *k["W6"]), k["x8"], k["c8"], None, None,
                     gin, gw6, gb6, tail=tail)
    torch.cuda.synchronize()
    return (*gin, gw6, gb6, gw7)


# nconv7's planes: its whole 32 x 48 grid (H x W = 30 x 46), and a 33 x 47 window of its 36 x 50 grid from
# row / column 1 (34 x 48). The fused tail needs an exactly-2x upsample, so nconv6's own grid is even.
@pytest.mark.parametrize("H,W,window", [(30, 46, None), (34, 48, (33, 47)), (34, 48, None), (30, 46, (31, 47))])
def test_tail_conf_matches_two_general_backwards(nconv_amd, gpu, H, W, window):
    """nconv_bwd_tail_conf's input gradients (gxa, gca, gxb, gcb) -- and both layers' weight gradients --
    against nconv7's general nconv_bwd with gcout, then nconv6's: normwise within 1e-5. With tail_gcout =
    NULL the new entry point writes bitwise what nconv_bwd_ex writes."""
    N = nconv_amd.nconv
    k = _tail_case(nconv_amd, gpu, H, W, window)
    got = _tail_fused(nconv_amd, gpu, k, window, k["gc9"])
    e = torch.empty_like
    g8 = (e(k["x8"]), e(k["c8"]))
    gw7 = e(k["W7"][0])
    N.layer_backward(k["sp7"], N.Operands(k["x8"], k["c8"], None, None, *k["W7"]), k["x9"], k["c9"], k["g9"],
                     k["gc9"], N.InputGrads(*g8), gw7, None)
    gin = N.InputGrads(e(k["x2"]), e(k["c2"]), e(k["x7"]), e(k["c7"]))
    gw6, gb6 = e(k["W6"][0]), e(k["W6"][1])
    N.layer_backward(k["sp6"], N.Operands(k["x2"], k["c2"], k["x7"], k["c7"], *k["W6"]), k["x8"], k["c8"], *g8, gin,
                     gw6, gb6)
    torch.cuda.synchronize()
    for name, a, b in zip(("gxa", "gca", "gxb", "gcb", "gw6", "gb6", "gw7"), got, (*gin, gw6, gb6, gw7)):
        rel = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
        print(f"{name}: {rel:.2e}")
        assert torch.isfinite(a).all() and rel <= 1e-5, f"{name}: {rel:.2e}"
    null = _tail_fused(nconv_amd, gpu, k, window, None)           # nconv_bwd_tail_conf(tail_gcout = NULL)
    ex = _tail_fused(nconv_amd, gpu, k, window, None, conf_entry=False)  # nconv_bwd_ex
    assert all(torch.equal(a, b) for a, b in zip(null, ex))
    assert not torch.equal(null[1], got[1])  # and the plane changes the result


def test_graphed_step_with_confidence_loss(nconv_amd, gpu):
    """A GraphedTrainStep of forward_with_confidence + ConfidenceLoss at 2 x 64 x 96 reproduces the eager
    steps' parameters bit for bit after two steps, and set_epoch between replays takes effect (the third
    step is the eager one's with the new lam, not with the captured one)."""
    g = torch.Generator().manual_seed(5)
    S = sparse_depth(g, 2, 64, 96, density=0.1).to(gpu)
    gt = _gt(g, (2, 1, 64, 96)).to(gpu, torch.float32)

    def setup():
        torch.manual_seed(0)
        net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu)
        net.train()
        opt = nconv_amd.train.get_optimizer(net, "adam", 1e-2, 1e-7, capturable=True)
        loss = nconv_amd.ConfidenceLoss(p=1.0).to(gpu)
        return net, opt, loss, (lambda m, s, t: loss(m.forward_with_confidence(s), t))

    net_e, opt_e, loss_e, fn_e = setup()
    net_g, opt_g, loss_g, fn_g = setup()
    net_r, opt_r, _, fn_r = setup()  # the control: three eager steps that keep lam = 1
    step = nconv_amd.train.GraphedTrainStep(net_g, opt_g, fn_g, (S, gt))

    def both():
        opt_e.zero_grad(set_to_none=True)
        le = fn_e(net_e, S, gt)
        le.backward()
        opt_e.step()
        lg = step()
        torch.cuda.synchronize()
        assert le.item() == lg.item()
        for (n, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), n
        return le.item()

    def control():
        opt_r.zero_grad(set_to_none=True)
        lr = fn_r(net_r, S, gt)
        lr.backward()
        opt_r.step()
        return lr.item()

    assert both() == control()
    assert both() == control()
    loss_e.set_epoch(5.0)
    loss_g.set_epoch(5.0)
    l3, l3_kept = both(), control()  # (a replay that kept the captured lam would part from the eager step here)
    torch.cuda.synchronize()
    assert np.isfinite(l3) and l3 != l3_kept  # and lam = 0.2 gives another step than lam = 1 does
    assert any(not torch.equal(a, b) for a, b in zip(net_g.state_dict().values(), net_r.state_dict().values()))
