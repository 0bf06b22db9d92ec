"""The fused confidence loss (train.ConfLossFn: nconv_conf_loss_fwd / _bwd) on the GPU against the fp32
rule restated in numpy (bit for bit per element) and the float64 sum (within the derived bound)."""
import numpy as np
import pytest
import torch

import confloss_cases as CC
import reduce_tree as RT

pytestmark = pytest.mark.gpu


def _run(nconv_amd, r, c, t, lam, err, beta, gloss=None):
    r = r.detach().requires_grad_(True)
    c = c.detach().requires_grad_(True)
    L = nconv_amd.confidence_loss(r, t, c, lam, err, beta)
    L.backward(gloss)
    torch.cuda.synchronize()
    return L.detach(), r.grad, c.grad


def _check(nconv_amd, r, c, t, lam, err, beta):
    L, g_r, g_c = _run(nconv_amd, r, c, t, lam, err, beta)
    rn, cn, tn = (x.detach().cpu().numpy() for x in (r, c, t))
    terms, want_r, want_c = CC.rule_fp32(rn, cn, tn, lam, err, beta)
    assert np.array_equal(g_r.cpu().numpy(), want_r) and np.array_equal(g_c.cpu().numpy(), want_c)
    L64 = terms.astype(np.float64).sum() / terms.size  # the fp32 terms are the kernel's: only the sum differs
    exact = CC.published_loss(r.detach().double().cpu(), c.detach().double().cpu(), t.double().cpu(), lam, err, beta)
    bound = CC.loss_bound(rn, cn, tn, lam, err, beta)
    print(f"L {L.item():.9g} fp32-terms {L64:.9g} float64 {exact.item():.9g} bound {bound:.3g}")
    assert abs(L.item() - exact.item()) <= bound
    L2, g_r2, g_c2 = _run(nconv_amd, r, c, t, lam, err, beta)  # the same bits on a second run
    assert torch.equal(L, L2) and torch.equal(g_r, g_r2) and torch.equal(g_c, g_c2)


@pytest.mark.parametrize("err,beta,lam", [("smooth_l1", 1.0, 1.0), ("smooth_l1", 0.5, 0.25), ("l2", 1.0, 0.5)])
@pytest.mark.parametrize("H,W", [(64, 96), (45, 67), (1, 1)])
def test_conf_loss_matches_rule(nconv_amd, gpu, H, W, err, beta, lam):
    g = torch.Generator().manual_seed(100 * H + W)
    r, c, t = CC.loss_inputs(g, (2, 1, H, W), beta)
    if H == 1:  # both pixels valid, one on each smooth-L1 branch
        t = torch.tensor([3.0, 5.0]).reshape(2, 1, 1, 1)
        r = torch.tensor([3.25, 9.0]).reshape(2, 1, 1, 1)
        c = torch.tensor([1.0, 0.5]).reshape(2, 1, 1, 1)
    _check(nconv_amd, r.to(gpu), c.to(gpu), t.to(gpu), lam, err, beta)


@pytest.mark.parametrize("shape", [(3, 33, 70), (17, 17, 65)], ids=["3x33x70", "17x17x65"])
def test_conf_loss_sum_is_the_stated_tree(nconv_amd, gpu, shape):
    """L bit for bit from the rule's fp32 terms summed in the order csrc/wave_ops.h states (reduce_tree.py,
    conf_loss.hip's thread map): partial tiles in both directions and six tiles per image; seventeen
    images, so that a wave of the finalize stage takes a second one."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * B + W)
    r, c, t = CC.loss_inputs(g, (B, 1, H, W))
    L = nconv_amd.confidence_loss(r.to(gpu), t.to(gpu), c.to(gpu), 0.5)
    terms, _, _ = CC.rule_fp32(r.numpy(), c.numpy(), t.numpy(), 0.5)
    want = RT.loss(terms.reshape(B, H, W), float(B * H * W), RT.QUAD)
    print(f"L {L.item():.9g} tree {want:.9g}")
    assert RT.same_bits(L.item(), want)


@pytest.mark.parametrize("err", ["smooth_l1", "l2"])
def test_conf_loss_on_cropped_strided_views(nconv_amd, gpu, err):
    """r and c cropped out of larger buffers at an odd offset (the rows are not 16-byte aligned: the
    per-element loads), t out of another with other strides."""
    g = torch.Generator().manual_seed(9)
    r, c, t = CC.loss_inputs(g, (2, 1, 45, 67))
    big_r = torch.full((2, 1, 49, 71), 1e30, device=gpu)
    big_c = torch.full((2, 1, 49, 71), 1e30, device=gpu)
    big_t = torch.full((2, 1, 47, 80), 1e30, device=gpu)
    rv, cv, tv = big_r[:, :, 1:46, 1:68], big_c[:, :, 1:46, 1:68], big_t[:, :, 2:47, 4:71]
    rv.copy_(r), cv.copy_(c), tv.copy_(t)
    assert not rv.is_contiguous() and not tv.is_contiguous()
    _check(nconv_amd, rv, cv, tv, 1.0, err, 1.0)
    L, g_r, g_c = _run(nconv_amd, rv, cv, tv, 1.0, err, 1.0)
    assert g_r.is_contiguous() and g_c.is_contiguous() and g_r.shape == (2, 1, 45, 67)


def test_conf_loss_gloss_and_single_gradient(nconv_amd, gpu):
    g = torch.Generator().manual_seed(10)
    r, c, t = (x.to(gpu) for x in CC.loss_inputs(g, (2, 1, 33, 65)))
    _, g_r, g_c = _run(nconv_amd, r, c, t, 0.5, "smooth_l1", 1.0, gloss=torch.tensor(3.0, device=gpu))
    _, want_r, want_c = CC.rule_fp32(r.cpu().numpy(), c.cpu().numpy(), t.cpu().numpy(), 0.5, gloss=3.0)
    assert np.array_equal(g_r.cpu().numpy(), want_r) and np.array_equal(g_c.cpu().numpy(), want_c)
    rr = r.clone().requires_grad_(True)  # only the prediction needs a gradient
    nconv_amd.confidence_loss(rr, t, c, 0.5).backward()
    _, one_r, _ = CC.rule_fp32(r.cpu().numpy(), c.cpu().numpy(), t.cpu().numpy(), 0.5)
    assert np.array_equal(rr.grad.cpu().numpy(), one_r)


def test_conf_loss_lam_is_read_at_replay(nconv_amd, gpu):
    """A captured forward + backward reads the device lam when it runs: set_epoch between two replays
    changes the loss and both gradients to the new value's."""
    g = torch.Generator().manual_seed(11)
    r, c, t = (x.to(gpu) for x in CC.loss_inputs(g, (2, 1, 64, 96)))
    loss = nconv_amd.ConfidenceLoss(p=1.0).to(gpu)
    r.requires_grad_(True), c.requires_grad_(True)
    seed = torch.ones((), device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss((r, c), t).backward(seed)
    torch.cuda.current_stream().wait_stream(side)
    r.grad = c.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L = loss((r, c), t)
        L.backward(seed)
    got = {}
    for p in (1.0, 4.0):
        loss.set_epoch(p)
        graph.replay()
        torch.cuda.synchronize()
        got[p] = (L.item(), r.grad.clone(), c.grad.clone())
        _, want_r, want_c = CC.rule_fp32(r.detach().cpu().numpy(), c.detach().cpu().numpy(), t.cpu().numpy(), 1.0 / p)
        assert np.array_equal(got[p][1].cpu().numpy(), want_r) and np.array_equal(got[p][2].cpu().numpy(), want_c)
        eager = nconv_amd.confidence_loss(r.detach(), t, c.detach(), 1.0 / p)
        assert eager.item() == got[p][0]
    assert got[1.0][0] != got[4.0][0] and not torch.equal(got[1.0][2], got[4.0][2])


def test_conf_loss_refuses_bad_operands(nconv_amd, gpu):
    x = torch.ones(2, 1, 4, 8, device=gpu)
    with pytest.raises(ValueError, match="err must be"):
        nconv_amd.confidence_loss(x, x, x, 1.0, err="l1")
    with pytest.raises(ValueError, match="beta must be positive"):
        nconv_amd.confidence_loss(x, x, x, 1.0, beta=0.0)
    with pytest.raises(ValueError, match="one shape"):
        nconv_amd.confidence_loss(x, x, x[:, :, :2], 1.0)
    with pytest.raises(ValueError, match="fp32 device plane"):
        nconv_amd.confidence_loss(x, x, x.double(), 1.0)
    with pytest.raises(ValueError, match="tensor lam"):
        nconv_amd.confidence_loss(x, x, x, torch.ones(1))
