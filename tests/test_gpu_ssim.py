"""The SSIM photometric loss (warp.photometric_ssim_loss: nconv_photo_ssim_loss_*) on the GPU: bit for bit
against the fp32 rule restated in numpy (ssim_cases.rule_fp32), the loss in the stated summation tree, the
L1 parity at alpha = 0, exact constructions that need no reference, strided views, the module and the
ViewWarper dispatch, and a captured training step."""
import numpy as np
import pytest
import torch

import reduce_tree as RT
import ssim_cases as SC
import warp_cases as WC
from test_gpu_dnet import sparse_depth

pytestmark = pytest.mark.gpu


def _dev(x, gpu):
    t = {key: (None if v is None or not isinstance(v, np.ndarray) else torch.as_tensor(v).to(gpu))
         for key, v in x.items()}
    t["depth"] = t["depth"][:, None]
    if t["mask"] is not None:
        t["mask"] = t["mask"][:, None]
    return t


def _run(nconv_amd, t, alpha, R, gloss=None):
    """(loss, n_v, n_w, g_depth) of the fused loss."""
    d = t["depth"].detach().requires_grad_(True)
    L, n_v, n_w = nconv_amd.photometric_ssim_loss(d, t["k"], t["tgt"], t["src"], t["m"], t["mask"], alpha=alpha,
                                                  data_range=R, return_counts=True)
    L.backward(gloss)
    torch.cuda.synchronize()
    return L.detach().clone(), n_v.clone(), n_w.clone(), d.grad


def _check(nconv_amd, x, gpu, alpha, gloss=None):
    t = _dev(x, gpu)
    R = x["data_range"]
    got = _run(nconv_amd, t, alpha, R, gloss)
    rule = SC.rule_fp32(*SC.call_args(x), alpha=alpha, data_range=R, gloss=1.0 if gloss is None else gloss.item())
    L, n_v, n_w, g = got
    print(f"L {L.item():.9g} rule {rule['L']:.9g} n_v {n_v.item()} n_w {n_w.item()}")
    assert n_v.dtype == torch.int32 and n_w.dtype == torch.int32
    assert (n_v.item(), n_w.item()) == (rule["n_v"], rule["n_w"])
    assert RT.same_bits(L.item(), rule["L"])  # the terms and their sums: the stated tree
    assert g.shape == t["depth"].shape and np.array_equal(g[:, 0].cpu().numpy(), rule["g_depth"])
    again = _run(nconv_amd, t, alpha, R, gloss)  # the same bits on a second run
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    return got, rule


SHAPES = [((3, 3), None), ((17, 65), (19, 70)), ((45, 67), None), ((64, 96), None)]


@pytest.mark.parametrize("alpha", [0.85, 1.0])
@pytest.mark.parametrize("per_image_m", [True, False], ids=["m_per_image", "m_shared"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("size,src_size", SHAPES, ids=["3x3", "17x65_from_19x70", "45x67", "64x96"])
def test_loss_and_gradient_match_rule(nconv_amd, gpu, size, src_size, C, per_image_m, alpha):
    """L (so Lw's and Lv's terms and both sums), n_v, n_w and g_depth bit for bit the rule's; the halo
    crosses tile edges in both directions and the tiles are partial; a second run gives equal bits."""
    R = 255.0 if C == 3 else 1.0
    x = SC.ssim_inputs(100 * size[0] + size[1] + C, 2, C, size, src_size, per_image_m, with_mask=(C == 1),
                       data_range=R)
    _, rule = _check(nconv_amd, x, gpu, alpha)
    if size != (3, 3):
        assert 0 < rule["n_w"] < rule["n_v"] < rule["valid"].size


def test_gloss_scales_the_gradient(nconv_amd, gpu):
    x = SC.ssim_inputs(77, 2, 3, (17, 65), (19, 70), True, False, 255.0)
    _check(nconv_amd, x, gpu, 0.85, gloss=torch.tensor(3.0, device=gpu))


def test_loss_sum_is_the_stated_tree(nconv_amd, gpu):
    """L bit for bit from the rule's fp32 terms summed in the order csrc/wave_ops.h states (reduce_tree.py):
    seventeen images, so that a wave of the finalize stage takes a second one; partial tiles."""
    B, H, W = 17, 17, 65
    x = SC.ssim_inputs(1000 * B + W, B, 3, (H, W), None, True, False, 255.0)
    t = _dev(x, gpu)
    L, n_v, n_w = nconv_amd.photometric_ssim_loss(t["depth"], t["k"], t["tgt"], t["src"], t["m"], alpha=0.85,
                                                  data_range=255.0, return_counts=True)
    rule = SC.rule_fp32(*SC.call_args(x), alpha=0.85, data_range=255.0)
    Lw = RT.loss(rule["terms_w"], float(3 * rule["n_w"]), RT.ROWS)
    Lv = RT.loss(rule["terms"], float(rule["den"]), RT.ROWS)
    want = np.float32(0.85) * Lw + (np.float32(1.0) - np.float32(0.85)) * Lv
    print(f"L {L.item():.9g} tree {want:.9g} n_v {n_v.item()} n_w {n_w.item()}")
    assert (n_v.item(), n_w.item()) == (rule["n_v"], rule["n_w"]) and 0 < rule["n_w"] < rule["n_v"] < B * H * W
    assert RT.same_bits(L.item(), want)


@pytest.mark.parametrize("C,with_mask", [(3, False), (1, True)])
def test_alpha_zero_is_the_l1_loss(nconv_amd, gpu, C, with_mask):
    """alpha = 0: the loss and the gradient are torch.equal to photometric_loss's on the same operands."""
    x = SC.ssim_inputs(31 + C, 2, C, (45, 67), (47, 70), True, with_mask, 255.0)
    t = _dev(x, gpu)
    for gloss in (None, torch.tensor(3.0, device=gpu)):
        L, n_v, _, g = _run(nconv_amd, t, 0.0, 255.0, gloss)
        d = t["depth"].detach().requires_grad_(True)
        L1, n1 = nconv_amd.photometric_loss(d, t["k"], t["tgt"], t["src"], t["m"], t["mask"], return_valid_count=True)
        L1.backward(gloss)
        assert torch.equal(L, L1) and torch.equal(g, d.grad) and n_v.item() == n1.item()


def _exact_setup(gpu, B=2, C=3, H=21, W=70):
    g = torch.Generator().manual_seed(7)
    src = (torch.rand(B, C, H, W, generator=g) * 255).to(gpu)
    k = torch.tensor([[64.0, 0, 30], [0, 64.0, 9], [0, 0, 1]], device=gpu)
    d = torch.full((B, 1, H, W), 4.0, device=gpu)
    return d, k, src


def test_identity_pose_and_equal_frames_give_zero(nconv_amd, gpu):
    """Identity pose (u = j, v = i exactly) and tgt = src: x == y, ssim == 1 exactly, L == 0, every interior
    pixel has a window."""
    d, k, src = _exact_setup(gpu)
    m = nconv_amd.warp_projection(k, torch.eye(4, device=gpu))
    B, _, H, W = src.shape
    L, n_v, n_w = nconv_amd.photometric_ssim_loss(d, k, src.clone(), src, m, return_counts=True)
    assert L.item() == 0.0 and n_v.item() == B * H * W and n_w.item() == B * (H - 2) * (W - 2)


def test_constant_frames_equal_the_scalar_formula(nconv_amd, gpu):
    """x = 0.5, y = 0.25, R = 1: every window is the scalar formula's, in fp32 operation by operation."""
    d, k, src = _exact_setup(gpu, C=1)
    m = nconv_amd.warp_projection(k, torch.eye(4, device=gpu))
    x, y = torch.full_like(src, 0.5), torch.full_like(src, 0.25)
    L = nconv_amd.photometric_ssim_loss(d, k, y, x, m, alpha=1.0, data_range=1.0)
    f = np.float32
    c1, c2 = SC.constants(1.0)
    A1, A2 = f(2) * (f(0.5) * f(0.25)) + c1, f(2) * (f(0.125) - f(0.125)) + c2
    B1, B2 = (f(0.25) + f(0.0625)) + c1, (f(0) + f(0)) + c2
    t = (f(1) - (A1 * A2) / (B1 * B2)) * f(0.5)
    B, _, H, W = src.shape
    terms = np.zeros((B, H, W), dtype=f)
    terms[:, 1:-1, 1:-1] = t  # the window sums of a constant are exact: every window's term is t itself
    assert 0 < t < 1 and RT.same_bits(L.item(), RT.loss(terms, float(B * (H - 2) * (W - 2)), RT.ROWS))


def test_no_window_is_the_l1_part_alone(nconv_amd, gpu):
    """A 2 x 5 image has no window: n_w = 0, L = (1 - alpha) Lv and the gradient is the L1 part's."""
    x = SC.ssim_inputs(9, 2, 3, (2, 5), (4, 8), True, False, 255.0)
    (L, n_v, n_w, g), rule = _check(nconv_amd, x, gpu, 0.85)
    assert n_w.item() == 0 and n_v.item() > 0
    a = np.float32(0.85)
    assert RT.same_bits(L.item(), a * np.float32(0) + (np.float32(1) - a) * rule["Lv"])
    t = _dev(x, gpu)
    d = t["depth"].detach().requires_grad_(True)
    nconv_amd.photometric_loss(d, t["k"], t["tgt"], t["src"], t["m"]).backward(
        torch.tensor(float(np.float32(1) - a), device=gpu))
    assert torch.equal(g, d.grad)


def test_three_by_three_has_one_window(nconv_amd, gpu):
    """A 3 x 3 image whose nine pixels are valid has exactly one window; one invalid pixel removes it."""
    k = torch.tensor([[64.0, 0, 1], [0, 64.0, 1], [0, 0, 1]], device=gpu)
    g = torch.Generator().manual_seed(3)
    src, tgt = torch.rand(1, 3, 3, 3, generator=g).to(gpu), torch.rand(1, 3, 3, 3, generator=g).to(gpu)
    d = torch.full((1, 1, 3, 3), 4.0, device=gpu)
    m = nconv_amd.warp_projection(k, torch.eye(4, device=gpu))
    _, n_v, n_w = nconv_amd.photometric_ssim_loss(d, k, tgt, src, m, data_range=1.0, return_counts=True)
    assert (n_v.item(), n_w.item()) == (9, 1)
    d[0, 0, 2, 0] = 0.0
    _, n_v, n_w = nconv_amd.photometric_ssim_loss(d, k, tgt, src, m, data_range=1.0, return_counts=True)
    assert (n_v.item(), n_w.item()) == (8, 0)


def test_cropped_strided_views(nconv_amd, gpu):
    """depth cropped out of a larger buffer at an odd offset (DNET's cropped output; 1e30 outside), tgt, src
    and the mask out of others with other strides: the results are the contiguous ones."""
    x = SC.ssim_inputs(21, 2, 3, (45, 67), (47, 70), True, True, 255.0)
    t = _dev(x, gpu)
    want = _run(nconv_amd, t, 0.85, 255.0)
    big_d = torch.full((2, 1, 49, 71), 1e30, device=gpu)
    big_s = torch.full((2, 4, 50, 80), 1e30, device=gpu)
    big_t = torch.full((3, 3, 47, 69), 1e30, device=gpu)
    big_m = torch.ones((2, 1, 46, 75), dtype=torch.uint8, device=gpu)
    v = dict(t)
    v["depth"], v["src"] = big_d[:, :, 3:48, 1:68], big_s[:, 1:, 2:49, 5:75]
    v["tgt"], v["mask"] = big_t[1:, :, 1:46, 2:69], big_m[:, :, 1:, 3:70]
    for key in ("depth", "src", "tgt", "mask"):
        v[key].copy_(t[key])
        assert not v[key].is_contiguous()
    got = _run(nconv_amd, v, 0.85, 255.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[3].is_contiguous()


def test_module_and_warper_dispatch(nconv_amd, gpu):
    """PhotometricLoss(alpha=0.85) and ViewWarper(alpha=0.85).loss are the function; alpha = 0 stays the L1 loss."""
    x = SC.ssim_inputs(41, 2, 3, (17, 65), (19, 70), True, False, 255.0)
    t = _dev(x, gpu)
    L, n_v, _, g = _run(nconv_amd, t, 0.85, 255.0)
    d = t["depth"].detach().requires_grad_(True)
    Lm = nconv_amd.PhotometricLoss(alpha=0.85)(d, t["k"], t["tgt"], t["src"], t["m"])
    Lm.backward()
    assert torch.equal(Lm.detach(), L) and torch.equal(d.grad, g)
    vw = nconv_amd.ViewWarper((17, 65), (19, 70), B=2, C=3, device=gpu, alpha=0.85)
    d = t["depth"].detach().requires_grad_(True)
    Lw, nv = vw.loss(d, t["k"], t["tgt"], t["src"], t["m"], return_valid_count=True)
    Lw.backward()
    assert torch.equal(Lw.detach(), L) and nv.item() == n_v.item() and torch.equal(d.grad, g)
    assert Lw.data_ptr() == vw._ssim["loss"].data_ptr() and torch.equal(vw._ssim["g_depth"], g)
    L1 = nconv_amd.photometric_loss(t["depth"], t["k"], t["tgt"], t["src"], t["m"])
    assert torch.equal(nconv_amd.PhotometricLoss()(t["depth"], t["k"], t["tgt"], t["src"], t["m"]), L1)
    plain = nconv_amd.ViewWarper((17, 65), (19, 70), B=2, C=3, device=gpu)
    assert plain._ssim is None and torch.equal(plain.loss(t["depth"], t["k"], t["tgt"], t["src"], t["m"]), L1)


def test_graphed_step_with_ssim_and_smoothness(nconv_amd, gpu):
    """A GraphedTrainStep on a small DNET (2 x 64 x 96) whose loss is calculate_loss + w photo_ssim + w2 smooth,
    replayed twice: the parameters and the loss are the eager steps' bit for bit."""
    g = torch.Generator().manual_seed(6)
    S = sparse_depth(g, 2, 64, 96, density=0.1).to(gpu)
    gt = ((torch.rand(2, 1, 64, 96, generator=g) * 80) * (torch.rand(2, 1, 64, 96, generator=g) < 0.3)).to(gpu)
    rgb = (torch.rand(2, 3, 64, 96, generator=g) * 255).to(gpu)
    near = (torch.rand(2, 3, 64, 96, generator=g) * 255).to(gpu)
    k = torch.tensor(WC.intrinsics(64, 96, 80.0), dtype=torch.float32, device=gpu)
    pose = torch.tensor(np.stack([WC.rigid(0.004, -0.006, 0.003, (0.12, -0.04, 0.45))] * 2), device=gpu)
    m0 = nconv_amd.warp_projection(k, pose)
    w, w2 = 0.01, 0.1

    def setup():
        torch.manual_seed(0)
        net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu)
        net.train()
        opt = nconv_amd.train.get_optimizer(net, "adam", 1e-2, 1e-7, capturable=True)
        photo = nconv_amd.PhotometricLoss(z_min=1e-3, alpha=0.85)

        def fn(model, s, t, a, b, m):
            pred = model(s)
            return (nconv_amd.train.calculate_loss(pred, t, True) + w * photo(pred, k, a, b, m)
                    + w2 * nconv_amd.smoothness_loss(pred))
        return net, opt, fn

    net_e, opt_e, fn_e = setup()
    net_g, opt_g, fn_g = setup()
    step = nconv_amd.train.GraphedTrainStep(net_g, opt_g, fn_g, (S, gt, rgb, near, m0))
    for _ in range(2):
        opt_e.zero_grad(set_to_none=True)
        loss = fn_e(net_e, S, gt, rgb, near, m0)
        loss.backward()
        opt_e.step()
        lg = step(S, gt, rgb, near, m0)
        torch.cuda.synchronize()
        assert np.isfinite(loss.item()) and loss.item() == lg.item()
        for (n, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), n
