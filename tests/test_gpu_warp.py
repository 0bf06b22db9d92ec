"""The view warp and the fused photometric loss (warp.view_warp / photometric_loss: nconv_view_warp_*,
nconv_photo_loss_*) on the GPU: bit for bit against the fp32 rule restated in numpy
(warp_cases.rule_fp32), the loss within the derived summation bound, exact constructions that need no
reference, strided views, the fused path against the unfused one, and a captured training step."""
import numpy as np
import pytest
import torch

import reduce_tree as RT
import warp_cases as WC
from test_gpu_dnet import sparse_depth

pytestmark = pytest.mark.gpu


def _dev(x, gpu):
    t = {key: (None if v is None else torch.as_tensor(v).to(gpu)) for key, v in x.items()}
    t["depth"] = t["depth"][:, None]
    if t["mask"] is not None:
        t["mask"] = t["mask"][:, None]
    return t


def _run(nconv_amd, t, gloss=None):
    """(warped, valid, g_depth through view_warp, loss, n_v, g_depth through the fused loss)."""
    d = t["depth"].detach().requires_grad_(True)
    warped, valid = nconv_amd.view_warp(d, t["k"], t["src"], t["m"], t["mask"], return_valid=True)
    warped.backward(t["g_warped"])
    g_w = d.grad
    d2 = t["depth"].detach().requires_grad_(True)
    L, n_v = nconv_amd.photometric_loss(d2, t["k"], t["tgt"], t["src"], t["m"], t["mask"], return_valid_count=True)
    L.backward(gloss)
    torch.cuda.synchronize()
    return warped.detach(), valid, g_w, L.detach().clone(), n_v.clone(), d2.grad


def _check(nconv_amd, x, t, gloss=None):
    got = _run(nconv_amd, t, gloss)
    rule = WC.rule_fp32(x["depth"], x["k"], x["src"], x["m"], x["mask"], x["tgt"], x["g_warped"],
                        gloss=1.0 if gloss is None else gloss.item())
    warped, valid, g_w, L, n_v, g_p = got
    assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), rule["valid"])
    assert np.array_equal(warped.cpu().numpy(), rule["warped"])
    assert g_w.shape == t["depth"].shape and np.array_equal(g_w[:, 0].cpu().numpy(), rule["g_depth_warp"])
    assert n_v.dtype == torch.int32 and n_v.item() == rule["n_v"]
    assert np.array_equal(g_p[:, 0].cpu().numpy(), rule["g_depth_photo"])
    # the terms are the rule's bit for bit (what the gradient's signs are taken from): only the sum differs
    L64 = rule["terms"].astype(np.float64).sum() / float(rule["den"])
    bound = WC.loss_bound(rule["terms"], rule["den"], L64)
    print(f"L {L.item():.9g} fp32-terms {L64:.9g} bound {bound:.3g} n_v {n_v.item()}")
    assert abs(L.item() - L64) <= bound
    again = _run(nconv_amd, t, gloss)  # the same bits on a second run
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    return got, rule


SHAPES = [((17, 65), (19, 70)), ((45, 67), None), ((64, 96), None)]


@pytest.mark.parametrize("per_image_m", [True, False], ids=["m_per_image", "m_shared"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("size,src_size", SHAPES, ids=["17x65_from_19x70", "45x67", "64x96"])
def test_warp_and_loss_match_rule(nconv_amd, gpu, size, src_size, C, per_image_m):
    x = WC.warp_inputs(100 * size[0] + size[1] + C, 2, C, size, src_size, per_image_m, with_mask=(C == 1))
    (_, valid, *_), rule = _check(nconv_amd, x, _dev(x, gpu))
    assert 0 < rule["n_v"] < valid.numel()  # both kinds of pixel took part


@pytest.mark.parametrize("shape", [(3, 33, 70), (17, 17, 65)], ids=["3x33x70", "17x17x65"])
def test_photo_loss_sum_is_the_stated_tree(nconv_amd, gpu, shape):
    """L bit for bit from the rule's fp32 terms summed in the order csrc/wave_ops.h states (reduce_tree.py,
    view_warp.hip's thread map): partial tiles in both directions and six tiles per image; seventeen
    images, so that a wave of the finalize stage takes a second one."""
    B, H, W = shape
    x = WC.warp_inputs(1000 * B + W, B, 3, (H, W), None, True, with_mask=False)
    t = _dev(x, gpu)
    L, n_v = nconv_amd.photometric_loss(t["depth"], t["k"], t["tgt"], t["src"], t["m"], return_valid_count=True)
    rule = WC.rule_fp32(x["depth"], x["k"], x["src"], x["m"], None, x["tgt"])
    want = RT.loss(rule["terms"], float(rule["den"]), RT.ROWS)
    print(f"L {L.item():.9g} tree {want:.9g} n_v {n_v.item()}")
    assert n_v.item() == rule["n_v"] and 0 < rule["n_v"] < B * H * W
    assert RT.same_bits(L.item(), want)


@pytest.mark.parametrize("C", [1, 3])
def test_one_by_one(nconv_amd, gpu, C):
    """A 1 x 1 target from a 1 x 1 source: u = v = 0 is the only valid position. Image 0 hits it, image 1
    has no depth."""
    k = np.array([[64, 0, 0], [0, 64, 0], [0, 0, 1]], dtype=np.float32)
    x = {"depth": np.array([4.0, 0.0], dtype=np.float32).reshape(2, 1, 1), "k": k,
         "src": np.array([[0.75] * C, [0.5] * C], dtype=np.float32).reshape(2, C, 1, 1),
         "tgt": np.full((2, C, 1, 1), 0.25, dtype=np.float32), "m": (k.astype(np.float64) @ WC.rigid()).astype(np.float32),
         "mask": None, "g_warped": np.ones((2, C, 1, 1), dtype=np.float32)}
    (warped, valid, _, L, n_v, _), rule = _check(nconv_amd, x, _dev(x, gpu))
    assert valid.flatten().tolist() == [True, False] and n_v.item() == 1
    assert warped.flatten().tolist() == [0.75] * C + [0.0] * C and L.item() == 0.5


def _exact_setup(gpu, B=2, C=3, H=21, W=70, t=(0.0, 0.0, 0.0), depth=4.0):
    g = torch.Generator().manual_seed(7)
    src = torch.rand(B, C, H, W, generator=g).to(gpu)
    k = torch.tensor([[64.0, 0, 30], [0, 64.0, 9], [0, 0, 1]], device=gpu)
    d = torch.full((B, 1, H, W), depth, device=gpu)
    pose = torch.tensor(WC.rigid(t=t), device=gpu)
    return d, k, src, pose


def test_identity_pose_returns_the_source(nconv_amd, gpu):
    """fx = fy = 64, integer cx, cy, depth 4 and the identity pose: u = j, v = i exactly."""
    d, k, src, pose = _exact_setup(gpu)
    warped, valid = nconv_amd.view_warp(d, k, src, nconv_amd.warp_projection(k, pose), return_valid=True)
    assert valid.all() and torch.equal(warped, src)


def test_half_metre_sideways_shifts_by_eight_columns(nconv_amd, gpu):
    """t = (0.5, 0, 0) in the same setup: u = j + 8 exactly; the last 8 columns leave the source."""
    d, k, src, pose = _exact_setup(gpu, t=(0.5, 0.0, 0.0))
    W = src.shape[-1]
    d.requires_grad_(True)
    L, n_v = nconv_amd.photometric_loss(d, k, torch.zeros_like(src), src, nconv_amd.warp_projection(k, pose),
                                        return_valid_count=True)
    L.backward()
    warped, valid = nconv_amd.view_warp(d.detach(), k, src, nconv_amd.warp_projection(k, pose), return_valid=True)
    assert valid[..., :W - 8].all() and not valid[..., W - 8:].any()
    assert torch.equal(warped[..., :W - 8], src[..., 8:]) and (warped[..., W - 8:] == 0).all()
    assert n_v.item() == valid.sum().item() and (d.grad[..., W - 8:] == 0).all()
    assert (d.grad[..., :W - 9] != 0).any()


def test_invalid_pixels_have_no_value_count_or_gradient(nconv_amd, gpu):
    """c <= 0 (a point behind the source camera), a NaN, infinite, zero or negative depth, a depth outside
    [z_min, z_max] and a mask of 0 are not valid: warped 0, not in n_v, g_depth 0."""
    d, k, src, pose = _exact_setup(gpu, t=(0.0, 0.0, -1.0), depth=8.0)  # c = z - 1: u = 8 j / 7, v = 8 i / 7
    d[:, :, 0] = 0.5           # c = -0.5, a row each
    d[:, :, 1] = 1.0           # c = 0
    d[:, :, 2] = float("nan")
    d[:, :, 3] = float("inf")
    d[:, :, 4] = 0.0
    d[:, :, 5] = -8.0
    d[:, :, 6] = 0.125         # below z_min
    d[:, :, 7] = 100.0         # above z_max
    mask = torch.ones(d.shape, dtype=torch.bool, device=gpu)
    mask[:, :, 8] = False
    m = nconv_amd.warp_projection(k, pose)
    d.requires_grad_(True)
    L, n_v = nconv_amd.photometric_loss(d, k, torch.zeros_like(src), src, m, mask, z_min=0.25, z_max=50.0,
                                        return_valid_count=True)
    L.backward()
    warped, valid = nconv_amd.view_warp(d.detach(), k, src, m, mask, z_min=0.25, z_max=50.0, return_valid=True)
    assert not valid[:, :9].any() and valid[:, 9:].any()
    assert (warped[:, :, :9] == 0).all() and (d.grad[:, :, :9] == 0).all() and torch.isfinite(d.grad).all()
    assert n_v.item() == valid.sum().item() > 0 and torch.isfinite(L)
    want = warped.double().abs().sum() / (src.shape[1] * n_v.item())
    assert abs(L.item() - want.item()) <= 1e-5 * want.item()


def test_cropped_strided_views(nconv_amd, gpu):
    """depth cropped out of a larger buffer at an odd offset (1e30 outside), src, tgt and the mask out of
    others with other strides: the results are the contiguous ones."""
    x = WC.warp_inputs(21, 2, 3, (45, 67), (47, 70), True, with_mask=True)
    t = _dev(x, gpu)
    want = _run(nconv_amd, t)
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
    got = _run(nconv_amd, v)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert got[2].is_contiguous() and got[5].is_contiguous()


def test_fused_loss_is_the_unfused_path(nconv_amd, gpu):
    """photometric_loss against view_warp followed by torch's masked L1 mean (within the summation bound),
    and its g_depth against view_warp's backward fed g_s = kk sign(warped - tgt) with kk built by the
    rule's three fp32 operations: bit for bit. gloss scales through kk."""
    x = WC.warp_inputs(33, 2, 3, (45, 67), None, True, with_mask=False)
    t = _dev(x, gpu)
    C = 3
    for gloss in (None, torch.tensor(3.0, device=gpu)):
        warped, valid, _, L, n_v, g_p = _run(nconv_amd, t, gloss)
        diff = warped - t["tgt"]
        vf = valid[:, None].float()
        unfused = (diff.double().abs() * vf).sum() / (C * n_v.item())
        terms = (diff.abs() * vf).sum(1)
        den = np.float32(C) * np.float32(n_v.item())
        assert abs(L.item() - unfused.item()) <= WC.loss_bound(terms.cpu().numpy(), den, unfused.item()) + \
            3 * WC.U * unfused.item()  # torch's terms are summed over the channels in double, the rule's in fp32
        kk = float(np.float32(1.0 if gloss is None else gloss.item()) * (np.float32(1.0) / den))
        d = t["depth"].detach().requires_grad_(True)
        nconv_amd.view_warp(d, t["k"], t["src"], t["m"]).backward(kk * torch.sign(diff))
        assert torch.equal(d.grad, g_p)


def test_view_warper_keeps_its_buffers_and_replays(nconv_amd, gpu):
    """ViewWarper: no allocation after construction, so the warp and the loss with its backward are
    captured and replayed; refilling m in place changes the replay's results to the eager ones."""
    x = WC.warp_inputs(41, 2, 3, (17, 65), (19, 70), True, with_mask=False)
    t = _dev(x, gpu)
    vw = nconv_amd.ViewWarper((17, 65), (19, 70), B=2, C=3, device=gpu)
    d = t["depth"].clone().requires_grad_(True)
    m = t["m"].clone()
    seed = torch.ones((), device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vw.loss(d, t["k"], t["tgt"], t["src"], m).backward(seed)
    torch.cuda.current_stream().wait_stream(side)
    d.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        warped = vw(d.detach(), t["k"], t["src"], m)
        L = vw.loss(d, t["k"], t["tgt"], t["src"], m)
        L.backward(seed)
    assert warped.data_ptr() == vw._warp["warped"].data_ptr() and L.data_ptr() == vw._loss["loss"].data_ptr()
    seen = []
    for scale in (1.0, 0.5):
        m.copy_(t["m"])
        m[:, :, 3] *= scale  # another translation
        graph.replay()
        torch.cuda.synchronize()
        rule = WC.rule_fp32(x["depth"], x["k"], x["src"], m.cpu().numpy(), None, x["tgt"])
        assert np.array_equal(warped.cpu().numpy(), rule["warped"])
        assert np.array_equal(d.grad[:, 0].cpu().numpy(), rule["g_depth_photo"])
        assert L.item() == nconv_amd.photometric_loss(t["depth"], t["k"], t["tgt"], t["src"], m).item()
        seen.append((L.item(), d.grad.clone()))
    assert seen[0][0] != seen[1][0] and not torch.equal(seen[0][1], seen[1][1])
    with pytest.raises(ValueError, match="ViewWarper was built for"):
        vw(t["depth"][:1], t["k"], t["src"][:1], m[:1])


def test_gpu_argument_checks(nconv_amd, gpu):
    x = WC.warp_inputs(5, 2, 3, (8, 16), None, True, with_mask=False)
    t = _dev(x, gpu)
    with pytest.raises(ValueError, match="scatter"):
        nconv_amd.view_warp(t["depth"], t["k"], t["src"].clone().requires_grad_(True), t["m"])
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.view_warp(t["depth"], t["k"], t["src"].cpu(), t["m"])
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.photometric_loss(t["depth"], t["k"], t["tgt"].cpu(), t["src"], t["m"])


def test_graphed_step_with_photometric_term(nconv_amd, gpu):
    """A GraphedTrainStep on a small DNET (2 x 64 x 96) whose loss is calculate_loss + w * photo(pred, k,
    rgb, rgb_near, m), replayed three times: the parameters and the loss are the eager steps' bit for bit,
    and m changed in place between replays changes the step (the third is the eager one's with the new m,
    not with the captured one)."""
    g = torch.Generator().manual_seed(6)
    S = sparse_depth(g, 2, 64, 96, density=0.1).to(gpu)
    gt = ((torch.rand(2, 1, 64, 96, generator=g) * 80) * (torch.rand(2, 1, 64, 96, generator=g) < 0.3)).to(gpu)
    rgb = torch.rand(2, 3, 64, 96, generator=g).to(gpu)
    near = torch.rand(2, 3, 64, 96, generator=g).to(gpu)
    k = torch.tensor(WC.intrinsics(64, 96, 80.0), dtype=torch.float32, device=gpu)
    pose = torch.tensor(np.stack([WC.rigid(0.004, -0.006, 0.003, (0.12, -0.04, 0.45))] * 2), device=gpu)
    m0 = nconv_amd.warp_projection(k, pose)
    w = 0.1

    def setup():
        torch.manual_seed(0)
        net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu)
        net.train()
        opt = nconv_amd.train.get_optimizer(net, "adam", 1e-2, 1e-7, capturable=True)
        photo = nconv_amd.PhotometricLoss(z_min=1e-3)

        def fn(model, s, t, a, b, m):
            pred = model(s)
            return nconv_amd.train.calculate_loss(pred, t, True) + w * photo(pred, k, a, b, m)
        return net, opt, fn

    net_e, opt_e, fn_e = setup()
    net_g, opt_g, fn_g = setup()
    net_r, opt_r, fn_r = setup()  # the control: three eager steps that keep m0
    step = nconv_amd.train.GraphedTrainStep(net_g, opt_g, fn_g, (S, gt, rgb, near, m0))

    def eager(net, opt, fn, mm):
        opt.zero_grad(set_to_none=True)
        loss = fn(net, S, gt, rgb, near, mm)
        loss.backward()
        opt.step()
        return loss.item()

    def both(mm):
        le = eager(net_e, opt_e, fn_e, mm)
        lg = step(S, gt, rgb, near, mm)
        torch.cuda.synchronize()
        assert le == lg.item()
        for (n, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), n
        return le

    assert both(m0) == eager(net_r, opt_r, fn_r, m0)
    assert both(m0) == eager(net_r, opt_r, fn_r, m0)
    m1 = m0.clone()
    m1[:, :, 3] *= 0.25
    step.static_inputs[4].copy_(m1)  # in place, in the step's own buffer
    l3, l3_kept = both(step.static_inputs[4]), eager(net_r, opt_r, fn_r, m0)
    assert np.isfinite(l3) and l3 != l3_kept
    assert any(not torch.equal(a, b) for a, b in zip(net_g.state_dict().values(), net_r.state_dict().values()))
