"""The minimum-reprojection loss (warp.min_reprojection_loss: nconv_photo_min_loss_*) on the GPU: bit for bit
against the fp32 rule restated in numpy (minreproj_cases.min_rule_fp32), the S = 1 parities with
photometric_loss and photometric_ssim_loss, sources that each leave the frame, exact auto-mask constructions,
the source order, strided views, and capture (MinReprojector, a graphed training step)."""
import numpy as np
import pytest
import torch

import minreproj_cases as MC
import reduce_tree as RT
import warp_cases as WC
from test_gpu_dnet import sparse_depth

pytestmark = pytest.mark.gpu


def _dev(x, gpu):
    T = lambda v: torch.as_tensor(v).to(gpu)  # noqa: E731
    t = {"depth": T(x["depth"])[:, None], "k": T(x["k"]), "tgt": T(x["tgt"]),
         "mask": None if x["mask"] is None else T(x["mask"])[:, None],
         "srcs": [T(s) for s in x["srcs"]], "ms": [T(m) for m in x["ms"]]}
    return t


def _run(nconv_amd, t, alpha, R, automask, gloss=None):
    """(loss, n_c, n_m, winner, error, g_depth) of the fused loss."""
    d = t["depth"].detach().requires_grad_(True)
    L, n_c, n_m, winner, error = nconv_amd.min_reprojection_loss(
        d, t["k"], t["tgt"], t["srcs"], t["ms"], t["mask"], alpha=alpha, data_range=R, automask=automask,
        return_counts=True, return_winner=True, return_error=True)
    L.backward(gloss)
    torch.cuda.synchronize()
    return L.detach().clone(), n_c.clone(), n_m.clone(), winner, error, d.grad


def _check(nconv_amd, x, gpu, alpha, automask, gloss=None):
    t = _dev(x, gpu)
    R = x["data_range"]
    got = _run(nconv_amd, t, alpha, R, automask, gloss)
    rule = MC.min_rule_fp32(*MC.call_args(x), alpha=alpha, data_range=R, automask=automask,
                            gloss=1.0 if gloss is None else gloss.item())
    L, n_c, n_m, winner, error, g = got
    print(f"L {L.item():.9g} rule {rule['L']:.9g} n_c {n_c.item()} n_m {n_m.item()} of {rule['has'].size}")
    assert n_c.dtype == torch.int32 and n_m.dtype == torch.int32
    assert (n_c.item(), n_m.item()) == (rule["n_c"], rule["n_m"])
    assert winner.dtype == torch.uint8 and np.array_equal(winner.cpu().numpy(), rule["winner"])
    assert np.array_equal(error.cpu().numpy(), rule["error"])
    assert RT.same_bits(L.item(), rule["L"])  # the terms and their sum: the stated tree
    assert g.shape == t["depth"].shape and np.array_equal(g[:, 0].cpu().numpy(), rule["g_depth"])
    again = _run(nconv_amd, t, alpha, R, automask, gloss)  # the same bits on a second run
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    return got, rule


SHAPES = [((3, 3), None), ((17, 65), (19, 70)), ((45, 67), None), ((64, 96), None)]
IDS = ["3x3", "17x65_from_19x70", "45x67", "64x96"]


ALPHAS = [0.0, 0.85, 1.0]
# every shape, S, alpha and auto-mask setting; 17 x 65 from 19 x 70 sources with auto-masking off only
CASES = [(shape, S, ai, am) for shape in range(len(SHAPES)) for S in (1, 2, 3) for ai in range(len(ALPHAS))
         for am in (False, True) if not (am and SHAPES[shape][1] is not None)]


@pytest.mark.parametrize("shape,S,ai,automask", CASES,
                         ids=[f"{IDS[c[0]]}-S{c[1]}-alpha{ALPHAS[c[2]]}-{'automask' if c[3] else 'plain'}"
                              for c in CASES])
def test_loss_winner_and_gradient_match_rule(nconv_amd, gpu, shape, S, ai, automask):
    """L, n_c, n_m, the winner plane, the error plane and g_depth bit for bit the rule's. 45 x 67 and 64 x 96
    cross the 16 x 64 tile borders in both directions, where a halo or a winner byte read one pixel off shows.
    C, the sharing of m and the mask alternate over the cases, so that both values of each meet every S, alpha,
    auto-mask setting and shape."""
    size, src_size = SHAPES[shape]
    alpha = ALPHAS[ai]
    C = 3 if (shape + S) % 2 else 1
    per_image_m = (S + ai + int(automask)) % 2 == 0
    with_mask = (shape + ai + int(automask)) % 2 == 1
    R = 255.0 if C == 3 else 1.0
    x = MC.min_inputs(100 * size[0] + size[1] + 10 * S + C, 2, C, size, src_size, S, per_image_m, with_mask, R)
    _, rule = _check(nconv_amd, x, gpu, alpha, automask)
    if size != (3, 3):
        assert 0 < rule["n_c"] < rule["has"].size
        if S > 1:
            assert all((rule["winner"] == s).any() for s in range(S))
        if automask:
            assert 0 < rule["n_m"] < rule["n_c"]


@pytest.mark.parametrize("C,per_image_m,with_mask", [(1, True, False), (3, False, True), (3, True, False)])
def test_both_channel_counts_with_gloss(nconv_amd, gpu, C, per_image_m, with_mask):
    """gloss given (it scales kl and kq), for both channel counts, m per image and shared, with and without mask."""
    x = MC.min_inputs(77 + C, 2, C, (45, 67), None, 2, per_image_m, with_mask, 255.0)
    _check(nconv_amd, x, gpu, 0.85, True, gloss=torch.tensor(3.0, device=gpu))


@pytest.mark.parametrize("C,with_mask", [(3, False), (1, True)])
def test_one_source_alpha_zero_is_the_l1_loss(nconv_amd, gpu, C, with_mask):
    """S = 1, no auto-mask, alpha = 0: L and g_depth are torch.equal to photometric_loss's."""
    x = MC.min_inputs(31 + C, 2, C, (45, 67), (47, 70), 1, True, with_mask, 255.0)
    t = _dev(x, gpu)
    for gloss in (None, torch.tensor(3.0, device=gpu)):
        L, n_c, _, _, _, g = _run(nconv_amd, t, 0.0, 255.0, False, gloss)
        d = t["depth"].detach().requires_grad_(True)
        L1, n1 = nconv_amd.photometric_loss(d, t["k"], t["tgt"], t["srcs"][0], t["ms"][0], t["mask"],
                                            return_valid_count=True)
        L1.backward(gloss)
        assert torch.equal(L, L1) and torch.equal(g, d.grad) and n_c.item() == n1.item() > 0


@pytest.mark.parametrize("C,with_mask", [(3, False), (1, True)])
def test_one_source_alpha_one_is_the_ssim_loss(nconv_amd, gpu, C, with_mask):
    """S = 1, no auto-mask, alpha = 1: L and g_depth are torch.equal to photometric_ssim_loss(alpha=1)'s."""
    x = MC.min_inputs(51 + C, 2, C, (45, 67), (47, 70), 1, True, with_mask, 255.0)
    t = _dev(x, gpu)
    for gloss in (None, torch.tensor(3.0, device=gpu)):
        L, n_c, _, _, _, g = _run(nconv_amd, t, 1.0, 255.0, False, gloss)
        d = t["depth"].detach().requires_grad_(True)
        L1, _, n_w = nconv_amd.photometric_ssim_loss(d, t["k"], t["tgt"], t["srcs"][0], t["ms"][0], t["mask"],
                                                     alpha=1.0, data_range=255.0, return_counts=True)
        L1.backward(gloss)
        assert torch.equal(L, L1) and torch.equal(g, d.grad) and n_c.item() == n_w.item() > 0


def _exact_setup(gpu, B=2, C=3, H=21, W=70, seed=7):
    g = torch.Generator().manual_seed(seed)
    tgt = (torch.rand(B, C, H, W, generator=g) * 255).to(gpu)
    k = torch.tensor([[64.0, 0, 30], [0, 64.0, 9], [0, 0, 1]], device=gpu)
    d = torch.full((B, 1, H, W), 4.0, device=gpu)
    return d, k, tgt


def _shift_pose(gpu, tx):
    """x = tx at depth 4 with fx = 64: u = j + 16 tx, v = i, exactly."""
    pose = torch.eye(4, device=gpu)
    pose[0, 3] = tx
    return pose


def test_sources_that_each_leave_the_frame(nconv_amd, gpu):
    """u = j + 32 for source 0 (columns above 37 leave it) and u = j - 32 for source 1 (columns below 32 leave
    it): every pixel with a winner outside the overlap takes the only source that sees it, n_c is the size of
    the union of the two window sets, and in the overlap a pixel won by source 0 next to a window won by source
    1 exists and its gradient is the rule's, which adds both sources' terms. A sum of two single-source losses
    has neither this n_c nor this L."""
    d, k, tgt = _exact_setup(gpu)
    B, C, H, W = tgt.shape
    g = torch.Generator().manual_seed(11)
    srcs = [(torch.rand(B, C, H, W, generator=g) * 255).to(gpu) for _ in range(2)]
    ms = [nconv_amd.warp_projection(k, _shift_pose(gpu, tx)) for tx in (2.0, -2.0)]
    x = {"depth": d[:, 0].cpu().numpy(), "k": k.cpu().numpy(), "tgt": tgt.cpu().numpy(), "mask": None,
         "srcs": [s.cpu().numpy() for s in srcs], "ms": [m.cpu().numpy() for m in ms], "data_range": 255.0}
    (L, n_c, n_m, winner, _, grad), rule = _check(nconv_amd, x, gpu, 0.85, False)
    w = winner.cpu().numpy()
    cols = np.arange(W)[None, None, :] + np.zeros_like(w, dtype=np.int64)
    has = w != MC.NONE
    assert n_c.item() == B * (H - 2) * (W - 2) and n_m.item() == 0  # the union: every interior pixel
    assert (w[has & (cols < 33)] == 0).all() and (w[has & (cols > 36)] == 1).all()
    assert not has[:, 0].any() and not has[:, :, 0].any() and has[:, 1:-1, 1:-1].all()
    won0, won1 = w == 0, w == 1
    near1 = np.zeros_like(won1)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            near1[:, 1:-1, 1:-1] |= won1[:, 1 + di:H - 1 + di, 1 + dj:W - 1 + dj]
    both = won0 & near1
    assert both.any() and (both & (cols >= 32) & (cols <= 36)).sum() == both.sum()  # next to the overlap's 33 .. 36
    assert np.array_equal(grad[:, 0].cpu().numpy()[both], rule["g_depth"][both])
    singles = [nconv_amd.photometric_ssim_loss(d, k, tgt, s, m, return_counts=True) for s, m in zip(srcs, ms)]
    assert all(nw.item() < n_c.item() for _, _, nw in singles)
    assert L.item() != (singles[0][0] + singles[1][0]).item()


def test_automask_masks_a_standing_camera(nconv_amd, gpu):
    """Sources equal to the target under the identity pose: every pixel with a winner is masked (the identity
    wins the tie 0 <= 0), L == 0, g_depth is all zero, n_m == n_c."""
    d, k, tgt = _exact_setup(gpu)
    B, C, H, W = tgt.shape
    m = nconv_amd.warp_projection(k, torch.eye(4, device=gpu))
    for alpha, count in ((0.85, B * (H - 2) * (W - 2)), (0.0, B * H * W)):
        dd = d.clone().requires_grad_(True)
        L, n_c, n_m, winner = nconv_amd.min_reprojection_loss(dd, k, tgt, [tgt.clone(), tgt.clone()], [m, m],
                                                              alpha=alpha, return_counts=True, return_winner=True)
        L.backward()
        assert L.item() == 0.0 and n_c.item() == n_m.item() == count
        assert not dd.grad.any() and set(winner.unique().tolist()) <= {MC.MASKED, MC.NONE}
        L, n_c, n_m = nconv_amd.min_reprojection_loss(d, k, tgt, [tgt.clone(), tgt.clone()], [m, m], alpha=alpha,
                                                      automask=False, return_counts=True)
        assert L.item() == 0.0 and n_c.item() == count and n_m.item() == 0


def test_automask_keeps_a_source_that_warps_onto_the_target(nconv_amd, gpu):
    """src is tgt moved by 32 columns and the pose moves it back (u = j + 32 exactly): warped == tgt where it is
    valid, so best == 0, while the unwarped source differs strongly: nothing is masked."""
    d, k, tgt = _exact_setup(gpu)
    B, C, H, W = tgt.shape
    g = torch.Generator().manual_seed(5)
    src = (torch.rand(B, C, H, W, generator=g) * 255).to(gpu)
    src[..., 32:] = tgt[..., :W - 32]
    m = nconv_amd.warp_projection(k, _shift_pose(gpu, 2.0))
    L, n_c, n_m, winner = nconv_amd.min_reprojection_loss(d, k, tgt, [src], [m], return_counts=True,
                                                          return_winner=True)
    assert L.item() == 0.0 and n_m.item() == 0 and n_c.item() == B * (H - 2) * (W - 32 - 2)
    assert set(winner.unique().tolist()) == {0, MC.NONE}


def test_a_nan_in_a_source_reaches_the_loss(nconv_amd, gpu):
    """One NaN in a source: its windows' errors are NaN, a NaN replaces a number and is not masked, so L is NaN
    as torch.min and torch.sum propagate it; nothing faults, and the winner plane is the rule's."""
    x = MC.min_inputs(13, 2, 3, (45, 67), None, 2, True, False, 255.0)
    x["srcs"][1][1, 2, 20, 30] = np.nan
    t = _dev(x, gpu)
    L, _, _, winner, _, g = _run(nconv_amd, t, 0.85, 255.0, True)
    rule = MC.min_rule_fp32(*MC.call_args(x), alpha=0.85, data_range=255.0, automask=True)
    assert np.isnan(L.item()) and np.isnan(rule["L"])
    assert np.array_equal(winner.cpu().numpy(), rule["winner"])
    assert np.array_equal(g[:, 0].cpu().numpy(), rule["g_depth"], equal_nan=True)


def test_source_order_permutes_the_winner_plane(nconv_amd, gpu):
    """Permuting the sources gives the same L bits, the same counts and the permuted winner plane (the inputs
    are random frames: no two errors of a pixel are equal, which the rule's E confirms)."""
    x = MC.min_inputs(61, 2, 3, (45, 67), None, 3, True, True, 255.0)
    rule = MC.min_rule_fp32(*MC.call_args(x), alpha=0.85, data_range=255.0, automask=True)
    E = np.where(rule["comparable"], rule["E"], np.inf)
    srt = np.sort(E, axis=0)
    assert not ((srt[1:] == srt[:-1]) & np.isfinite(srt[1:])).any() and not (rule["Imin"] == rule["best"])[rule["has"]].any()
    t = _dev(x, gpu)
    L, n_c, n_m, winner, error, _ = _run(nconv_amd, t, 0.85, 255.0, True)
    perm = [2, 0, 1]
    p = dict(t)
    p["srcs"], p["ms"] = [t["srcs"][i] for i in perm], [t["ms"][i] for i in perm]
    Lp, n_cp, n_mp, winner_p, error_p, _ = _run(nconv_amd, p, 0.85, 255.0, True)
    assert torch.equal(L, Lp) and n_c.item() == n_cp.item() and n_m.item() == n_mp.item()
    assert torch.equal(error, error_p)
    back = torch.arange(256, dtype=torch.uint8, device=gpu)
    back[:3] = torch.tensor(perm, dtype=torch.uint8, device=gpu)  # winner_p's index s is source perm[s]
    assert torch.equal(back[winner_p.long()], winner)


def test_cropped_strided_views(nconv_amd, gpu):
    """depth cropped out of a larger buffer at an odd offset (DNET's cropped output; 1e30 outside), tgt, the
    sources and the mask out of others with other strides: the results are the contiguous ones."""
    x = MC.min_inputs(21, 2, 3, (45, 67), None, 2, True, True, 255.0)
    t = _dev(x, gpu)
    want = _run(nconv_amd, t, 0.85, 255.0, True)
    big_d = torch.full((2, 1, 49, 71), 1e30, device=gpu)
    big_s = [torch.full((2, 4, 50, 80), 1e30, device=gpu), torch.full((3, 3, 46, 70), 1e30, device=gpu)]
    big_t = torch.full((3, 3, 47, 69), 1e30, device=gpu)
    big_m = torch.ones((2, 1, 46, 75), dtype=torch.uint8, device=gpu)
    v = dict(t)
    v["depth"], v["srcs"] = big_d[:, :, 3:48, 1:68], [big_s[0][:, 1:, 2:47, 5:72], big_s[1][:2, :, 1:, 3:]]
    v["tgt"], v["mask"] = big_t[1:, :, 1:46, 2:69], big_m[:, :, 1:, 3:70]
    for key in ("depth", "tgt", "mask"):
        v[key].copy_(t[key])
        assert not v[key].is_contiguous()
    for a, b in zip(v["srcs"], t["srcs"]):
        a.copy_(b)
        assert not a.is_contiguous()
    got = _run(nconv_amd, v, 0.85, 255.0, True)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[5].is_contiguous()


def test_module_is_the_function(nconv_amd, gpu):
    x = MC.min_inputs(41, 2, 3, (17, 65), None, 2, True, False, 255.0)
    t = _dev(x, gpu)
    L, _, _, _, _, g = _run(nconv_amd, t, 0.85, 255.0, True)
    d = t["depth"].detach().requires_grad_(True)
    Lm = nconv_amd.MinReprojectionLoss()(d, t["k"], t["tgt"], t["srcs"], t["ms"])
    Lm.backward()
    assert torch.equal(Lm.detach(), L) and torch.equal(d.grad, g)


def test_min_reprojector_keeps_its_buffers_and_replays(nconv_amd, gpu):
    """MinReprojector: no allocation after construction, so the loss with its backward is captured and replayed;
    the replay is bitwise the eager call, also after the matrices are refilled in place."""
    x = MC.min_inputs(43, 2, 3, (45, 67), None, 2, True, False, 255.0)
    t = _dev(x, gpu)
    mr = nconv_amd.MinReprojector((45, 67), S=2, B=2, C=3, device=gpu)
    d = t["depth"].clone().requires_grad_(True)
    ms = [m.clone() for m in t["ms"]]
    seed = torch.ones((), device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mr(d, t["k"], t["tgt"], t["srcs"], ms).backward(seed)
    torch.cuda.current_stream().wait_stream(side)
    d.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L, n_c, n_m, winner, error = mr(d, t["k"], t["tgt"], t["srcs"], ms, return_counts=True, return_winner=True,
                                        return_error=True)
        L.backward(seed)
    assert L.data_ptr() == mr._out["loss"].data_ptr() and winner.data_ptr() == mr._out["winner"].data_ptr()
    assert error.data_ptr() == mr._out["error"].data_ptr()
    seen = []
    for scale in (1.0, 0.5):
        for m, m0 in zip(ms, t["ms"]):
            m.copy_(m0)
            m[:, :, 3] *= scale  # another translation
        graph.replay()
        torch.cuda.synchronize()
        e = dict(t)
        e["ms"] = ms
        Le, n_ce, n_me, winner_e, error_e, ge = _run(nconv_amd, e, 0.85, 255.0, True)
        assert torch.equal(L, Le) and (n_c.item(), n_m.item()) == (n_ce.item(), n_me.item())
        assert torch.equal(winner, winner_e) and torch.equal(error, error_e) and torch.equal(d.grad, ge)
        assert torch.equal(mr._out["g_depth"], ge)
        seen.append((L.item(), d.grad.clone()))
    assert seen[0][0] != seen[1][0] and not torch.equal(seen[0][1], seen[1][1])


def test_graphed_step_with_min_reprojection_and_smoothness(nconv_amd, gpu):
    """A GraphedTrainStep on a small DNET (2 x 64 x 96) whose loss is calculate_loss + w min_reprojection (two
    sources, auto-masking) + w2 smooth, replayed twice: the parameters and the loss are the eager steps' bit
    for bit."""
    g = torch.Generator().manual_seed(6)
    S = sparse_depth(g, 2, 64, 96, density=0.1).to(gpu)
    gt = ((torch.rand(2, 1, 64, 96, generator=g) * 80) * (torch.rand(2, 1, 64, 96, generator=g) < 0.3)).to(gpu)
    rgb = (torch.rand(2, 3, 64, 96, generator=g) * 255).to(gpu)
    prev = (torch.rand(2, 3, 64, 96, generator=g) * 255).to(gpu)
    nxt = (torch.rand(2, 3, 64, 96, generator=g) * 255).to(gpu)
    k = torch.tensor(WC.intrinsics(64, 96, 80.0), dtype=torch.float32, device=gpu)
    pose0 = torch.tensor(np.stack([WC.rigid(0.004, -0.006, 0.003, (0.12, -0.04, 0.45))] * 2), device=gpu)
    pose1 = torch.tensor(np.stack([WC.rigid(-0.003, 0.005, -0.002, (-0.1, 0.03, -0.4))] * 2), device=gpu)
    m0, m1 = nconv_amd.warp_projection(k, pose0), nconv_amd.warp_projection(k, pose1)
    w, w2 = 0.01, 0.1

    def setup():
        torch.manual_seed(0)
        net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu)
        net.train()
        opt = nconv_amd.train.get_optimizer(net, "adam", 1e-2, 1e-7, capturable=True)
        photo = nconv_amd.MinReprojectionLoss(z_min=1e-3)

        def fn(model, s, t, a, b, c, ma, mb):
            pred = model(s)
            return (nconv_amd.train.calculate_loss(pred, t, True) + w * photo(pred, k, a, (b, c), (ma, mb))
                    + w2 * nconv_amd.smoothness_loss(pred))
        return net, opt, fn

    net_e, opt_e, fn_e = setup()
    net_g, opt_g, fn_g = setup()
    step = nconv_amd.train.GraphedTrainStep(net_g, opt_g, fn_g, (S, gt, rgb, prev, nxt, m0, m1))
    for _ in range(2):
        opt_e.zero_grad(set_to_none=True)
        loss = fn_e(net_e, S, gt, rgb, prev, nxt, m0, m1)
        loss.backward()
        opt_e.step()
        lg = step(S, gt, rgb, prev, nxt, m0, m1)
        torch.cuda.synchronize()
        assert np.isfinite(loss.item()) and loss.item() == lg.item()
        for (n, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), n
