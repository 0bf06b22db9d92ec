"""The cross-view depth consistency check with fusion and the geometry-consistency loss
(consistency.depth_consistency / geometry_consistency_loss: nconv_depth_consistency,
nconv_geo_consistency_loss_*) on the GPU: bit for bit against the fp32 rules restated in numpy
(consistency_cases), the analytic wall-and-rectangle scene, corner cases that need no reference, strided views,
determinism, the loss's summation tree, refusals and capture."""
import numpy as np
import pytest
import torch

import consistency_cases as CC
import reduce_tree as RT
import warp_cases as WC
from test_gpu_dnet import sparse_depth

pytestmark = pytest.mark.gpu


def _dev(x, gpu):
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    t = {"depth": up(x["depth"])[:, None], "k": up(x["k"]), "src_depths": [up(s)[:, None] for s in x["src_depths"]],
         "k_srcs": [up(a) for a in x["k_srcs"]], "ms": [up(a) for a in x["ms"]],
         "m_backs": [up(a) for a in x["m_backs"]], "poses": [up(a) for a in x["poses"]],
         "mask": None if x["mask"] is None else up(x["mask"])[:, None]}
    return t


def _fuser(nconv_amd, gpu, t, **kw):
    B, _, H, W = t["depth"].shape
    return nconv_amd.DepthFuser((H, W), tuple(t["src_depths"][0].shape[-2:]), S=len(t["src_depths"]), B=B, device=gpu,
                                **kw)


def _check_run(nconv_amd, gpu, t, **kw):
    """(fused, count, views, reproj, reldiff) through DepthFuser, i.e. with exactly the matrices of the scene."""
    out = _fuser(nconv_amd, gpu, t, **kw)(t["depth"], t["k"], t["src_depths"], t["k_srcs"], t["ms"], t["m_backs"],
                                          t["mask"], return_views=True, return_error=True)
    torch.cuda.synchronize()
    return tuple(o.clone() for o in out)


def _loss_run(nconv_amd, t, s, gloss=None):
    d = t["depth"].detach().clone().requires_grad_(True)
    L, diff, n_g = nconv_amd.geometry_consistency_loss(d, t["k"], t["src_depths"][s], None, None, t["mask"],
                                                       return_diff=True, return_count=True, m=t["ms"][s])
    L.backward(gloss)
    torch.cuda.synchronize()
    return L.detach().clone(), n_g.clone(), diff.clone(), d.grad


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


CASES = [((17, 65), (19, 70)), ((45, 67), None), ((64, 96), None)]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense_src", "sparse_src"])
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("per_image", [True, False], ids=["per_image", "shared"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("size,src_size", CASES, ids=["17x65_from_19x70", "45x67", "64x96"])
def test_check_and_loss_match_rule(nconv_amd, gpu, size, src_size, S, per_image, with_mask, sparse):
    x = CC.scene(1000 * size[0] + 10 * S + 2 * per_image + with_mask, 2, size, src_size, S, per_image, with_mask, sparse)
    t = _dev(x, gpu)
    got = _check_run(nconv_amd, gpu, t)
    rule = CC.rule_fp32(x["depth"], x["k"], x["src_depths"], x["k_srcs"], x["ms"], x["m_backs"], mask=x["mask"])
    fused, count, views, reproj, reldiff = got
    _same(fused[:, 0], rule["fused"], "fused")
    _same(count, rule["count"], "count")
    _same(views, rule["views"], "views")
    _same(reproj, rule["reproj"], "reproj")
    _same(reldiff, rule["reldiff"], "reldiff")
    n_cons = int(rule["cons"].sum())
    print(f"consistent {n_cons} of {rule['cons'].size}, fused > 0 on {(rule['fused'] > 0).mean():.3f}")
    assert 0 < n_cons < rule["cons"].size  # both decisions took part
    gloss = torch.tensor(3.0, device=gpu)
    for s in range(S):
        L, n_g, diff, g = _loss_run(nconv_amd, t, s, gloss)
        lr = CC.loss_rule_fp32(x["depth"], x["k"], x["src_depths"][s], x["ms"][s], x["mask"], gloss=3.0)
        assert n_g.dtype == torch.int32 and n_g.item() == lr["n_g"] and 0 < lr["n_g"] < diff.numel()
        _same(diff[:, 0], lr["terms"], "diff")
        assert RT.same_bits(L.item(), lr["loss"]), (L.item(), lr["loss"])
        _same(g[:, 0], lr["g_depth"], "g_depth")


def test_analytic_wall_and_rectangle(nconv_amd, gpu):
    """A wall at 8 m with a rectangle at 2 m in front, the source camera 0.5 m to the side, both depth maps rendered
    by exact ray casting: on every pixel at least 2 px from a silhouette edge in either view, wall pixels the
    source sees are consistent, wall pixels hidden behind the rectangle in the source and pixels that leave the
    source frame are not; fused is 0 where count < min_views and finite and positive elsewhere."""
    x = CC.analytic_scene()
    t = _dev(x, gpu)
    fused, count, views, reproj, reldiff = _check_run(nconv_amd, gpu, t)
    count, expect, kind = count.cpu().numpy(), x["expect"], x["kind"]
    for name in ("seen", "hidden", "left", "rect"):
        sel = kind == name
        print(name, int(sel.sum()), "pixels, consistent", int(count[sel].sum()))
        assert sel.sum() > 20, name
        assert (count[sel] == (1 if name in ("seen", "rect") else 0)).all(), name
    assert (count[expect == 1] == 1).all() and (count[expect == 0] == 0).all()
    assert np.array_equal(views.cpu().numpy(), count)  # one source: bit 0
    f = fused[:, 0].cpu().numpy()
    assert (f[count < 1] == 0).all() and np.isfinite(f).all() and (f[count >= 1] > 0).all()
    assert np.abs(f[kind == "seen"] - 8.0).max() < 1e-4 and np.abs(f[kind == "rect"] - 2.0).max() < 1e-4
    # the hidden wall pixels read the rectangle's 2 m where they expect 8 m: the loss's map says so
    _, _, diff, _ = _loss_run(nconv_amd, t, 0)
    d = diff[:, 0].cpu().numpy()
    assert np.abs(d[kind == "hidden"] - 0.6).max() < 1e-5 and d[kind == "seen"].max() < 1e-5


def test_identity_pose_source_equal_to_target(nconv_amd, gpu):
    """The source is the target itself under the identity pose (fx = fy = 64, integer cx, cy, depths that are
    multiples of 1/4: u = j, v = i exactly): count == S on every valid pixel, fused == z."""
    g = torch.Generator().manual_seed(3)
    z = (torch.randint(8, 80, (2, 1, 21, 70), generator=g).float() / 4).to(gpu)
    z[:, :, 5, 7] = 0.0
    z[:, :, 6, 9] = float("nan")
    k = torch.tensor([[64.0, 0, 30], [0, 64.0, 9], [0, 0, 1]], device=gpu)
    eye = torch.tensor(WC.rigid(), device=gpu)
    for S in (1, 3):
        fused, count = nconv_amd.depth_consistency(z, k, [z] * S, [k] * S, [eye] * S)
        valid = torch.isfinite(z[:, 0]) & (z[:, 0] > 0)
        # a pixel next to the hole or the NaN in the row above / to the left still has its own four taps: u = j
        # makes j1 = j + 1 a tap of weight 0, which must be a depth all the same
        tap_ok = valid.clone()
        tap_ok[:, :, :-1] &= valid[:, :, 1:]
        tap_ok[:, :-1, :] &= valid[:, 1:, :]
        tap_ok[:, :-1, :-1] &= valid[:, 1:, 1:]
        assert (count[tap_ok] == S).all() and (count[~tap_ok] == 0).all()
        assert torch.equal(fused[:, 0][tap_ok], z[:, 0][tap_ok]) and (fused[:, 0][~tap_ok] == 0).all()


def test_min_views_zero_keeps_z(nconv_amd, gpu):
    x = CC.scene(11, 2, (17, 65), (19, 70), S=2)
    t = _dev(x, gpu)
    for src in t["src_depths"]:
        src += 3.0  # no source agrees within 1 %
    fused, count, *_ = _check_run(nconv_amd, gpu, t, min_views=0)
    z = t["depth"][:, 0]
    valid = torch.isfinite(z) & (z > 1e-3)
    assert (count == 0).all() and torch.equal(fused[:, 0][valid], z[valid]) and (fused[:, 0][~valid] == 0).all()
    fused1, *_ = _check_run(nconv_amd, gpu, t, min_views=1)
    assert (fused1 == 0).all()


def test_nan_depth_or_tap_is_never_consistent(nconv_amd, gpu):
    x = CC.scene(12, 2, (17, 65), None, S=1, holes=False)
    t = _dev(x, gpu)
    base = _check_run(nconv_amd, gpu, t, rel_tol=0.05)
    assert base[1].float().mean() > 0.5  # most pixels agree at 5 %
    t["src_depths"][0][:] = float("nan")
    fused, count, views, reproj, reldiff = _check_run(nconv_amd, gpu, t, rel_tol=0.05)
    assert (count == 0).all() and (views == 0).all() and (fused == 0).all()
    assert torch.isinf(reproj).all() and torch.isinf(reldiff).all()
    L, n_g, diff, g = _loss_run(nconv_amd, t, 0)
    assert n_g.item() == 0 and L.item() == 0.0 and (diff == 0).all() and (g == 0).all()
    t = _dev(x, gpu)
    t["depth"][:] = float("nan")
    fused, count, *_ = _check_run(nconv_amd, gpu, t, rel_tol=0.05)
    assert (count == 0).all() and (fused == 0).all()


def test_one_by_one(nconv_amd, gpu):
    """A 1 x 1 target from a 1 x 1 source under the identity: image 0 agrees, image 1 has no depth."""
    k = torch.tensor([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]], device=gpu)
    z = torch.tensor([4.0, 0.0], device=gpu).reshape(2, 1, 1, 1)
    src = torch.tensor([4.0, 4.0], device=gpu).reshape(2, 1, 1, 1)
    eye = torch.tensor(WC.rigid(), device=gpu)
    fused, count, views = nconv_amd.depth_consistency(z, k, [src], [k], [eye], return_views=True)
    assert fused.flatten().tolist() == [4.0, 0.0] and count.flatten().tolist() == [1, 0]
    assert views.flatten().tolist() == [1, 0]
    d = z.clone().requires_grad_(True)
    L, n_g = nconv_amd.geometry_consistency_loss(d, k, src * 3, k, eye, return_count=True)
    L.backward()
    assert n_g.item() == 1 and L.item() == 0.5 and d.grad.flatten()[1].item() == 0.0  # |4 - 12| / 16


def test_cropped_strided_views_and_determinism(nconv_amd, gpu):
    """depth cropped out of a larger buffer at an odd offset (DNET's output is such a view), the sources and the
    mask out of others: the results are the contiguous ones; and two runs are torch.equal."""
    x = CC.scene(21, 2, (45, 67), (47, 70), S=2, with_mask=True, sparse=True)
    t = _dev(x, gpu)
    want = _check_run(nconv_amd, gpu, t) + _loss_run(nconv_amd, t, 1)
    again = _check_run(nconv_amd, gpu, t) + _loss_run(nconv_amd, t, 1)
    assert all(torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and
               torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(want, again))
    v = dict(t)
    big_d = torch.full((2, 1, 49, 71), 1e30, device=gpu)
    big_m = torch.ones((2, 1, 46, 75), dtype=torch.uint8, device=gpu)
    v["depth"], v["mask"] = big_d[:, :, 3:48, 1:68], big_m[:, :, 1:, 3:70]
    v["src_depths"] = [torch.full((2, 2, 50, 80), 1e30, device=gpu)[:, 1:, 2:49, 5:75] for _ in range(2)]
    v["depth"].copy_(t["depth"]), v["mask"].copy_(t["mask"])
    for a, b in zip(v["src_depths"], t["src_depths"]):
        a.copy_(b)
        assert not a.is_contiguous()
    got = _check_run(nconv_amd, gpu, v) + _loss_run(nconv_amd, v, 1)
    for a, b in zip(got, want):
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and (torch.isnan(a) == torch.isnan(b)).all()
    # the package's own entry with poses: DNET's cropped output as the depth
    net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu).eval()
    with torch.no_grad():
        pred = net(sparse_depth(torch.Generator().manual_seed(2), 2, 64, 96, density=0.2).to(gpu))
    k = torch.tensor(WC.intrinsics(*pred.shape[-2:], 80.0), dtype=torch.float32, device=gpu)
    eye = torch.tensor(WC.rigid(), device=gpu)
    fused, count = nconv_amd.depth_consistency(pred[:, :1], k, [pred[:, :1]], [k], [eye], px_tol=1.0, rel_tol=0.01)
    assert fused.shape == pred[:, :1].shape and count.dtype == torch.uint8 and count.max().item() <= 1


def test_loss_sum_is_the_stated_tree(nconv_amd, gpu):
    """L bit for bit from the rule's fp32 terms summed in the order csrc/wave_ops.h states (reduce_tree.py,
    view_warp.hip's thread map) at (3, 33, 70): partial tiles in both directions, six tiles per image."""
    B, H, Wd = 3, 33, 70
    x = CC.scene(1000 * B + Wd, B, (H, Wd), None, S=1)
    t = _dev(x, gpu)
    L, n_g, diff, _ = _loss_run(nconv_amd, t, 0)
    lr = CC.loss_rule_fp32(x["depth"], x["k"], x["src_depths"][0], x["ms"][0])
    want = RT.loss(diff[:, 0].cpu().numpy(), float(max(n_g.item(), 1)), RT.ROWS)
    print(f"L {L.item():.9g} tree {want:.9g} n_g {n_g.item()}")
    assert n_g.item() == lr["n_g"] and 0 < lr["n_g"] < B * H * Wd
    assert RT.same_bits(L.item(), want) and RT.same_bits(L.item(), lr["loss"])


def test_invalid_pixels_have_no_value_count_or_gradient(nconv_amd, gpu):
    """c <= 0, a NaN, infinite, zero or negative depth, a depth outside [z_min, z_max] and a mask of 0: fused 0,
    count 0, not in n_g, diff 0, g_depth 0."""
    B, H, Wd = 2, 21, 70
    d = torch.full((B, 1, H, Wd), 8.0, device=gpu)
    k = torch.tensor([[64.0, 0, 30], [0, 64.0, 9], [0, 0, 1]], device=gpu)
    pose = torch.tensor(WC.rigid(t=(0.0, 0.0, -1.0)), device=gpu)  # c = z - 1
    for row, val in enumerate((0.5, 1.0, float("nan"), float("inf"), 0.0, -8.0, 0.125, 100.0)):
        d[:, :, row] = val
    mask = torch.ones(d.shape, dtype=torch.bool, device=gpu)
    mask[:, :, 8] = False
    src = torch.full((B, 1, H, Wd), 7.0, device=gpu)
    fuser = nconv_amd.DepthFuser((H, Wd), S=1, B=B, device=gpu, z_min=0.25, z_max=50.0, rel_tol=0.05)
    m = nconv_amd.warp_projection(k, pose)
    mb = nconv_amd.warp_projection(k, nconv_amd.inverse_pose(pose))
    fused, count = fuser(d, k, [src], [k], [m], [mb], mask)
    assert (count[:, :9] == 0).all() and (fused[:, :, :9] == 0).all() and (count[:, 9:] == 1).any()
    d.requires_grad_(True)
    geo = nconv_amd.GeometryConsistency((H, Wd), B=B, device=gpu, z_min=0.25, z_max=50.0)
    L, diff, n_g = geo(d, k, src * 1.5, m, mask, return_diff=True, return_count=True)
    L.backward()
    assert (diff[:, :, :9] == 0).all() and (d.grad[:, :, :9] == 0).all() and torch.isfinite(d.grad).all()
    assert n_g.item() == int((diff != 0).sum().item()) > 0 and torch.isfinite(L) and (d.grad[:, :, 9:] != 0).any()


def test_refusals(nconv_amd, gpu):
    x = CC.scene(5, 2, (8, 16), None, S=1)
    t = _dev(x, gpu)
    args = (t["depth"], t["k"], t["src_depths"][0], None, None)
    with pytest.raises(ValueError, match="scatter"):
        nconv_amd.geometry_consistency_loss(t["depth"], t["k"], t["src_depths"][0].clone().requires_grad_(True), None,
                                            None, m=t["ms"][0])
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.geometry_consistency_loss(t["depth"], t["k"], t["src_depths"][0].cpu(), None, None, m=t["ms"][0])
    with pytest.raises(ValueError, match="min_views"):
        nconv_amd.depth_consistency(t["depth"], t["k"], t["src_depths"], t["k_srcs"], t["poses"], min_views=2)
    with pytest.raises(ValueError, match="px_tol"):
        nconv_amd.depth_consistency(t["depth"], t["k"], t["src_depths"], t["k_srcs"], t["poses"], px_tol=-1.0)
    with pytest.raises(ValueError, match="one per source"):
        nconv_amd.depth_consistency(t["depth"], t["k"], t["src_depths"], t["k_srcs"] * 2, t["poses"])
    with pytest.raises(ValueError, match="DepthFuser was built for"):
        _fuser(nconv_amd, gpu, t)(t["depth"][:1], t["k"], [t["src_depths"][0][:1]], t["k_srcs"], t["ms"], t["m_backs"])
    with pytest.raises(ValueError, match="GeometryConsistency was built for"):
        nconv_amd.GeometryConsistency((8, 16), B=1, device=gpu)(*args[:3], t["ms"][0])


def test_fuser_and_loss_capture_and_replay(nconv_amd, gpu):
    """DepthFuser and GeometryConsistency: no allocation after construction, so the check and the loss with its
    backward are captured and replayed; refilling m and m_back in place changes the replay's results to the eager
    ones."""
    x = CC.scene(41, 2, (17, 65), (19, 70), S=2)
    t = _dev(x, gpu)
    fuser = _fuser(nconv_amd, gpu, t)
    geo = nconv_amd.GeometryConsistency((17, 65), (19, 70), B=2, device=gpu)
    d = t["depth"].clone().requires_grad_(True)
    ms, mbs = [m.clone() for m in t["ms"]], [m.clone() for m in t["m_backs"]]
    seed = torch.ones((), device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fuser(d, t["k"], t["src_depths"], t["k_srcs"], ms, mbs, return_views=True, return_error=True)
        geo(d, t["k"], t["src_depths"][0], ms[0]).backward(seed)
    torch.cuda.current_stream().wait_stream(side)
    d.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fuser(d, t["k"], t["src_depths"], t["k_srcs"], ms, mbs, return_views=True, return_error=True)
        L = geo(d, t["k"], t["src_depths"][0], ms[0])
        L.backward(seed)
    assert outs[0].data_ptr() == fuser._out["fused"].data_ptr() and L.data_ptr() == geo._out["loss"].data_ptr()
    seen = []
    for shift in (0.0, 0.05):
        poses = [p.copy() for p in x["poses"]]
        for p in poses:
            p[:, 2, 3] += shift  # another translation along z
        for s in range(2):
            ms[s].copy_(nconv_amd.warp_projection(t["k_srcs"][s], torch.tensor(poses[s], device=gpu)))
            mbs[s].copy_(nconv_amd.warp_projection(t["k"], nconv_amd.inverse_pose(torch.tensor(poses[s], device=gpu))))
        graph.replay()
        torch.cuda.synchronize()
        rule = CC.rule_fp32(x["depth"], x["k"], x["src_depths"], x["k_srcs"], [m.cpu().numpy() for m in ms],
                            [m.cpu().numpy() for m in mbs])
        lr = CC.loss_rule_fp32(x["depth"], x["k"], x["src_depths"][0], ms[0].cpu().numpy())
        _same(outs[0][:, 0], rule["fused"], "fused")
        _same(outs[1], rule["count"], "count")
        _same(outs[2], rule["views"], "views")
        _same(outs[3], rule["reproj"], "reproj")
        _same(d.grad[:, 0], lr["g_depth"], "g_depth")
        eager = nconv_amd.depth_consistency(t["depth"], t["k"], t["src_depths"], t["k_srcs"],
                                            [torch.tensor(p, device=gpu) for p in poses])
        assert torch.equal(eager[0], outs[0]) and torch.equal(eager[1], outs[1])
        assert L.item() == nconv_amd.geometry_consistency_loss(t["depth"], t["k"], t["src_depths"][0], None, None,
                                                               m=ms[0]).item()
        seen.append((L.item(), outs[1].clone(), d.grad.clone()))
    assert seen[0][0] != seen[1][0] and not torch.equal(seen[0][1], seen[1][1])
    assert not torch.equal(seen[0][2], seen[1][2])


def test_graphed_step_with_geometry_term(nconv_amd, gpu):
    """A GraphedTrainStep on a small DNET (2 x 64 x 96) whose loss is calculate_loss + w * geo(pred, k, prev, m=m),
    replayed three times: the parameters and the loss are the eager steps' bit for bit, and m changed in place
    between replays changes the step (test_gpu_warp.py's construction with this term)."""
    g = torch.Generator().manual_seed(6)
    S = sparse_depth(g, 2, 64, 96, density=0.1).to(gpu)
    gt = ((torch.rand(2, 1, 64, 96, generator=g) * 80) * (torch.rand(2, 1, 64, 96, generator=g) < 0.3)).to(gpu)
    prev = (torch.rand(2, 1, 64, 96, generator=g) * 40 + 5).to(gpu)
    k = torch.tensor(WC.intrinsics(64, 96, 80.0), dtype=torch.float32, device=gpu)
    pose = torch.tensor(np.stack([WC.rigid(0.004, -0.006, 0.003, (0.12, -0.04, 0.45))] * 2), device=gpu)
    m0 = nconv_amd.warp_projection(k, pose)
    w = 0.1

    def setup():
        torch.manual_seed(0)
        net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu)
        net.train()
        opt = nconv_amd.train.get_optimizer(net, "adam", 1e-2, 1e-7, capturable=True)
        geo = nconv_amd.GeometryConsistencyLoss()

        def fn(model, s, t, p, m):
            pred = model(s)
            return nconv_amd.train.calculate_loss(pred, t, True) + w * geo(pred[:, :1], k, p, m=m)
        return net, opt, fn

    net_e, opt_e, fn_e = setup()
    net_g, opt_g, fn_g = setup()
    net_r, opt_r, fn_r = setup()  # the control: three eager steps that keep m0
    step = nconv_amd.train.GraphedTrainStep(net_g, opt_g, fn_g, (S, gt, prev, m0))

    def eager(net, opt, fn, mm):
        opt.zero_grad(set_to_none=True)
        loss = fn(net, S, gt, prev, mm)
        loss.backward()
        opt.step()
        return loss.item()

    def both(mm):
        le = eager(net_e, opt_e, fn_e, mm)
        lg = step(S, gt, prev, mm)
        torch.cuda.synchronize()
        assert le == lg.item()
        for (n, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
            assert torch.equal(a, b), n
        return le

    assert both(m0) == eager(net_r, opt_r, fn_r, m0)
    assert both(m0) == eager(net_r, opt_r, fn_r, m0)
    m1 = m0.clone()
    m1[:, :, 3] *= 0.25
    step.static_inputs[3].copy_(m1)  # in place, in the step's own buffer
    l3, l3_kept = both(step.static_inputs[3]), eager(net_r, opt_r, fn_r, m0)
    assert np.isfinite(l3) and l3 != l3_kept
    assert any(not torch.equal(a, b) for a, b in zip(net_g.state_dict().values(), net_r.state_dict().values()))
