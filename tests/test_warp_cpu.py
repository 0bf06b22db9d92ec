"""The view warp and the photometric loss without a GPU: the fp32 rule of include/nconv.h
(warp_cases.rule_fp32, what the kernels reproduce bit for bit) against the float64 torch composition
(meshgrid, matrix product, F.grid_sample, masked mean) and its autograd gradient of the depth, inside
kappa x the derived majorant; the Python argument checks; and the host-side argument checks of
nconv_view_warp_* / nconv_photo_loss_* from a plain C program."""
import numpy as np
import pytest
import torch

import host_harness
import warp_cases as WC

CASES = [c[0] for c in WC.CPU_CASES]


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def budgets():
    return {name: WC.case_budget(name) for name in CASES}


def test_kappa_json_is_complete_and_current(budgets):
    """A kappa_ref and kappa = 4 kappa_ref for every case and output; recomputed, the file's figures."""
    K = WC.load_kappa()
    assert set(K) == set(CASES)
    for name in CASES:
        assert set(K[name]) == set(WC.OUTPUTS)
        x, args, ref, keep, omit, A = budgets[name]
        got = WC.ratios(WC.composition(*args, dtype=torch.float32), ref, keep, A)
        for key in WC.OUTPUTS:
            assert K[name][key]["kappa"] == pytest.approx(4 * K[name][key]["kappa_ref"], rel=1e-3)
            assert got[key] == pytest.approx(K[name][key]["kappa_ref"], rel=2e-2), (name, key)


@pytest.mark.parametrize("name", CASES)
def test_fp32_rule_matches_float64_composition(budgets, name):
    """warped, the gradient of the depth through view_warp (a random g_warped) and through the
    photometric loss: |rule - float64| <= kappa A per compared element. The compared pixels are the valid
    ones away from the gradient's discontinuities; at most 2 % are left out; the rule and the reference
    agree on which pixels are valid (so on n_v) and are both exactly 0 on the others."""
    x, args, ref, keep, omit, A = budgets[name]
    rule = WC.rule_fp32(*args)
    kappa = WC.kappa_for(WC.load_kappa())
    assert all(share <= 0.02 for share in omit.values()), omit
    assert np.array_equal(rule["valid"], ref["valid"]) and rule["n_v"] == ref["n_v"] > 0
    invalid = ~ref["valid"]
    assert invalid.any()
    for key in WC.OUTPUTS:
        err = np.abs(rule[key].astype(np.float64) - ref[key])
        worst = (err[keep[key]] / (kappa[key] * A[key][keep[key]] + 1e-300)).max()
        print(f"{name} {key}: err / (kappa A) max {worst:.3g}, kappa {kappa[key]:.4g}, omitted {omit[key]:.4f}")
        assert worst <= 1.0, (name, key, worst)
        off = np.broadcast_to(invalid[:, None], err.shape) if err.ndim == 4 else invalid
        assert (rule[key][off] == 0).all() and (ref[key][off] == 0).all()
    # the value is continuous across the integers: the loss over ALL valid pixels is inside the budget
    L32 = rule["terms"].astype(np.float64).sum() / float(rule["den"])
    C = x["src"].shape[1]
    bound = kappa["warped"] * A["warped"].sum() / (C * ref["n_v"]) + 4 * WC.U * abs(ref["loss"])
    assert abs(L32 - ref["loss"]) <= bound


def test_rule_exact_constructions():
    """fx = fy = 64, integer cx, cy, depth 4 and the identity pose: u = j and v = i exactly, warped is src;
    with t = (0.5, 0, 0), u = j + 8 exactly: src shifted by 8 columns, the last 8 columns invalid."""
    B, C, H, W = 2, 3, 9, 20
    g = torch.Generator().manual_seed(5)
    src = torch.rand(B, C, H, W, generator=g).numpy()
    k = np.array([[64, 0, 10], [0, 64, 4], [0, 0, 1]], dtype=np.float32)
    depth = np.full((B, H, W), 4.0, dtype=np.float32)
    m0 = (k.astype(np.float64) @ WC.rigid()).astype(np.float32)
    r = WC.rule_fp32(depth, k, src, m0)
    assert r["valid"].all() and np.array_equal(r["warped"], src)
    m1 = (k.astype(np.float64) @ WC.rigid(t=(0.5, 0, 0))).astype(np.float32)
    r = WC.rule_fp32(depth, k, src, m1)
    assert r["valid"][:, :, :W - 8].all() and not r["valid"][:, :, W - 8:].any()
    assert np.array_equal(r["warped"][..., :W - 8], src[..., 8:]) and (r["warped"][..., W - 8:] == 0).all()


def test_warp_projection_is_k_times_pose(nconv_amd):
    k = torch.tensor(WC.intrinsics(19, 70, 60.0), dtype=torch.float32)
    pose = torch.tensor(WC.rigid(0.01, -0.02, 0.005, (0.1, -0.2, 0.8)))
    want = (k.double() @ pose).float()[None]
    for p in (pose, torch.cat((pose, torch.tensor([[0.0, 0, 0, 1]], dtype=torch.float64))), pose[None].float()):
        assert torch.allclose(nconv_amd.warp_projection(k, p), want, rtol=1e-6, atol=1e-6)
    both = nconv_amd.warp_projection(torch.stack((k, 2 * k)), torch.stack((pose, pose)))
    assert both.shape == (2, 3, 4) and both.dtype == torch.float32 and both.is_contiguous()
    ident = torch.eye(4)
    assert torch.equal(nconv_amd.warp_projection(k, ident)[0], nconv_amd.projection_from_k(k))
    with pytest.raises(ValueError, match="pose must be"):
        nconv_amd.warp_projection(k, torch.eye(3))


def test_python_argument_checks(nconv_amd):
    """Shapes, C, dtypes and gradients are refused with a message wherever the call runs; then CPU
    tensors are, as everywhere else: there is no PyTorch path."""
    depth = torch.ones(2, 1, 4, 8)
    k = torch.eye(3)
    src = torch.ones(2, 3, 5, 9)
    tgt = torch.ones(2, 3, 4, 8)
    m = torch.zeros(2, 3, 4)
    W = nconv_amd.view_warp
    with pytest.raises(ValueError, match=r"depth must be \(B, 1, H, W\)"):
        W(depth[:, 0], k, src, m)
    with pytest.raises(TypeError, match="depth"):
        W(depth.double(), k, src, m)
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        W(depth, k, torch.ones(2, 2, 5, 9), m)
    with pytest.raises(ValueError, match="src must be"):
        W(depth, k, src[:1], m)
    with pytest.raises(TypeError, match="src"):
        W(depth, k, src.half(), m)
    with pytest.raises(ValueError, match="unit-stride rows"):
        W(depth, k, src.transpose(2, 3).contiguous().transpose(2, 3), m)
    with pytest.raises(ValueError, match="scatter"):
        W(depth, k, src.clone().requires_grad_(True), m)
    with pytest.raises(ValueError, match="m requires a gradient"):
        W(depth, k, src, m.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="m must be"):
        W(depth, k, src, torch.zeros(3, 3, 4))
    with pytest.raises(ValueError, match="k must be"):
        W(depth, torch.eye(4), src, m)
    with pytest.raises(ValueError, match="mask must be"):
        W(depth, k, src, m, mask=torch.ones(2, 1, 4, 7, dtype=torch.bool))
    with pytest.raises(TypeError, match="mask"):
        W(depth, k, src, m, mask=torch.ones(2, 1, 4, 8))
    with pytest.raises(ValueError, match="z_min"):
        W(depth, k, src, m, z_min=-1.0)
    with pytest.raises(ValueError, match="z_max"):
        W(depth, k, src, m, z_min=2.0, z_max=1.0)
    with pytest.raises(ValueError, match="tgt must be"):
        nconv_amd.photometric_loss(depth, k, tgt[:, :1], src, m)
    with pytest.raises(ValueError, match="does not match depth"):
        nconv_amd.photometric_loss(depth, k, torch.ones(2, 3, 4, 9), src, m)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        W(depth, k, src, m)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.photometric_loss(depth, k, tgt, src, m)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.PhotometricLoss()(depth, k, tgt, src, m)
    with pytest.raises(ValueError, match="z_min"):
        nconv_amd.PhotometricLoss(z_min=-1)
    assert nconv_amd.warp.workspace_bytes(2, 4, 8) == 8 + 2 * 8 + 2 * 4 + 2 * 8
    with pytest.raises(ValueError, match="too large"):
        nconv_amd.warp.workspace_bytes(1 << 20, 64, 64)


# ------------------------------------------------------------------------------------------------
# the C boundary from a plain C host
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "warp_host")


def test_host_descriptor_layout_matches_ctypes(nconv_amd, report):
    want = host_harness.ctypes_layout(nconv_amd._lib.NconvViewWarp, "nconv_view_warp")
    assert {key: report[key] for key in want} == want
    assert report["abi"] == [27, 27]


def test_host_workspace_sizes(report):
    small, full, zero_b, neg_w, odd = report["ws"]
    tiles = lambda B, H, W: B * ((H + 15) // 16) * ((W + 63) // 64)  # noqa: E731
    size = lambda B, H, W: 8 + 8 * B + 4 * (B + B % 2) + 8 * tiles(B, H, W)  # noqa: E731
    assert (small, full, odd) == (size(2, 4, 8), size(8, 352, 1216), size(3, 17, 65))
    assert zero_b == 0 and neg_w == 0 and odd % 8 == 0


ALL = ("wfwd", "wbwd", "pfwd", "pbwd")
PHOTO = ("pfwd", "pbwd")
ENTRY = {"wfwd": "nconv_view_warp_fwd", "wbwd": "nconv_view_warp_bwd", "pfwd": "nconv_photo_loss_fwd",
         "pbwd": "nconv_photo_loss_bwd"}


@pytest.mark.parametrize("case,why,sides", [
    ("null_descriptor", "null descriptor", ALL),
    ("null_depth", "null depth, src, k or m", ALL), ("null_src", "null depth, src, k or m", ALL),
    ("null_k", "null depth, src, k or m", ALL), ("null_m", "null depth, src, k or m", ALL),
    ("C_2", "C must be 1 or 3", ALL), ("C_0", "C must be 1 or 3", ALL), ("C_4", "C must be 1 or 3", ALL),
    ("B_zero", "non-positive", ALL), ("H_negative", "non-positive", ALL), ("Ws_zero", "non-positive", ALL),
    ("W_above_2_24", "at most 2^24", ALL), ("batch_too_large", "batch too large", ALL),
    ("k_stride_negative", "negative k or m image stride", ALL),
    ("m_stride_negative", "negative k or m image stride", ALL),
    ("z_min_negative", "z_min must be >= 0", ALL), ("z_min_nan", "z_min must be >= 0", ALL),
    ("z_max_below_z_min", "z_max < z_min", ALL), ("z_max_nan", "z_max < z_min", ALL),
    ("depth_misaligned", "not 4-byte aligned", ALL),
    ("depth_row_stride_short", "depth: row stride smaller than W", ALL),
    ("depth_row_stride_negative", "depth: row stride smaller than W", ALL),
    ("depth_image_stride_short", "depth: image stride smaller", ALL),
    ("mask_row_stride_short", "mask: row stride smaller than W", ALL),
    ("mask_image_stride_short", "mask: image stride smaller", ALL),
    ("src_row_stride_short", "src: row stride smaller than W", ALL),
    ("src_channel_stride_short", "src: channel stride smaller", ALL),
    ("src_image_stride_short", "src: image stride too small", ALL),
    ("src_stride_negative", "src: stride negative", ALL),
    ("depth_plane_too_large", "depth: plane too large", ALL), ("src_plane_too_large", "src: plane too large", ALL),
    ("mask_plane_too_large", "mask: plane too large", ALL),
    ("null_g_depth", "null g", ("wbwd", "pbwd")),
    ("null_tgt", "null tgt", PHOTO), ("tgt_row_stride_short", "tgt: row stride smaller than W", PHOTO),
    ("tgt_channel_stride_short", "tgt: channel stride smaller", PHOTO),
    ("tgt_plane_too_large", "tgt: plane too large", PHOTO),
    ("workspace_small", "workspace too small", PHOTO), ("workspace_null", "workspace too small", PHOTO),
    ("workspace_misaligned", "workspace not 8-byte aligned", PHOTO),
    ("null_loss", "null loss", ("pfwd",))])
def test_host_refuses_bad_arguments(report, case, why, sides):
    for side in sides:
        rc, text = report[f"{side}_{case}"]
        assert rc == -22 and why in text and text.startswith(ENTRY[side] + ":"), (side, rc, text)


def test_host_warp_only_checks(report):
    rc, text = report["wfwd_no_output_or_null_gradient"]
    assert rc == -22 and "null warped and valid" in text
    rc, text = report["wbwd_no_output_or_null_gradient"]
    assert rc == -22 and "null g_warped or g_depth" in text
