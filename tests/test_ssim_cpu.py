"""The SSIM photometric loss without a GPU: the fp32 rule of include/nconv.h (ssim_cases.rule_fp32, what the
kernels reproduce bit for bit) against the float64 torch composition (F.grid_sample, F.avg_pool2d on the
interior, the window-validity product, two masked means) and its autograd gradient of the depth, inside
kappa x the derived majorant; exact constructions; the L1 parity at alpha = 0; the Python argument checks; and
the host-side argument checks of nconv_photo_ssim_loss_* from a plain C program."""
import numpy as np
import pytest
import torch

import host_harness
import reduce_tree as RT
import ssim_cases as SC
import warp_cases as WC

CASES = [c[0] for c in SC.CPU_CASES]
f32 = np.float32


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def budgets():
    return {name: SC.case_budget(name) for name in CASES}


def test_kappa_json_is_complete_and_current(budgets):
    """A kappa_ref and kappa = 4 kappa_ref for every case and output; recomputed, the file's figures."""
    K = SC.load_kappa()
    assert set(K) == set(CASES)
    for name in CASES:
        assert set(K[name]) == set(SC.OUTPUTS)
        x, ref, keep, omit, A = budgets[name]
        got = SC.ratios(SC.composition(*SC.call_args(x), alpha=SC.ALPHA, data_range=x["data_range"],
                                       dtype=torch.float32), ref, keep, A)
        for key in SC.OUTPUTS:
            assert K[name][key]["kappa"] == pytest.approx(4 * K[name][key]["kappa_ref"], rel=1e-3)
            assert got[key] == pytest.approx(K[name][key]["kappa_ref"], rel=2e-2), (name, key)


def test_cases_cover_both_data_ranges():
    assert sorted(c[8] for c in SC.CPU_CASES) == [1.0, 255.0, 255.0]


@pytest.mark.parametrize("name", CASES)
def test_fp32_rule_matches_float64_composition(budgets, name):
    """Lw's terms and g_depth: |rule - float64| <= kappa A per compared element. The compared pixels of the
    gradient are those away from its discontinuities (the pixel's own integer crossings of u and v, x == y,
    clamp edges of its windows); at most 2 % are left out; the rule and the reference agree exactly on valid,
    on which pixels have a window, on n_v and on n_w, and 0 < n_w < n_v < B H W."""
    x, ref, keep, omit, A = budgets[name]
    rule = SC.rule_fp32(*SC.call_args(x), alpha=SC.ALPHA, data_range=x["data_range"])
    kappa = SC.kappa_for(SC.load_kappa())
    assert all(share <= 0.02 for share in omit.values()), omit
    assert np.array_equal(rule["valid"], ref["valid"]) and np.array_equal(rule["win"], ref["win"])
    assert (rule["n_v"], rule["n_w"]) == (ref["n_v"], ref["n_w"])
    assert 0 < rule["n_w"] < rule["n_v"] < rule["valid"].size
    for key in SC.OUTPUTS:
        err = np.abs(rule[key].astype(np.float64) - ref[key])
        worst = (err[keep[key]] / (kappa[key] * A[key][keep[key]] + 1e-300)).max()
        print(f"{name} {key}: err / (kappa A) max {worst:.3g}, kappa {kappa[key]:.4g}, omitted {omit[key]:.4f}")
        assert worst <= 1.0, (name, key, worst)
    assert (rule["terms_w"][~ref["win"]] == 0).all() and (ref["terms_w"][~ref["win"]] == 0).all()
    assert (rule["g_depth"][~ref["valid"]] == 0).all() and (ref["g_depth"][~ref["valid"]] == 0).all()
    # the value is continuous: Lw over ALL windows is inside the terms' budget
    C = x["src"].shape[1]
    bound = kappa["terms_w"] * A["terms_w"].sum() / (C * ref["n_w"]) + 4 * WC.U * abs(ref["loss_w"])
    assert abs(rule["terms_w"].astype(np.float64).sum() / (C * ref["n_w"]) - ref["loss_w"]) <= bound


def _exact(B=2, C=3, H=9, W=20, seed=5):
    g = torch.Generator().manual_seed(seed)
    src = (torch.rand(B, C, H, W, generator=g) * 255).numpy().astype(f32)
    k = np.array([[64, 0, 10], [0, 64, 4], [0, 0, 1]], dtype=f32)
    depth = np.full((B, H, W), 4.0, dtype=f32)
    m = (k.astype(np.float64) @ WC.rigid()).astype(f32)
    return depth, k, src, m


def test_identity_pose_and_equal_frames_give_zero():
    """fx = fy = 64, integer cx, cy, depth 4, the identity pose and tgt = src: x == y, so ssim == 1 exactly."""
    depth, k, src, m = _exact()
    B, C, H, W = src.shape
    r = SC.rule_fp32(depth, k, src, m, None, src.copy())
    assert r["L"] == 0 and r["n_v"] == B * H * W and r["n_w"] == B * (H - 2) * (W - 2)
    assert (r["terms_w"] == 0).all() and np.array_equal(r["warped"], src)


def test_constant_frames_equal_the_scalar_formula():
    depth, k, src, m = _exact(C=1)
    x, y = np.full_like(src, 0.5), np.full_like(src, 0.25)
    r = SC.rule_fp32(depth, k, x, m, None, y, alpha=1.0, data_range=1.0)
    c1, c2 = SC.constants(1.0)
    ssim = ((2 * 0.5 * 0.25 + float(c1)) * float(c2)) / ((0.25 + 0.0625 + float(c1)) * float(c2))
    t = r["terms_w"][r["win"]]
    assert (t == t[0]).all() and abs(float(t[0]) - (1 - ssim) / 2) <= 8 * WC.U and 0 < t[0] < 1


def test_no_window_is_the_l1_part_alone():
    """A 2 x 5 image has no window: n_w = 0, L = (1 - alpha) Lv, and the gradient is the L1 part's."""
    x = SC.ssim_inputs(9, 2, 3, (2, 5), (4, 8), True, False, 255.0)
    a = f32(0.85)
    r = SC.rule_fp32(*SC.call_args(x), alpha=0.85, data_range=255.0)
    assert r["n_w"] == 0 and r["n_v"] > 0 and RT.same_bits(r["L"], (f32(1) - a) * r["Lv"])
    l1 = WC.rule_fp32(*SC.call_args(x), None, gloss=float(f32(1) - a))
    assert np.array_equal(r["g_depth"], l1["g_depth_photo"])


def test_three_by_three_has_one_window():
    depth, k, src, m = _exact(B=1, H=3, W=3)
    k[0, 2] = k[1, 2] = 1
    m = (k.astype(np.float64) @ WC.rigid()).astype(f32)
    tgt = src[:, :, ::-1].copy()
    r = SC.rule_fp32(depth, k, src, m, None, tgt)
    assert (r["n_v"], r["n_w"]) == (9, 1) and r["win"][0, 1, 1] and r["L"] > 0
    depth[0, 2, 0] = 0.0
    r = SC.rule_fp32(depth, k, src, m, None, tgt)
    assert (r["n_v"], r["n_w"]) == (8, 0)


@pytest.mark.parametrize("name", CASES)
def test_alpha_zero_is_the_l1_rule(name):
    """alpha = 0: L and g_depth are warp_cases.rule_fp32's photometric outputs (the required property)."""
    x = SC.case_inputs(name)
    r = SC.rule_fp32(*SC.call_args(x), alpha=0.0, data_range=x["data_range"], gloss=3.0)
    l1 = WC.rule_fp32(*SC.call_args(x), None, gloss=3.0)
    assert np.array_equal(r["g_depth"], l1["g_depth_photo"])
    assert RT.same_bits(r["L"], RT.loss(l1["terms"], float(l1["den"]), RT.ROWS))


def test_python_argument_checks(nconv_amd):
    depth = torch.ones(2, 1, 4, 8)
    k = torch.eye(3)
    src = torch.ones(2, 3, 5, 9)
    tgt = torch.ones(2, 3, 4, 8)
    m = torch.zeros(2, 3, 4)
    P = nconv_amd.photometric_ssim_loss
    with pytest.raises(ValueError, match=r"alpha = 1.5 is outside \[0, 1\]"):
        P(depth, k, tgt, src, m, alpha=1.5)
    with pytest.raises(ValueError, match="alpha"):
        P(depth, k, tgt, src, m, alpha=float("nan"))
    with pytest.raises(ValueError, match="data_range"):
        P(depth, k, tgt, src, m, data_range=0.0)
    with pytest.raises(ValueError, match="data_range"):
        P(depth, k, tgt, src, m, data_range=float("inf"))
    with pytest.raises(TypeError, match="Python floats"):
        P(depth, k, tgt, src, m, alpha=torch.tensor(0.85))
    with pytest.raises(ValueError, match="tgt must be"):
        P(depth, k, tgt[:, :1], src, m)
    with pytest.raises(ValueError, match="does not match depth"):
        P(depth, k, torch.ones(2, 3, 4, 9), src, m)
    with pytest.raises(ValueError, match="scatter"):
        P(depth, k, tgt, src.clone().requires_grad_(True), m)
    with pytest.raises(ValueError, match="tgt requires a gradient"):
        P(depth, k, tgt.clone().requires_grad_(True), src, m)
    with pytest.raises(ValueError, match="k requires a gradient"):
        P(depth, k.clone().requires_grad_(True), tgt, src, m)
    with pytest.raises(ValueError, match="m requires a gradient"):
        P(depth, k, tgt, src, m.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="z_min"):
        P(depth, k, tgt, src, m, z_min=-1.0)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        P(depth, k, tgt, src, m)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.PhotometricLoss(alpha=0.85)(depth, k, tgt, src, m)
    with pytest.raises(ValueError, match="alpha"):
        nconv_amd.PhotometricLoss(alpha=-0.1)
    with pytest.raises(ValueError, match="alpha"):
        nconv_amd.ViewWarper((4, 8), alpha=2.0, device="cpu")
    assert nconv_amd.PhotometricLoss().alpha == 0.0
    assert nconv_amd.warp.ssim_workspace_bytes(2, 4, 8) == 8 + 24 * 2 + 16 * 2
    with pytest.raises(ValueError, match="too large"):
        nconv_amd.warp.ssim_workspace_bytes(1 << 20, 64, 64)


# ------------------------------------------------------------------------------------------------
# the C boundary from a plain C host
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "ssim_host")


def test_host_exports_and_abi(nconv_amd, report):
    assert report["abi"] == [27, 27]
    for name in ("nconv_photo_ssim_workspace_bytes", "nconv_photo_ssim_loss_fwd", "nconv_photo_ssim_loss_bwd"):
        assert name in nconv_amd._lib.EXPORTED


def test_host_workspace_sizes(report):
    small, full, zero_b, neg_w, odd = report["ws"]
    tiles = lambda B, H, W: B * ((H + 15) // 16) * ((W + 63) // 64)  # noqa: E731
    size = lambda B, H, W: 8 + 24 * B + 16 * tiles(B, H, W)  # noqa: E731
    assert (small, full, odd) == (size(2, 4, 8), size(8, 352, 1216), size(3, 17, 65))
    assert zero_b == 0 and neg_w == 0 and odd % 8 == 0


BOTH = ("fwd", "bwd")
ENTRY = {"fwd": "nconv_photo_ssim_loss_fwd", "bwd": "nconv_photo_ssim_loss_bwd"}


@pytest.mark.parametrize("case,why", [
    ("null_descriptor", "null descriptor"),
    ("null_depth", "null depth, src, k or m"), ("null_src", "null depth, src, k or m"),
    ("null_k", "null depth, src, k or m"), ("null_m", "null depth, src, k or m"),
    ("C_2", "C must be 1 or 3"), ("C_0", "C must be 1 or 3"), ("C_4", "C must be 1 or 3"),
    ("B_zero", "non-positive"), ("H_negative", "non-positive"), ("Ws_zero", "non-positive"),
    ("W_above_2_24", "at most 2^24"), ("batch_too_large", "batch too large"),
    ("k_stride_negative", "negative k or m image stride"), ("m_stride_negative", "negative k or m image stride"),
    ("z_min_negative", "z_min must be >= 0"), ("z_min_nan", "z_min must be >= 0"),
    ("z_max_below_z_min", "z_max < z_min"), ("z_max_nan", "z_max < z_min"),
    ("depth_misaligned", "not 4-byte aligned"),
    ("depth_row_stride_short", "depth: row stride smaller than W"),
    ("depth_row_stride_negative", "depth: row stride smaller than W"),
    ("depth_image_stride_short", "depth: image stride smaller"),
    ("mask_row_stride_short", "mask: row stride smaller than W"),
    ("mask_image_stride_short", "mask: image stride smaller"),
    ("src_row_stride_short", "src: row stride smaller than W"),
    ("src_channel_stride_short", "src: channel stride smaller"),
    ("src_image_stride_short", "src: image stride too small"),
    ("src_stride_negative", "src: stride negative"),
    ("depth_plane_too_large", "depth: plane too large"), ("src_plane_too_large", "src: plane too large"),
    ("mask_plane_too_large", "mask: plane too large"),
    ("null_tgt", "null tgt"), ("tgt_row_stride_short", "tgt: row stride smaller than W"),
    ("tgt_channel_stride_short", "tgt: channel stride smaller"), ("tgt_plane_too_large", "tgt: plane too large"),
    ("workspace_small", "workspace too small"), ("workspace_null", "workspace too small"),
    ("workspace_misaligned", "workspace not 8-byte aligned"),
    ("alpha_negative", "alpha must be in [0, 1]"), ("alpha_above_one", "alpha must be in [0, 1]"),
    ("alpha_nan", "alpha must be in [0, 1]"),
    ("c1_zero", "c1 and c2 must be finite and > 0"), ("c1_negative", "c1 and c2 must be finite and > 0"),
    ("c1_nan", "c1 and c2 must be finite and > 0"), ("c1_infinite", "c1 and c2 must be finite and > 0"),
    ("c2_zero", "c1 and c2 must be finite and > 0"), ("c2_nan", "c1 and c2 must be finite and > 0"),
    ("c2_infinite", "c1 and c2 must be finite and > 0")])
def test_host_refuses_bad_arguments(report, case, why):
    for side in BOTH:
        rc, text = report[f"{side}_{case}"]
        assert rc == -22 and why in text and text.startswith(ENTRY[side] + ":"), (side, rc, text)


def test_host_refuses_null_outputs(report):
    rc, text = report["fwd_null_output"]
    assert rc == -22 and "null loss" in text
    rc, text = report["bwd_null_output"]
    assert rc == -22 and "null g_depth" in text
