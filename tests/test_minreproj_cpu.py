"""The minimum-reprojection loss without a GPU: the fp32 rule of include/nconv.h (minreproj_cases.min_rule_fp32,
what the kernels reproduce bit for bit) against the existing restatements at S = 1, against a float64 torch
composition that is fed the rule's winner plane (inside kappa x the derived majorant), the selection itself
checked separately in float64, the Python argument checks, and the host-side argument checks of
nconv_photo_min_loss_* from a plain C program."""
import numpy as np
import pytest
import torch

import host_harness
import minreproj_cases as MC
import reduce_tree as RT
import ssim_cases as SC
import warp_cases as WC

CASES = [c[0] for c in MC.CPU_CASES]
f32 = np.float32


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def budgets():
    return {name: MC.case_budget(name) for name in CASES}


# ------------------------------------------------------------------------------------------------
# agreement with the existing restatements
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in SC.CPU_CASES])
def test_one_source_is_the_existing_rules(name):
    """S = 1, no auto-mask: at alpha = 1 L, n_c and g_depth are ssim_cases.rule_fp32's bitwise, at alpha = 0
    warp_cases.rule_fp32's photometric ones (the two required properties)."""
    x = SC.case_inputs(name)
    a = SC.call_args(x)
    one = (x["depth"], x["k"], [x["src"]], [x["m"]], x["mask"], x["tgt"])
    r = MC.min_rule_fp32(*one, alpha=1.0, data_range=x["data_range"], automask=False, gloss=3.0)
    s = SC.rule_fp32(*a, alpha=1.0, data_range=x["data_range"], gloss=3.0)
    assert RT.same_bits(r["L"], s["L"]) and r["n_c"] == s["n_w"] > 0 and np.array_equal(r["g_depth"], s["g_depth"])
    assert np.array_equal(r["winner"] == 0, s["win"]) and r["n_m"] == 0
    r = MC.min_rule_fp32(*one, alpha=0.0, data_range=x["data_range"], automask=False, gloss=3.0)
    l1 = WC.rule_fp32(*a, None, gloss=3.0)
    assert RT.same_bits(r["L"], RT.loss(l1["terms"], float(l1["den"]), RT.ROWS)) and r["n_c"] == l1["n_v"] > 0
    assert np.array_equal(r["g_depth"], l1["g_depth_photo"]) and np.array_equal(r["winner"] == 0, l1["valid"])


@pytest.mark.parametrize("alpha", [0.0, 0.85])
def test_two_identical_sources_are_one(alpha):
    """Two identical sources: the lowest index wins every tie, so winner is 0 wherever there is one, and L and
    g_depth are bitwise the S = 1 ones (source 1 wins nothing and adds +0)."""
    x = SC.case_inputs("64x96_c3_r255")
    one = (x["depth"], x["k"], [x["src"]], [x["m"]], x["mask"], x["tgt"])
    two = (x["depth"], x["k"], [x["src"], x["src"].copy()], [x["m"], x["m"].copy()], x["mask"], x["tgt"])
    r1 = MC.min_rule_fp32(*one, alpha=alpha, automask=False)
    r2 = MC.min_rule_fp32(*two, alpha=alpha, automask=False)
    assert set(np.unique(r2["winner"])) == {0, MC.NONE} and np.array_equal(r1["winner"], r2["winner"])
    assert RT.same_bits(r1["L"], r2["L"]) and r1["g_depth"].tobytes() == r2["g_depth"].tobytes()


def test_masked_pixels_stay_in_the_mean():
    """The denominator is n_c, not the kept count: with auto-masking the sum loses the masked pixels' terms and
    nothing else changes."""
    x = MC.case_inputs(CASES[0])
    a = MC.min_rule_fp32(*MC.call_args(x), alpha=0.85, automask=True)
    b = MC.min_rule_fp32(*MC.call_args(x), alpha=0.85, automask=False)
    C = x["tgt"].shape[1]
    assert a["n_c"] == b["n_c"] and 0 < a["n_m"] < a["n_c"] and np.array_equal(a["has"], b["has"])
    assert np.array_equal(a["terms"], np.where(a["masked"], f32(0), b["terms"]))
    assert RT.same_bits(a["L"], RT.loss(a["terms"], float(C * a["n_c"]), RT.ROWS)) and a["L"] < b["L"]
    assert (a["error"][a["masked"]] == 0).all() and np.array_equal(a["error"][a["kept"]], b["error"][a["kept"]])


# ------------------------------------------------------------------------------------------------
# the rule against the float64 reference
# ------------------------------------------------------------------------------------------------
def test_kappa_json_is_complete_and_current(budgets):
    """A kappa_ref and kappa = 4 kappa_ref for every case and output; recomputed, the file's figures."""
    K = MC.load_kappa()
    assert set(K) == set(CASES)
    for name in CASES:
        assert set(K[name]) == set(MC.OUTPUTS)
        x, rule, ref, keep, omit, A = budgets[name]
        got = MC.ratios(MC.composition(*MC.call_args(x), winner=rule["winner"], alpha=MC.ALPHA,
                                       data_range=x["data_range"], dtype=torch.float32), ref, keep, A)
        for key in MC.OUTPUTS:
            assert K[name][key]["kappa"] == pytest.approx(4 * K[name][key]["kappa_ref"], rel=1e-3)
            assert got[key] == pytest.approx(K[name][key]["kappa_ref"], rel=2e-2), (name, key)


@pytest.mark.parametrize("name", CASES)
def test_fp32_rule_matches_float64_composition(budgets, name):
    """E of every source and g_depth: |rule - float64| <= kappa A per compared element, the float64 composition
    fed the rule's winner plane. The rule and the reference agree exactly on every source's validity and
    comparable pixels; at most 3 % of the gradient's pixels (S sources' discontinuities) are left out."""
    x, rule, ref, keep, omit, A = budgets[name]
    kappa = MC.kappa_for(MC.load_kappa())
    assert all(share <= 0.03 for share in omit.values()), omit
    assert np.array_equal(rule["comparable"], ref["comparable"]) and rule["n_c"] == ref["n_c"]
    assert all(np.array_equal(rule["valid"][s], p["valid"]) for s, p in enumerate(ref["per"]))
    assert 0 < rule["n_c"] < rule["has"].size and len(np.unique(rule["winner"])) >= len(x["srcs"]) + 1
    got = {"E": np.where(rule["comparable"], rule["E"], f32(0)), "g_depth": rule["g_depth"]}
    for key in MC.OUTPUTS:
        err = np.abs(got[key].astype(np.float64) - ref[key])
        worst = (err[keep[key]] / (kappa[key] * A[key][keep[key]] + 1e-300)).max()
        print(f"{name} {key}: err / (kappa A) max {worst:.3g}, kappa {kappa[key]:.4g}, omitted {omit[key]:.4f}")
        assert worst <= 1.0, (name, key, worst)
    # the value is continuous: L is inside the kept terms' budget
    C = x["tgt"].shape[1]
    kept = rule["kept"]
    sel = np.where(kept, rule["winner"], 0).astype(np.int64)[None]
    A_best = np.take_along_axis(A["E"], sel, 0)[0][kept]
    bound = kappa["E"] * A_best.sum() / (C * ref["n_c"]) + WC.loss_bound(rule["terms"], C * ref["n_c"], rule["L"])
    assert abs(float(rule["L"]) - ref["loss"]) <= bound


@pytest.mark.parametrize("name", CASES)
def test_selection_in_float64(budgets, name):
    """The winner is, in float64, within the fp32 error bound of the smallest comparable error; a pixel is
    masked only if Imin64 <= E64min + tau and kept only if Imin64 + tau >= E64min, tau the fp32 error bounds of
    the quantities compared (kappa x the majorants)."""
    x, rule, ref, keep, omit, A = budgets[name]
    kE = MC.kappa_for(MC.load_kappa())["E"]
    automask = next(c for c in MC.CPU_CASES if c[0] == name)[9]
    E = np.where(ref["comparable"], ref["E"], np.inf)
    has = rule["has"]
    arg = np.argmin(E, axis=0)[None]
    Emin, A_min = np.take_along_axis(E, arg, 0)[0], np.take_along_axis(A["E"], arg, 0)[0]
    w = np.where(has, np.where(rule["masked"], 0, rule["winner"]), 0).astype(np.int64)
    if rule["masked"].any():  # the winner of a masked pixel is not in the plane: take it from the rule's best
        w = np.where(rule["masked"], np.argmin(np.abs(rule["E"].astype(np.float64)
                                                      - rule["best"][None].astype(np.float64)), axis=0), w)
    Ew, A_w = np.take_along_axis(E, w[None], 0)[0], np.take_along_axis(A["E"], w[None], 0)[0]
    tau = kE * (A_w + A_min)
    assert np.isfinite(Ew[has]).all() and (Ew[has] <= Emin[has] + tau[has]).all()
    assert np.array_equal(has, np.isfinite(Emin))
    if automask:
        I, A_I = MC.identity64(x, MC.ALPHA)
        argi = np.argmin(I, axis=0)[None]
        Imin, A_imin = np.take_along_axis(I, argi, 0)[0], np.take_along_axis(A_I, argi, 0)[0]
        tau2 = tau + kE * A_imin
        m, kpt = rule["masked"], rule["kept"]
        assert m.any() and kpt.any()
        assert (Imin[m] <= Emin[m] + tau2[m]).all() and (Imin[kpt] + tau2[kpt] >= Emin[kpt]).all()
    else:
        assert not rule["masked"].any()


# ------------------------------------------------------------------------------------------------
# the Python argument checks
# ------------------------------------------------------------------------------------------------
def test_python_argument_checks(nconv_amd):
    depth = torch.ones(2, 1, 4, 8)
    k = torch.eye(3)
    src = torch.ones(2, 3, 4, 8)
    tgt = torch.ones(2, 3, 4, 8)
    m = torch.zeros(2, 3, 4)
    P = nconv_amd.min_reprojection_loss
    with pytest.raises(ValueError, match=r"need 1\.\.4 sources"):
        P(depth, k, tgt, [], [])
    with pytest.raises(ValueError, match=r"need 1\.\.4 sources"):
        P(depth, k, tgt, [src] * 5, [m] * 5)
    with pytest.raises(ValueError, match="as many matrices"):
        P(depth, k, tgt, [src, src], [m])
    with pytest.raises(ValueError, match=r"alpha = 1.5 is outside \[0, 1\]"):
        P(depth, k, tgt, [src], [m], alpha=1.5)
    with pytest.raises(ValueError, match="data_range"):
        P(depth, k, tgt, [src], [m], data_range=0.0)
    with pytest.raises(TypeError, match="Python floats"):
        P(depth, k, tgt, [src], [m], alpha=torch.tensor(0.85))
    with pytest.raises(ValueError, match=r"automask.*srcs\[1\] is 5 x 9"):
        P(depth, k, tgt, [src, torch.ones(2, 3, 5, 9)], [m, m])
    with pytest.raises(ValueError, match="tgt must be"):
        P(depth, k, tgt[:, :1], [src], [m])
    with pytest.raises(ValueError, match="scatter"):
        P(depth, k, tgt, [src.clone().requires_grad_(True), src], [m, m])
    with pytest.raises(ValueError, match="tgt requires a gradient"):
        P(depth, k, tgt.clone().requires_grad_(True), [src], [m])
    with pytest.raises(ValueError, match="m requires a gradient"):
        P(depth, k, tgt, [src], [m.clone().requires_grad_(True)])
    with pytest.raises(ValueError, match="z_min"):
        P(depth, k, tgt, [src], [m], z_min=-1.0)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        P(depth, k, tgt, [src, src], [m, m])
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.MinReprojectionLoss()(depth, k, tgt, (src, src), (m, m))
    with pytest.raises(ValueError, match="alpha"):
        nconv_amd.MinReprojectionLoss(alpha=-0.1)
    with pytest.raises(ValueError, match="S in 1..4"):
        nconv_amd.MinReprojector((4, 8), S=5, device="cpu")
    assert nconv_amd.MinReprojectionLoss().alpha == 0.85 and nconv_amd.MinReprojectionLoss().automask is True
    assert nconv_amd.warp.min_workspace_bytes(2, 4, 8) == 8 + 16 * 2 + 12 * 2 + 2 * 4 * 8
    with pytest.raises(ValueError, match="too large"):
        nconv_amd.warp.min_workspace_bytes(1 << 20, 64, 64)


# ------------------------------------------------------------------------------------------------
# the C boundary from a plain C host
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "minreproj_host")


def test_host_exports_and_abi(nconv_amd, report):
    assert report["abi"] == [27, 27]
    for name in ("nconv_photo_min_workspace_bytes", "nconv_photo_min_loss_fwd", "nconv_photo_min_loss_bwd"):
        assert name in nconv_amd._lib.EXPORTED


def test_host_workspace_sizes(report):
    small, full, zero_b, neg_w, odd = report["ws"]
    tiles = lambda B, H, W: B * ((H + 15) // 16) * ((W + 63) // 64)  # noqa: E731
    size = lambda B, H, W: (8 + 16 * B + 12 * tiles(B, H, W) + B * H * W + 7) // 8 * 8  # noqa: E731
    assert (small, full, odd) == (size(2, 4, 8), size(8, 352, 1216), size(3, 17, 65))
    assert zero_b == 0 and neg_w == 0 and odd % 8 == 0 and (8 + 48 + 36 + 3 * 17 * 65) % 8 != 0


BOTH = ("fwd", "bwd")
ENTRY = {"fwd": "nconv_photo_min_loss_fwd", "bwd": "nconv_photo_min_loss_bwd"}
PER_VIEW = [
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
    ("src_plane_too_large", "src: plane too large")]


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("case,why", PER_VIEW)
def test_host_refuses_what_the_single_source_loss_refuses_for_each_view(report, case, why, view):
    for side in BOTH:
        rc, text = report[f"{side}_v{view}_{case}"]
        assert rc == -22 and text.startswith(f"{ENTRY[side]}: view {view}: ") and why in text, (side, rc, text)


@pytest.mark.parametrize("case,why", [
    ("null_descriptor", "null descriptor"),
    ("null_tgt", "null tgt"), ("tgt_row_stride_short", "tgt: row stride smaller than W"),
    ("tgt_channel_stride_short", "tgt: channel stride smaller"),
    ("workspace_small", "workspace too small"), ("workspace_ssim_sized", "workspace too small"),
    ("workspace_null", "workspace too small"), ("workspace_misaligned", "workspace not 8-byte aligned"),
    ("alpha_negative", "alpha must be in [0, 1]"), ("alpha_above_one", "alpha must be in [0, 1]"),
    ("alpha_nan", "alpha must be in [0, 1]"),
    ("c1_zero", "c1 and c2 must be finite and > 0"), ("c1_nan", "c1 and c2 must be finite and > 0"),
    ("c2_negative", "c1 and c2 must be finite and > 0"), ("c2_infinite", "c1 and c2 must be finite and > 0"),
    ("S_zero", "S must be in 1..4"), ("S_negative", "S must be in 1..4"), ("S_five", "S must be in 1..4"),
    ("differ_B", "view 1 differs from view 0 in B, C, H or W"),
    ("differ_C", "view 1 differs from view 0 in B, C, H or W"),
    ("differ_H", "view 1 differs from view 0 in B, C, H or W"),
    ("differ_W", "view 1 differs from view 0 in B, C, H or W"),
    ("differ_depth", "view 1 differs from view 0 in the depth view"),
    ("differ_depth_row_stride", "view 1 differs from view 0 in the depth view"),
    ("differ_depth_image_stride", "view 1 differs from view 0 in the depth view"),
    ("differ_mask", "view 1 differs from view 0 in the mask view"),
    ("differ_mask_strides", "view 1 differs from view 0 in the mask view"),
    ("differ_k", "view 1 differs from view 0 in k"), ("differ_k_stride", "view 1 differs from view 0 in k"),
    ("differ_z_min", "view 1 differs from view 0 in z_min or z_max"),
    ("differ_z_max", "view 1 differs from view 0 in z_min or z_max"),
    ("differ_in_third_view", "view 2 differs from view 0 in z_min or z_max"),
    ("automask_other_size", "automask needs sources of the target's size: view 0"),
    ("automask_two", "automask must be 0 or 1"),
    ("automask_one_other_size", "automask needs sources of the target's size: view 1"),
    ("automask_good_but_workspace", "workspace too small")])
def test_host_refuses_bad_arguments(report, case, why):
    for side in BOTH:
        rc, text = report[f"{side}_{case}"]
        assert rc == -22 and why in text and text.startswith(ENTRY[side] + ":"), (side, rc, text)


def test_host_refuses_null_outputs(report):
    rc, text = report["fwd_null_output"]
    assert rc == -22 and "null loss" in text
    rc, text = report["bwd_null_output"]
    assert rc == -22 and "null g_depth" in text
