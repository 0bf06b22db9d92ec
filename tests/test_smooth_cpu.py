"""The smoothness loss and the edge weights without a GPU: the fp32 rule of include/nconv.h
(smooth_cases.rule_fp32, E, edge_weights_rule: what the kernels reproduce bit for bit) against the float64
torch composition (slices, abs, exp, means) and its autograd gradient of the depth, inside kappa x the
derived majorant; E against float64 exp(-x) with the figure the header records; exact constructions; the
pyramid helpers; the Python argument checks; and the host-side argument checks of nconv_smooth_loss_* /
nconv_edge_weights from a plain C program."""
import numpy as np
import pytest
import torch

import host_harness
import smooth_cases as SC

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
        args, ref, maj = budgets[name]
        got = SC.ratios(SC.composition(*args, dtype=torch.float32), ref, maj)
        for key in SC.OUTPUTS:
            assert K[name][key]["kappa"] == pytest.approx(4 * K[name][key]["kappa_ref"], rel=1e-3)
            assert got[key] == pytest.approx(K[name][key]["kappa_ref"], rel=2e-2), (name, key)


@pytest.mark.parametrize("name", CASES)
def test_fp32_rule_matches_float64_composition(budgets, name):
    """L and g_depth: |rule - float64| <= kappa A (the loss with the 4 U |L| the warp's test allows its final
    rounding). The gradient is compared where every term of the element has |t| exactly 0 or above
    4 U sum |operands| in float64, so that its sign is the reference's; at most 1 % of the elements are left
    out; the inputs hold exactly equal neighbours, so sign(0) = 0 takes part. The counts are the
    reference's."""
    args, ref, maj = budgets[name]
    A_L, A_g, keep, zeros = maj
    rule = SC.rule_fp32(*args)
    kappa = SC.kappa_for(SC.load_kappa())
    omitted = 1.0 - keep.mean()
    assert omitted <= 0.01, omitted
    assert zeros > 0
    assert (rule["n_x"], rule["n_y"]) == (ref["n_x"], ref["n_y"]) and rule["n_x"] > 0 and rule["n_y"] > 0
    err = np.abs(rule["g_depth"].astype(np.float64) - ref["g_depth"])[keep]
    worst = (err / (kappa["g_depth"] * A_g[keep] + 1e-300)).max()
    eL = abs(float(rule["L"]) - ref["L"])
    print(f"{name}: g_depth err / (kappa A) max {worst:.3g}, kappa {kappa['g_depth']:.4g}, omitted {omitted:.4f}, "
          f"zero terms {zeros}; L err {eL:.3g}, kappa A_L {kappa['L'] * A_L:.3g}, 4 U |L| {4 * SC.U * abs(ref['L']):.3g}")
    assert worst <= 1.0, (name, worst)
    assert eL <= kappa["L"] * A_L + 4 * SC.U * abs(ref["L"])


def test_reference_inputs_flip_no_sign():
    """The stated inputs at 33 x 130 and 17 x 65, both orders, no mask: the float64 reference leaves out no
    element, the fp32 terms have the float64 terms' signs, and exactly-zero terms exist."""
    for H, W in ((33, 130), (17, 65)):
        d = SC.smooth_depth(2, H, W, seed=H)
        for order in (1, 2):
            _, _, keep, zeros = SC.majorants(d, None, order)
            (cx, tx, _, _), (cy, ty, _, _) = SC._terms64(d, None, order, None)
            rule = SC.rule_fp32(d, None, order)
            assert keep.all() and zeros >= 90
            assert np.array_equal(np.sign(rule["tx"])[cx], np.sign(tx)[cx])
            assert np.array_equal(np.sign(rule["ty"])[cy], np.sign(ty)[cy])


def test_E_matches_float64_exp_to_the_recorded_error():
    """E against float64 exp(-x) over the arguments alpha g reaches, g in [0, 255], at alpha = 1 / 255 and
    alpha = 1: the largest relative error, recomputed, is the figure written beside the rule in
    include/nconv.h; E(0) is exactly 1, E is +0 past its flush point and for a NaN."""
    recorded = SC.header_e_errors()
    for key, alpha in (("1/255", 1.0 / 255.0), ("1", 1.0)):
        got = SC.e_error(alpha)
        print(f"alpha = {key}: max relative error {got:.3e}, recorded {recorded[key]}")
        assert f"{got:.3e}" == recorded[key]
    e = SC.E(np.array([0.0, 86.0, 87.5, 255.0, np.inf, np.nan], dtype=f32))
    assert e[0] == 1.0 and e[1] > 0 and (e[2:] == 0).all() and not np.signbit(e[2:]).any()


def test_edge_weights_rule_matches_float64():
    """The rule's weights against exp(-alpha mean |dI|) in float64: within the recorded error of E plus the
    argument's own rounding (each |difference| one rounding, two sums, the division, the product: 5 U x)."""
    g = torch.Generator().manual_seed(3)
    rec = SC.header_e_errors()
    for C, alpha, key in ((3, 1.0 / 255.0, "1/255"), (1, 1.0 / 255.0, "1/255"), (3, 1.0, "1")):
        img = torch.randint(0, 256, (2, C, 17, 33), generator=g).float().numpy()
        if alpha == 1.0:
            img = (img / 255.0).astype(f32) * f32(40.0)
        got = SC.edge_weights_rule(img, alpha).astype(np.float64)
        want = SC.edge_weights_composition(img, alpha)
        x = -np.log(want) + alpha * np.abs(img).max()  # a difference's rounding is relative to its operands
        assert (np.abs(got - want) <= want * (float(rec[key]) + 5 * SC.U * x + SC.U)).all()
        assert (got[:, 0, :, -1] == 1).all() and (got[:, 1, -1, :] == 1).all()


def test_plane_is_exact():
    """d = a i + b j with small dyadic a, b: every second difference is exactly 0, every first difference
    exactly b or a, so the order-2 loss is 0 with a zero gradient and the order-1 loss is |b| + |a|."""
    i = np.arange(9, dtype=f32)[:, None]
    j = np.arange(20, dtype=f32)[None, :]
    a, b = f32(0.25), f32(-0.375)
    d = (a * i + b * j + f32(3.0))[None].repeat(2, axis=0)
    r2 = SC.rule_fp32(d, None, 2)
    assert r2["L"] == 0 and (r2["g_depth"] == 0).all() and r2["n_x"] == 2 * 9 * 18 and r2["n_y"] == 2 * 7 * 20
    r1 = SC.rule_fp32(d, None, 1)
    assert r1["L"] == f32(0.625) and r1["n_x"] == 2 * 9 * 19 and r1["n_y"] == 2 * 8 * 20
    inner = r1["g_depth"][:, 1:-1, 1:-1]
    assert (inner == 0).all()  # the two x terms of an inner pixel cancel, and the two y terms


def _step(H=6, W=8, col=4, lo=1.0, hi=3.0):
    d = np.full((1, H, W), lo, dtype=f32)
    d[:, :, col:] = hi
    return d


def test_step_edge_gradient_by_hand():
    """A single vertical step between columns 3 and 4 of a 6 x 8 image. Order 1: n_x = 42 terms, six of
    them non-zero (+2), so L = 12 / 42 and g_depth is -1/42 in column 3, +1/42 in column 4, 0 elsewhere.
    Order 2: t = +2 centred on column 3 and -2 on column 4 (n_x = 36): with q = 1/36,
    g = (+q, -2q - q, +q + 2q, -q) on columns 2 .. 5. A zero weight on that edge removes it; with order 2 the
    min takes the zero into both terms that straddle it."""
    d = _step()
    r = SC.rule_fp32(d, None, 1)
    q = f32(1.0) / f32(42.0)
    want = np.zeros((1, 6, 8), dtype=f32)
    want[:, :, 3], want[:, :, 4] = -q, q
    assert r["n_x"] == 42 and r["n_y"] == 40 and np.array_equal(r["g_depth"], want)
    assert r["L"] == f32(np.float64(12.0) / 42.0)
    r = SC.rule_fp32(d, None, 2)
    q = f32(1.0) / f32(36.0)
    want = np.zeros((1, 6, 8), dtype=f32)
    want[:, :, 2], want[:, :, 3], want[:, :, 4], want[:, :, 5] = q, (-q) - f32(2) * q, q + f32(2) * q, -q
    assert r["n_x"] == 36 and np.array_equal(r["g_depth"], want)
    assert r["L"] == f32(np.float64(24.0) / 36.0)
    w = np.ones((1, 2, 6, 8), dtype=f32)
    w[:, 0, :, 3] = 0
    for order in (1, 2):
        r = SC.rule_fp32(d, w, order)
        assert r["L"] == 0 and (r["g_depth"] == 0).all() and r["n_x"] == (42 if order == 1 else 36)


def test_mask_removes_the_terms_it_touches():
    """One masked pixel (2, 3) of a 6 x 8 image. Order 1: its two x terms and two y terms leave (42 - 2,
    40 - 2); order 2: the three x and three y terms whose stencil holds it (36 - 3, 32 - 3). With the step
    beside it the gradient of row 2 loses exactly the terms that cross the pixel; a NaN under the mask does
    not reach the loss."""
    d = _step()
    d[0, 2, 3] = np.nan
    mask = np.ones((1, 6, 8), dtype=np.uint8)
    mask[0, 2, 3] = 0
    r = SC.rule_fp32(d, None, 1, mask)
    assert (r["n_x"], r["n_y"]) == (40, 38)
    assert r["L"] == f32(np.float64(10.0) / 40.0) and np.isfinite(r["g_depth"]).all()
    assert (r["g_depth"][0, 2] == 0).all() and r["g_depth"][0, 1, 3] == -(f32(1) / f32(40))
    r = SC.rule_fp32(d, None, 2, mask)
    assert (r["n_x"], r["n_y"]) == (33, 29) and np.isfinite(r["L"])
    q = f32(1) / f32(33)
    assert np.isfinite(r["g_depth"]).all() and (r["g_depth"][0, 2] == 0).all() and r["g_depth"][0, 1, 2] == q
    r = SC.rule_fp32(_step(), None, 1, np.zeros((1, 6, 8), dtype=np.uint8))
    assert (r["n_x"], r["n_y"], float(r["L"])) == (0, 0, 0.0) and (r["g_depth"] == 0).all()


def test_degenerate_shapes():
    """1 x 1, 1 x W, H x 1, 2 x 2: the missing directions have n = 0 and contribute nothing."""
    for shape, o1, o2 in (((1, 1), (0, 0), (0, 0)), ((1, 5), (4, 0), (3, 0)), ((5, 1), (0, 4), (0, 3)),
                          ((2, 2), (2, 2), (0, 0))):
        d = SC.smooth_depth(1, *shape, seed=2)
        for order, want in ((1, o1), (2, o2)):
            r = SC.rule_fp32(d, None, order)
            c = SC.composition(d, None, order)
            assert (r["n_x"], r["n_y"]) == want == (c["n_x"], c["n_y"])
            assert abs(float(r["L"]) - c["L"]) <= 1e-5 and np.allclose(r["g_depth"], c["g_depth"], atol=1e-5)


def test_halved_matrices_project_to_the_half_resolution_grid(nconv_amd):
    """For random points, projecting with halve_projection(m) gives ((u - 0.5) / 2, (v - 0.5) / 2) of the
    full-resolution projection, and halve_intrinsics(k) back-projects the level's pixel j' to the ray of the
    full-resolution coordinate 2 j' + 0.5: float64, to rounding."""
    g = torch.Generator().manual_seed(11)
    k = torch.tensor([[721.5, 0, 609.6], [0, 718.9, 172.9], [0, 0, 1]], dtype=torch.float64)
    pose = torch.cat((torch.eye(3, dtype=torch.float64), torch.tensor([[0.3], [-0.1], [0.5]], dtype=torch.float64)), 1)
    m = k @ pose
    P = torch.cat((torch.rand(3, 100, generator=g, dtype=torch.float64) * 20 + 1, torch.ones(1, 100, dtype=torch.float64)))
    full = m @ P
    half = nconv_amd.halve_projection(m) @ P
    u, v = full[0] / full[2], full[1] / full[2]
    assert torch.allclose(half[0] / half[2], (u - 0.5) / 2, rtol=1e-13, atol=1e-11)
    assert torch.allclose(half[1] / half[2], (v - 0.5) / 2, rtol=1e-13, atol=1e-11)
    k2 = nconv_amd.halve_intrinsics(k)
    jp = torch.arange(50, dtype=torch.float64)
    assert torch.allclose((jp - k2[0, 2]) / k2[0, 0], (2 * jp + 0.5 - k[0, 2]) / k[0, 0], rtol=1e-13, atol=1e-13)
    assert torch.allclose((jp - k2[1, 2]) / k2[1, 1], (2 * jp + 0.5 - k[1, 2]) / k[1, 1], rtol=1e-13, atol=1e-13)
    assert torch.equal(k2[2], k[2]) and k2[0, 1] == 0
    kb = nconv_amd.halve_intrinsics(torch.stack((k, k)).float())
    assert kb.shape == (2, 3, 3) and kb.dtype == torch.float32 and torch.equal(kb[0], k2.float())
    assert nconv_amd.halve_projection(m[None].float()).shape == (1, 3, 4)
    with pytest.raises(ValueError, match="k must be"):
        nconv_amd.halve_intrinsics(m)
    with pytest.raises(ValueError, match="m must be"):
        nconv_amd.halve_projection(k)


def test_python_argument_checks(nconv_amd):
    """Shapes, order, dtypes and gradients are refused with a message wherever the call runs; then CPU
    tensors are, as everywhere else: there is no PyTorch path."""
    depth = torch.ones(2, 1, 4, 8)
    w = torch.ones(2, 2, 4, 8)
    rgb = torch.ones(2, 3, 4, 8)
    S = nconv_amd.smoothness_loss
    with pytest.raises(ValueError, match=r"depth must be \(B, 1, H, W\)"):
        S(depth[:, 0])
    with pytest.raises(TypeError, match="depth"):
        S(depth.double())
    with pytest.raises(ValueError, match="order must be 1"):
        S(depth, order=3)
    with pytest.raises(ValueError, match="weights must be"):
        S(depth, w[:, :1])
    with pytest.raises(TypeError, match="weights"):
        S(depth, w.double())
    with pytest.raises(ValueError, match="not contiguous"):
        S(depth, torch.ones(2, 2, 4, 16)[..., ::2])
    with pytest.raises(ValueError, match="weights requires a gradient"):
        S(depth, w.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="mask must be"):
        S(depth, mask=torch.ones(2, 1, 4, 7, dtype=torch.bool))
    with pytest.raises(TypeError, match="mask"):
        S(depth, mask=torch.ones(2, 1, 4, 8))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        S(depth, w)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.SmoothnessLoss(order=2)(depth)
    with pytest.raises(ValueError, match="order must be 1"):
        nconv_amd.SmoothnessLoss(order=0)
    E = nconv_amd.edge_weights
    with pytest.raises(ValueError, match="C = 1 or 3"):
        E(torch.ones(2, 2, 4, 8))
    with pytest.raises(TypeError, match="rgb"):
        E(rgb.to(torch.uint8))
    with pytest.raises(ValueError, match="unit-stride rows"):
        E(rgb.transpose(2, 3).contiguous().transpose(2, 3))
    with pytest.raises(ValueError, match="alpha"):
        E(rgb, alpha=-1.0)
    with pytest.raises(ValueError, match="alpha"):
        E(rgb, alpha=float("nan"))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        E(rgb)
    with pytest.raises(ValueError, match="alpha"):
        nconv_amd.EdgeWeights(alpha=float("inf"))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.EdgeWeights()({"rgb": rgb, "depth": depth})
    assert nconv_amd.smooth.workspace_bytes(2, 4, 8) == 8 + 2 * 16 + 2 * 8 + 2 * 16
    with pytest.raises(ValueError, match="too large"):
        nconv_amd.smooth.workspace_bytes(1 << 20, 64, 64)


# ------------------------------------------------------------------------------------------------
# the C boundary from a plain C host
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "smooth_host")


def test_host_descriptor_layouts_match_ctypes(nconv_amd, report):
    for struct, name in ((nconv_amd._lib.NconvSmoothLoss, "nconv_smooth_loss"),
                         (nconv_amd._lib.NconvEdgeWeights, "nconv_edge_weights")):
        want = host_harness.ctypes_layout(struct, name)
        assert {key: report[key] for key in want} == want
    assert report["abi"] == [27, 27]
    for name in ("nconv_smooth_loss_workspace_bytes", "nconv_smooth_loss_fwd", "nconv_smooth_loss_bwd",
                 "nconv_edge_weights"):
        assert name in nconv_amd._lib.EXPORTED


def test_host_workspace_sizes(report):
    small, full, zero_b, neg_w, odd = report["ws"]
    tiles = lambda B, H, W: B * ((H + 15) // 16) * ((W + 63) // 64)  # noqa: E731
    size = lambda B, H, W: 8 + 24 * B + 16 * tiles(B, H, W)  # noqa: E731
    assert (small, full, odd) == (size(2, 4, 8), size(8, 352, 1216), size(3, 17, 65))
    assert zero_b == 0 and neg_w == 0 and odd % 8 == 0


BOTH = ("fwd", "bwd")
ENTRY = {"fwd": "nconv_smooth_loss_fwd", "bwd": "nconv_smooth_loss_bwd", "edge": "nconv_edge_weights"}


@pytest.mark.parametrize("case,why,sides", [
    ("null_descriptor", "null descriptor", BOTH + ("edge",)),
    ("null_depth", "null depth", BOTH),
    ("order_0", "order must be 1 or 2", BOTH), ("order_3", "order must be 1 or 2", BOTH),
    ("order_negative", "order must be 1 or 2", BOTH),
    ("B_zero", "non-positive", BOTH + ("edge",)), ("H_negative", "non-positive", BOTH), ("W_zero", "non-positive", BOTH),
    ("batch_too_large", "batch too large", BOTH + ("edge",)),
    ("depth_misaligned", "not 4-byte aligned", BOTH), ("weights_misaligned", "not 4-byte aligned", BOTH + ("edge",)),
    ("depth_row_stride_short", "depth: row stride smaller than W", BOTH),
    ("depth_row_stride_negative", "depth: row stride smaller than W", BOTH),
    ("depth_image_stride_short", "depth: image stride smaller", BOTH),
    ("mask_row_stride_short", "mask: row stride smaller than W", BOTH),
    ("mask_image_stride_short", "mask: image stride smaller", BOTH),
    ("depth_plane_too_large", "depth: plane too large", BOTH), ("mask_plane_too_large", "mask: plane too large", BOTH),
    ("workspace_small", "workspace too small", BOTH), ("workspace_null", "workspace too small", BOTH),
    ("workspace_misaligned", "workspace not 8-byte aligned", BOTH),
    ("null_output", "null", BOTH), ("output_misaligned", "not 4-byte aligned", BOTH),
    ("g_depth_overlaps_depth", "g_depth overlaps depth", ("bwd",)),
    ("null_image", "null image or weights", ("edge",)), ("null_weights", "null image or weights", ("edge",)),
    ("C_2", "C must be 1 or 3", ("edge",)), ("C_0", "C must be 1 or 3", ("edge",)),
    ("W_negative", "non-positive", ("edge",)),
    ("alpha_negative", "alpha must be finite", ("edge",)), ("alpha_nan", "alpha must be finite", ("edge",)),
    ("alpha_infinite", "alpha must be finite", ("edge",)),
    ("image_misaligned", "not 4-byte aligned", ("edge",)),
    ("row_stride_short", "image: row stride smaller than W", ("edge",)),
    ("channel_stride_short", "image: channel stride smaller", ("edge",)),
    ("image_stride_short", "image: image stride too small", ("edge",)),
    ("stride_negative", "image: stride negative", ("edge",)),
    ("plane_too_large", "image: plane too large", ("edge",)),
    ("weights_overlap_image", "weights overlaps image", ("edge",))])
def test_host_refuses_bad_arguments(report, case, why, sides):
    for side in sides:
        rc, text = report[f"{side}_{case}"]
        assert rc == -22 and why in text and text.startswith(ENTRY[side] + ":"), (side, rc, text)
