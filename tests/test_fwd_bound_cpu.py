"""CPU checks of the element-wise forward criterion the GPU tests apply (tests/test_gpu_layers.py):
|got - ref| <= kappa * A + 1e-30 per element of y and cout, A the forward majorant of
nconv_cases.nconv2d_forward_majorant, kappa = 4 x kappa_ref of tests/golden/fwd_bound_kappa.json
(tools/fwd_kappa.py) by the rule of nconv_cases.kappa.

* the json holds a kappa for every case and output, and is what the tool computes now;
* the reference's own float32 run passes the criterion on every case, with room to spare;
* the majorant dominates the outputs it is derived from;
* four seeded defects of the kind a forward kernel can have, each inside the old
  1e-4 |ref| + 1e-5 bound, each fail the criterion;
* the expected-kernel rule and the channel-slice bands the GPU test copies are the source's.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import nconv_cases as NC
from oracle import nconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtime-depth-estimation-nconv_amd", "csrc")


@pytest.fixture(autouse=True)
def one_thread():
    """kappa_ref's last digits follow the float32 sums' order, and that follows the thread count:
    the tool and these checks run on one thread."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _cases():
    for c in NC.LAYER_CASES:
        yield "layer", c[0]
    for c in NC.PHASE_CASES:
        yield "phase", c[0]
    for e in NC.FWD_SLICE_CASES:
        yield "slice", e[2][0]


def test_kappa_json_is_complete_and_current():
    """A kappa for every case x output; three cases recomputed give the file's figures (4 digits,
    2 % of slack for another CPU's vector width in the float32 convolutions)."""
    K = NC.load_fwd_kappa()
    assert set(K["layer"]) == {c[0] for c in NC.LAYER_CASES}
    assert set(K["phase"]) == {c[0] for c in NC.PHASE_CASES}
    assert set(K["slice"]) == {e[2][0] for e in NC.FWD_SLICE_CASES}
    for kind, name in _cases():
        assert set(K[kind][name]) == set(NC.FWD_LABELS), (kind, name)
        assert all(0 < v < 1e-5 for v in K[kind][name].values()), (kind, name)
    for kind, name in (("layer", "down_pool_odd"), ("layer", "nconv1_thresh"), ("phase", "up_p1")):
        prob, ref, A = NC.fwd_budget(kind, name)
        for lab, v in prob.kappa_ref(ref, A).items():
            assert v == pytest.approx(K[kind][name][lab], rel=2e-2), (kind, name, lab)


@pytest.mark.parametrize("kind,name", list(_cases()), ids=lambda v: v)
def test_float32_reference_passes(kind, name):
    """The reference's float32 run is inside kappa on every element of both outputs: at a quarter
    of the bound where the json was written (kappa >= 4 kappa_ref: the cap of nconv_cases.kappa
    binds on no forward case), within half of it on a CPU whose float32 convolutions sum in
    another order. The comparison covers every element (asserted inside)."""
    prob, ref, A = NC.fwd_budget(kind, name)
    worst = NC.assert_outputs_elementwise(name, prob, prob.outputs(torch.float32), NC.load_fwd_kappa()[kind][name],
                                          "fp32", ref, A)
    assert set(worst) == set(NC.FWD_LABELS)
    assert all(v <= 0.5 for v in worst.values()), worst


@pytest.mark.parametrize("name", ["nconv2_plain", "generic_dil2_groups2", "nconv5_upcat_inexact", "nconv1_thresh"])
def test_majorant_dominates_outputs(name):
    """|y| <= A_y and |cout| <= A_c per element (A sums the magnitudes of the output's terms)."""
    prob, ref, A = NC.fwd_budget("layer", name)
    for lab, r, a in zip(NC.FWD_LABELS, ref, A):
        assert (r.abs() <= a * (1 + 1e-12) + 1e-300).all(), lab


# ------------------------------------------------------------------------------------------------
# seeded defects: the float64 oracle with one thing wrong
# ------------------------------------------------------------------------------------------------
def _parts(prob, w=None):
    """(x c, c, w, b, s) of the layer on the glued inputs, float64."""
    xa, ca, xb, cb, w0, b = prob.ops
    x, c = NC.glue(prob.mode, xa, ca, xb, cb)
    w = w0 if w is None else w
    return x * c, c, w, b.view(1, -1, 1, 1), w.reshape(w.shape[0], -1).sum(-1).view(1, -1, 1, 1)


def _defect_tap_scaled(prob):
    """One kernel tap (every channel pair of one position) is 1 + 2e-5 of itself in both sums; s is
    the true weights'."""
    xc, c, w, b, s = _parts(prob)
    w2 = w.clone()
    w2[:, :, 0, w.shape[3] - 1] *= 1 + 2e-5
    D = F.conv2d(c, w2, None, *prob.geom)
    return F.conv2d(xc, w2, None, *prob.geom) / (D + R.EPS) + b, D / s


def _defect_product_noise(prob):
    """Every product of both sums carries bf16x3's relative error (uniform in +-BF16X3_PER_PRODUCT):
    what a bf16x9 kernel that lost its low-order split terms computes."""
    xc, c, w, b, s = _parts(prob)
    stride, pad, dil, groups = prob.geom
    assert groups == 1
    g = torch.Generator().manual_seed(7)
    wf = w.reshape(w.shape[0], -1)                                   # (Cout, T)
    outs = []
    for src in (xc, c):
        cols = F.unfold(src, w.shape[2:], dil, pad, stride)          # (B, T, L)
        noise = (torch.rand(w.shape[0], *cols.shape, generator=g, dtype=torch.float64) * 2 - 1) * NC.BF16X3_PER_PRODUCT
        outs.append(torch.einsum("ot,btl,obtl->bol", wf, cols, 1 + noise))
    N, D = (t.reshape(xc.shape[0], w.shape[0], *NC.case_out_hw(_case(prob.name))) for t in outs)
    return N / (D + R.EPS) + b, D / s


def _defect_eps(prob):
    """eps = 2e-7 in place of 1e-7."""
    return prob.outputs(eps=2e-7)


def _case(name):
    return next(c for c in NC.LAYER_CASES if c[0] == name)


DEFECTS = {"tap_scaled": _defect_tap_scaled, "product_noise": _defect_product_noise, "eps": _defect_eps}
# The cases are those where the defect is larger than the reference's own float32 error, the only
# thing a budget measured from float32 can see. One tap of 25 x 8 at 1 + 2e-5 moves a full window's
# sums by 4e-7 of themselves, and noise of 1.1e-5 per product averages to ~6e-7 over 140 live
# products: both the size of kappa_ref there (5e-7), so for those two the cases are layers with few
# live taps per window (the sparse 1 -> 8 head, the 1x1 layer, 3x3 windows cut by the image corner).
# eps shows where D is small: the sparse head's windows holding one sample under a small weight.
DEFECT_CASES = [("nconv1_thresh", "tap_scaled"), ("nconv7_1x1_p2", "tap_scaled"), ("nconv4_upcat_exact", "tap_scaled"),
                ("nconv1_thresh", "product_noise"), ("generic_3x3_plain", "product_noise"),
                ("nconv4_upcat_exact", "product_noise"),
                ("nconv1_thresh", "eps"), ("nconv7_1x1_p2", "eps")]


def _old_bound_ok(ref, got):
    return all(((g - r).abs() <= 1e-4 * r.abs() + 1e-5).all() for r, g in zip(ref, got))


@pytest.mark.parametrize("name,defect", DEFECT_CASES)
def test_seeded_defect_is_caught(name, defect):
    """Each defect, applied to the float64 oracle, passes 1e-4 |ref| + 1e-5 on every element of both
    outputs and fails the element-wise budget under the exact-product (fp32 / bf16x9) kappa; the
    untouched oracle passes."""
    prob, ref, A = NC.fwd_budget("layer", name)
    kap = NC.load_fwd_kappa()["layer"][name]
    got = DEFECTS[defect](prob)
    assert _old_bound_ok(ref, got)
    for math in ("fp32", "bf16x9"):
        with pytest.raises(AssertionError, match=r"err / \(kappa A\)"):
            NC.assert_outputs_elementwise(f"{name} {defect}", prob, got, kap, math, ref, A)
    NC.assert_outputs_elementwise(name, prob, ref, kap, "fp32", ref, A)


@pytest.mark.parametrize("name", ["nconv2_plain", "nconv4_upcat_exact"])
def test_neighbour_normaliser_is_caught(name):
    """cout of output channel 1 divided by channel 0's s, on weights whose row sums differ by 1e-5
    (row 1 rescaled to s[0] (1 + 1e-5)): 1e-5 of cout, inside the old bound, outside the budget. The
    reference's float32 run on the same weights passes with the case's committed kappa."""
    base = NC.fwd_budget("layer", name)[0]
    w = base.ops[4].clone()
    s = w.reshape(w.shape[0], -1).sum(-1)
    w[1] *= s[0] * (1 + 1e-5) / s[1]
    prob = NC.FwdProblem(name, base.mode, base.ops[:4] + [NC.r32(w), base.ops[5]], base.geom)
    s = prob.ops[4].reshape(w.shape[0], -1).sum(-1)
    assert abs(float(s[1] / s[0]) - (1 + 1e-5)) < 1e-6
    ref, A = prob.outputs(), prob.majorant()
    kap = NC.load_fwd_kappa()["layer"][name]
    NC.assert_outputs_elementwise(name, prob, prob.outputs(torch.float32), kap, "fp32", ref, A)
    cout = ref[1].clone()
    cout[:, 1] *= s[1] / s[0]
    got = (ref[0], cout)
    assert _old_bound_ok(ref, got)
    with pytest.raises(AssertionError, match=r"cout \[fp32\]: err / \(kappa A\)"):
        NC.assert_outputs_elementwise(name, prob, got, kap, "fp32", ref, A)


def test_bf16x3_kappa_admits_its_product_noise():
    """The same per-product noise passes under the bf16x3 kappa (the addend is what it is for)."""
    name = "nconv4_upcat_exact"
    prob, ref, A = NC.fwd_budget("layer", name)
    NC.assert_outputs_elementwise(name, prob, _defect_product_noise(prob), NC.load_fwd_kappa()["layer"][name],
                                  "bf16x3", ref, A)


# ------------------------------------------------------------------------------------------------
# what the GPU tests copy from the source
# ------------------------------------------------------------------------------------------------
def test_slice_bands_are_the_dispatch_constants():
    """CS1_TILES / CS2_TILES are kCs1Tiles / kCs2Tiles of nconv_fwd.hip and tiles16 is go_tiled's
    expression: if the dispatch rule moves, the slice cases fail here instead of testing CS = 4
    three times."""
    with open(os.path.join(CSRC, "nconv_fwd.hip")) as fh:
        src = fh.read()
    m = re.search(r"constexpr long kCs1Tiles = (\d+), kCs2Tiles = (\d+);", src)
    assert m, "kCs1Tiles / kCs2Tiles not found as written"
    assert (int(m.group(1)), int(m.group(2))) == (NC.CS1_TILES, NC.CS2_TILES)
    assert "int cs = tiles16 >= kCs1Tiles ? 1 : tiles16 >= kCs2Tiles ? 2 : 4;" in src
    assert "const long tiles16 = (long)((gw + 31) / 32) * ((gh + 15) / 16) * d.L.B;" in src
    # the smallest shapes of each band: exactly on its lower edge, and the layer cases all below
    for cs, batch, case in NC.FWD_SLICE_CASES:
        assert NC.tiles16(batch, *NC.case_out_hw(case)) == {1: NC.CS1_TILES, 2: NC.CS2_TILES}[cs], case[0]
        assert NC.case_out_hw(case) == (241, 481)
    assert all(NC.tiles16(2, *NC.case_out_hw(c)) < NC.CS2_TILES for c in NC.LAYER_CASES)
    assert all(NC.tiles16(3, *NC.case_out_hw((c[0], c[1], 16, 8, 3, c[2], 1, 1, 1, c[3], c[4]))) < NC.CS2_TILES
               for c in NC.PHASE_CASES)


def test_expected_fwd_kernel_rule():
    """The expectation the GPU test asserts nconv_plan against, spelled out for the layer cases."""
    mfma = {"nconv2_plain", "down_pool_odd", "down_pool_even", "down_pool_ties", "nconv4_upcat_exact",
            "nconv5_upcat_inexact", "nconv6_upfirst_p0", "nconv2_w4", "nconv5_upcat_w4", "nconv6_upfirst_w4",
            "nconv2_h1", "nconv2_h2", "down_pool_h5", "nconv2_tile_plus1", "nconv4_upcat_tile_plus1"}
    tiled_only = {"nconv1_thresh", "nconv7_1x1_p2"}
    for c in NC.LAYER_CASES:
        for math in ("fp32", "bf16x3", "bf16x9"):
            if c[0] in mfma:
                want = "tiled_fp32" if math == "fp32" else "mfma_" + math
            else:
                want = "tiled_fp32" if c[0] in tiled_only else "generic"
            assert NC.expected_fwd_kernel(c, math) == want, (c[0], math)
    assert {c[0] for c in NC.LAYER_CASES} - mfma - tiled_only == {
        "generic_3x3_plain", "generic_stride2", "generic_dil2_groups2", "generic_pool_c3"}
