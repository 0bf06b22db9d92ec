"""CPU checks of the element-wise gradient criterion the GPU tests apply (tests/test_gpu_layers.py,
tests/test_gpu_dense_train.py): |got - ref| <= kappa * A + 1e-30 per element, A the gradient
majorant of nconv_cases.nconv2d_backward_majorant, kappa = 4 x kappa_ref of
tests/golden/bwd_bound_kappa.json (tools/bwd_kappa.py).

* the json is what the tool computes now;
* the reference's own float32 run passes the criterion on every case;
* the majorant dominates every term of the closed form it is derived from;
* four seeded defects of the kind a tiled backward can have, each far inside the old normwise
  1e-3 bound, each fail the criterion;
* the dense cases' seeds keep every ReLU pre-activation clear of the forward bound.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import dense_cases as DC
import nconv_cases as NC
from oracle import nconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def one_thread():
    """kappa_ref's last digits follow the float32 sums' order, and that follows the thread count:
    the tool and these checks run on one thread."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bwd_kappa
    finally:
        sys.path.pop(0)
    return bwd_kappa


def test_kappa_json_is_current():
    """Two layer cases, the phase cases and the dense cases recomputed: the file's figures (4
    digits). 2 % of slack for another CPU's vector width in the float32 convolutions."""
    K = NC.load_kappa()
    assert set(K["layer"]) == {c[0] for c in NC.LAYER_CASES}
    assert set(K["phase"]) == {c[0] for c in NC.PHASE_CASES}
    assert set(K["module"]) == {f"{H}x{W}" for H, W in NC.MODULE_SIZES}
    assert set(K["dense"]) == {DC.case_id(c) for c in DC.CASES}
    now = {"layer": {n: NC.layer_bwd_problem(next(c for c in NC.LAYER_CASES if c[0] == n)).kappa_ref()
                     for n in ("down_pool_odd", "nconv4_upcat_exact")},
           "dense": {DC.case_id(c): DC.DenseProblem(c).kappa_ref() for c in DC.CASES[:2]}}
    for sec, cases in now.items():
        for name, d in cases.items():
            assert set(d) == set(K[sec][name]), (sec, name)
            for lab, v in d.items():
                assert v == pytest.approx(K[sec][name][lab], rel=2e-2), (sec, name, lab)


def _problems():
    for c in NC.LAYER_CASES:
        yield "layer", c[0]
    for c in NC.PHASE_CASES:
        yield "phase", c[0]


@pytest.mark.parametrize("kind,name", list(_problems()), ids=lambda v: v)
def test_float32_reference_passes(kind, name):
    """The reference's float32 run is inside kappa = 4 x kappa_ref on every element of every
    gradient, and the comparison covers every element (asserted inside)."""
    prob, refs, A = NC.budget(kind, name)
    worst = NC.assert_gradients_elementwise(name, prob, prob.grads(torch.float32), NC.load_kappa()[kind][name],
                                            "fp32", refs, A)
    assert set(worst) == {lab for lab, r in zip(NC.GRAD_LABELS, refs) if r is not None}


@pytest.mark.parametrize("H,W", NC.MODULE_SIZES[:1])
def test_float32_reference_passes_module(H, W):
    w, b = NC.module_init_weights()
    prob = NC.module_bwd_problem(H, W, w, b)
    NC.assert_gradients_elementwise(prob.name, prob, prob.grads(torch.float32), NC.load_kappa()["module"][f"{H}x{W}"])


@pytest.mark.parametrize("name", ["nconv2_plain", "generic_dil2_groups2", "generic_stride2"])
def test_majorant_dominates_closed_form(name):
    """|g| <= A per element for the float64 gradients (A sums the magnitudes of g's terms), for the
    closed form's dilation / groups extension too; and the oracle's own closed form agrees with
    autograd where it is defined (no dilation, one group)."""
    prob, refs, A = NC.budget("layer", name)
    for lab, r, a in zip(NC.GRAD_LABELS, refs, A):
        if r is not None:
            assert (r.abs() <= a * (1 + 1e-12) + 1e-300).all(), lab
    if name == "nconv2_plain":
        xa, ca, _, _, w, b = prob.ops
        cf = R.nconv2d_backward(xa, ca, w, b, prob.gy, prob.gc, prob.geom[0], prob.geom[1])
        for r, g in zip((refs[0], refs[1], refs[4], refs[5]), cf):
            torch.testing.assert_close(g, r, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# seeded defects
# ------------------------------------------------------------------------------------------------
def _closed_form_parts(prob):
    """(x, c, gN, gD) of the closed form on the glued inputs, float64."""
    xa, ca, xb, cb, w, b = prob.ops
    x, c = NC.glue(prob.mode, xa, ca, xb, cb)
    D = F.conv2d(c, w, None, *prob.geom)
    N = F.conv2d(x * c, w, None, *prob.geom)
    s = w.reshape(w.shape[0], -1).sum(-1).view(1, -1, 1, 1)
    gN = prob.gy / (D + R.EPS)
    gD = -prob.gy * N / (D + R.EPS) ** 2 + prob.gc / s
    return x, c, gN, gD


def _input_delta(prob, wmask, omask):
    """What the taps wmask (a 0/1 tensor like w) of the output pixels omask (like gy) contribute to
    the six gradients' input part, through the glue's adjoint."""
    from torch.nn.grad import conv2d_input
    xa, ca, xb, cb, w, b = prob.ops
    x, c, gN, gD = _closed_form_parts(prob)
    gxc = conv2d_input(x.shape, w * wmask, gN * omask, *prob.geom)
    gcc = conv2d_input(x.shape, w * wmask, gD * omask, *prob.geom)
    return list(NC.glue_adjoint(prob.mode, xa, ca, xb, cb, gxc * c, gcc + gxc * x)) + [None, None]


def _defect_tap_at_column0(prob, refs):
    """(i) the centre tap's contribution of the output-column-0 pixels of one row is missing."""
    w = prob.ops[4]
    wmask = torch.zeros_like(w)
    wmask[:, :, w.shape[2] // 2, w.shape[3] // 2] = 1
    omask = torch.zeros_like(prob.gy)
    omask[:, :, min(3, omask.shape[2] - 1), 0] = 1
    return [None if d is None else -d for d in _input_delta(prob, wmask, omask)]


def _defect_tap_scaled(prob, refs):
    """(ii) one weight tap is 1 + 1e-3 of itself in the input gradient."""
    w = prob.ops[4]
    wmask = torch.zeros_like(w)
    wmask[:, :, 0, w.shape[3] - 1] = 1
    return [None if d is None else 1e-3 * d for d in _input_delta(prob, wmask, torch.ones_like(prob.gy))]


def _defect_wrong_slot(prob, refs):
    """(iii) one window's gradient lands in the neighbouring slot: the pooled gradient of one 2x2
    window beside its argmax, or (nearest upsample) one child's share in the neighbouring parent."""
    d = [None] * 6
    if prob.mode == NC.POOL2:
        g = refs[0]
        nz = g[0, 0].nonzero()
        i, j = (int(v) for v in nz[len(nz) // 2])
        d[0] = torch.zeros_like(g)
        d[0][0, 0, i, j] = -g[0, 0, i, j]
        d[0][0, 0, i, j ^ 1] = g[0, 0, i, j]
    else:
        g = refs[2]  # g_xb: each low pixel sums its four children
        nz = g[0, 0].nonzero()
        i, j = (int(v) for v in nz[len(nz) // 2])
        share = g[0, 0, i, j] / 4
        d[2] = torch.zeros_like(g)
        d[2][0, 0, i, j] = -share
        d[2][0, 0, i, j ^ 1] = share
    return d


def _defect_last_row_wgrad(prob, refs):
    """(iv) the last output row's contribution is missing from g_w."""
    from torch.nn.grad import conv2d_weight
    x, c, gN, gD = _closed_form_parts(prob)
    w = prob.ops[4]
    last = torch.zeros_like(gN)
    last[:, :, -1, :] = 1
    dw = conv2d_weight(x * c, w.shape, gN * last, *prob.geom) + conv2d_weight(c, w.shape, gD * last, *prob.geom)
    return [None, None, None, None, -dw, None]


DEFECTS = {"tap_at_column0": _defect_tap_at_column0, "tap_scaled": _defect_tap_scaled,
           "wrong_slot": _defect_wrong_slot, "last_row_wgrad": _defect_last_row_wgrad}
DEFECT_CASES = [(n, d) for n in ("nconv2_plain", "down_pool_odd", "nconv4_upcat_exact") for d in DEFECTS
                if not (n == "nconv2_plain" and d == "wrong_slot")]  # a plain layer has no slots


def _normwise_ok(refs, got):
    return all(((g - r).abs().max() / r.abs().max().clamp_min(1e-30)).item() <= 1e-3
               for r, g in zip(refs, got) if r is not None)


@pytest.mark.parametrize("name,defect", DEFECT_CASES)
def test_seeded_defect_is_caught(name, defect):
    """Each defect, applied to the float64 reference's gradients, passes the old normwise 1e-3 check
    (shrunk by halving until it does: the reason the element-wise criterion exists) and fails the
    element-wise one."""
    prob, refs, A = NC.budget("layer", name)
    delta = DEFECTS[defect](prob, refs)
    assert any(d is not None and d.abs().max() > 0 for d in delta)
    scale = 1.0
    apply = lambda: [None if r is None else (r if d is None else r + scale * d) for r, d in zip(refs, delta)]
    while not _normwise_ok(refs, apply()):
        scale /= 2
        assert scale > 2.0 ** -20
    got = apply()
    assert _normwise_ok(refs, got)
    print(f"{name} {defect}: defect scaled by {scale:g} passes 1e-3 normwise")
    with pytest.raises(AssertionError, match=r"err / \(kappa A\)"):
        NC.assert_gradients_elementwise(name, prob, got, NC.load_kappa()["layer"][name], "fp32", refs, A)
    # the untouched reference passes
    NC.assert_gradients_elementwise(name, prob, refs, NC.load_kappa()["layer"][name], "fp32", refs, A)


# ------------------------------------------------------------------------------------------------
# dense cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_dense_case_budget(case):
    """The seeds keep every ReLU pre-activation of the float64 reference outside the forward bound
    1e-6 * (|x| (*) |w| + |b|) (so the reference's mask is the one a correct forward takes); the
    float32 reference's weight / bias gradients pass kappa = 4 x kappa_ref; the input-gradient
    majorant is the adjoint of the forward's."""
    prob = DC.DenseProblem(case)
    assert prob.relu_margin_violations() == 0
    pre, _, ref = prob.run()
    _, _, g32 = prob.run(torch.float32)
    mask = (pre > 0) if prob.relu else torch.ones_like(pre, dtype=torch.bool)
    A = prob.majorants(mask)
    kap = NC.load_kappa()["dense"][DC.case_id(case)]
    for lab, r, g, a in zip(("g_x0", "g_x1", "g_w", "g_b"), ref, g32, A):
        if r is None:
            continue
        assert (r.abs() <= a * (1 + 1e-12)).all(), lab
        if lab in kap:
            ratio, _, n = NC.elementwise_excess(g, r, a, 4 * kap[lab])
            assert n == r.numel() and ratio <= 1, (lab, ratio)
