"""Shared input builders and the oracle-side layer (glue + nconv2d) for the parity tests."""
import functools

import torch
import torch.nn.functional as F

from oracle import nconv_ref as R

PLAIN, THRESH, POOL2, UPCAT_SKIP_FIRST, UPCAT_UP_FIRST = 0, 1, 2, 3, 4


def glue(mode, xa, ca, xb, cb, thresh=0.01):
    """The reference's glue op in front of a layer: (x, c) as NConv2d.forward receives them."""
    if mode == THRESH:
        return xa, (xa > thresh).to(xa.dtype)
    if mode == PLAIN:
        return xa, ca
    if mode == POOL2:
        return F.max_pool2d(xa, 2, 2), F.max_pool2d(ca, 2, 2)
    up = lambda t: F.interpolate(t, xa.shape[2:], mode="nearest")
    if mode == UPCAT_SKIP_FIRST:
        return torch.cat((xa, up(xb)), 1), torch.cat((ca, up(cb)), 1)
    return torch.cat((up(xb), xa), 1), torch.cat((up(cb), ca), 1)


def oracle_layer(mode, xa, ca, xb, cb, w, b, stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1, thresh=0.01):
    """The reference's glue op followed by NConv2d.forward, on whatever device/dtype given."""
    x, c = glue(mode, xa, ca, xb, cb, thresh)
    return R.nconv2d(x, c, w, b, stride, pad, dil, groups)


def rand_pair(g, B, C, H, W, dtype=torch.float32, density=0.7):
    """data U(0,10); confidence 0 with prob 1-density, else U(0.05, 1)."""
    x = torch.rand(B, C, H, W, generator=g, dtype=dtype) * 10
    keep = torch.rand(B, C, H, W, generator=g, dtype=dtype) < density
    c = (torch.rand(B, C, H, W, generator=g, dtype=dtype) * 0.95 + 0.05) * keep
    return x, c


def rand_weight(g, cout, cin, kh, kw, dtype=torch.float32):
    """Positive weights like a trained (softplus'd) NConv layer."""
    return torch.rand(cout, cin, kh, kw, generator=g, dtype=dtype) + 0.05


# (name, mode, cin, cout, k, pad, stride, dil, groups, a-shape, b-shape) — a/b shapes (C, H, W)
LAYER_CASES = [
    ("nconv1_thresh", THRESH, 1, 8, 5, 2, 1, 1, 1, (1, 37, 70), None),
    ("nconv2_plain", PLAIN, 8, 8, 5, 2, 1, 1, 1, (8, 37, 70), None),
    ("down_pool_odd", POOL2, 8, 8, 5, 2, 1, 1, 1, (8, 37, 71), None),
    ("down_pool_even", POOL2, 8, 8, 5, 2, 1, 1, 1, (8, 48, 130), None),
    ("down_pool_ties", POOL2, 8, 8, 5, 2, 1, 1, 1, (8, 30, 66), None),  # integer data: exact ties
    ("nconv4_upcat_exact", UPCAT_SKIP_FIRST, 16, 8, 3, 1, 1, 1, 1, (8, 24, 70), (8, 12, 35)),
    ("nconv5_upcat_inexact", UPCAT_SKIP_FIRST, 16, 8, 3, 1, 1, 1, 1, (8, 25, 71), (8, 12, 35)),
    ("nconv6_upfirst_p0", UPCAT_UP_FIRST, 16, 8, 3, 0, 1, 1, 1, (8, 37, 70), (8, 18, 35)),
    ("nconv7_1x1_p2", PLAIN, 8, 1, 1, 2, 1, 1, 1, (8, 35, 68), None),
    # widths a multiple of 4: the 16-byte store (and LDS-DMA staging) paths of the MFMA kernels
    ("nconv2_w4", PLAIN, 8, 8, 5, 2, 1, 1, 1, (8, 21, 68), None),
    ("nconv5_upcat_w4", UPCAT_SKIP_FIRST, 16, 8, 3, 1, 1, 1, 1, (8, 26, 72), (8, 13, 36)),
    ("nconv6_upfirst_w4", UPCAT_UP_FIRST, 16, 8, 3, 0, 1, 1, 1, (8, 34, 72), (8, 17, 36)),
    # 1, 2 and 5 output rows: the row-pair weight gradient's single-row / lone-pair segments
    ("nconv2_h1", PLAIN, 8, 8, 5, 2, 1, 1, 1, (8, 1, 70), None),
    ("nconv2_h2", PLAIN, 8, 8, 5, 2, 1, 1, 1, (8, 2, 40), None),
    ("down_pool_h5", POOL2, 8, 8, 5, 2, 1, 1, 1, (8, 10, 33), None),
    ("generic_3x3_plain", PLAIN, 8, 8, 3, 1, 1, 1, 1, (8, 29, 41), None),
    ("generic_stride2", PLAIN, 4, 6, 3, 1, 2, 1, 1, (4, 29, 41), None),
    ("generic_dil2_groups2", PLAIN, 4, 6, 3, 2, 1, 2, 2, (4, 29, 41), None),
    ("generic_pool_c3", POOL2, 3, 5, 5, 2, 1, 1, 1, (3, 21, 30), None),
    # one row and one column past a 16x32 tile; the exactly-2x UpCat likewise (low side 17x33)
    ("nconv2_tile_plus1", PLAIN, 8, 8, 5, 2, 1, 1, 1, (8, 33, 65), None),
    ("nconv4_upcat_tile_plus1", UPCAT_SKIP_FIRST, 16, 8, 3, 1, 1, 1, 1, (8, 34, 66), (8, 17, 33)),
]


def r32(t):
    """float64 tensor holding the fp32 rounding of t: the operand the GPU sees."""
    return None if t is None else t.float().double()


def build_case(case, seed, batch=2):
    """float64 operands (xa, ca, xb, cb, w, b) of a LAYER_CASES entry at batch 2 (or `batch`)."""
    name, mode, cin, cout, k, pad, stride, dil, groups, a_shape, b_shape = case
    g = torch.Generator().manual_seed(seed)
    xa, ca = rand_pair(g, batch, *a_shape, dtype=torch.float64)
    if mode == THRESH:
        xa = xa * (torch.rand(xa.shape, generator=g, dtype=torch.float64) < 0.3)
        ca = None
    if name.endswith("_ties"):  # small integer values and a 3-level confidence: many exact ties
        xa = torch.randint(0, 3, xa.shape, generator=g).double()
        ca = torch.randint(0, 3, ca.shape, generator=g).double() * 0.5
    xb = cb = None
    if b_shape is not None:
        xb, cb = rand_pair(g, batch, *b_shape, dtype=torch.float64)
    w = rand_weight(g, cout, cin // groups, k, k, torch.float64)
    b = torch.rand(cout, generator=g, dtype=torch.float64) * 0.1
    return xa, ca, xb, cb, w, b


# Exact-2x UPCAT layers on the phase path (nconv_layer.wphase, nconv_fwd_phase.hip): both channel
# orders, paddings 0 / 1 / 2 (both phase parities), ragged widths, tiles cut by the image edge.
# (name, mode, pad, a-shape, b-shape)
PHASE_CASES = [
    ("skip_p1", 3, 1, (8, 24, 70), (8, 12, 35)),
    ("skip_p1_w4", 3, 1, (8, 26, 72), (8, 13, 36)),
    ("skip_p0", 3, 0, (8, 20, 64), (8, 10, 32)),
    ("skip_p2", 3, 2, (8, 18, 46), (8, 9, 23)),
    ("up_p0", 4, 0, (8, 34, 72), (8, 17, 36)),
    ("up_p1", 4, 1, (8, 36, 66), (8, 18, 33)),
]


# The channel-slice variants of the tiled exact-fp32 forward (nconv_fwd.hip go_tiled: fwd_tiled<..., CS>,
# CS output-channel slices per tile). CS follows tiles16 = ceil(Wo / 32) * ceil(Ho / 16) * B:
# CS = 1 from CS1_TILES, CS = 2 from CS2_TILES, CS = 4 below (test_fwd_bound_cpu pins the two
# constants to the source). Forward only, exact fp32; not in LAYER_CASES, so the backward matrix
# does not grow. The smallest shapes that reach each variant: 16 x 16 output tiles (241 x 481, one
# row and one column past the 15th tile) at batch 2 (512 tiles) and batch 4 (1024 tiles).
# CS = 4 needs no shapes of its own: every LAYER_CASES entry has a few dozen tiles. The 8 -> 1 1x1
# layer (nconv7) and the THRESH layer always run CS = 1 (go_tiled) and are LAYER_CASES entries.
# (cs, batch, LAYER_CASES-style entry)
CS2_TILES, CS1_TILES = 512, 1024
_SLICE_LAYERS = [
    ("plain", PLAIN, 8, 8, 5, 2, 1, 1, 1, (8, 241, 481), None),
    ("pool", POOL2, 8, 8, 5, 2, 1, 1, 1, (8, 482, 962), None),
    ("upcat_skip", UPCAT_SKIP_FIRST, 16, 8, 3, 1, 1, 1, 1, (8, 241, 481), (8, 120, 240)),
    ("upcat_up", UPCAT_UP_FIRST, 16, 8, 3, 1, 1, 1, 1, (8, 241, 481), (8, 120, 240)),
]
FWD_SLICE_CASES = [(cs, batch, (f"cs{cs}_{c[0]}",) + c[1:]) for cs, batch in ((2, 2), (1, 4)) for c in _SLICE_LAYERS]


def case_out_hw(case):
    """Output (Ho, Wo) of a LAYER_CASES-style entry."""
    _, mode, _, _, k, pad, stride, dil, _, a_shape, _ = case
    H, W = (a_shape[1] // 2, a_shape[2] // 2) if mode == POOL2 else a_shape[1:]
    return tuple((n + 2 * pad - dil * (k - 1) - 1) // stride + 1 for n in (H, W))


def tiles16(batch, Ho, Wo):
    """go_tiled's tile count: 16-row, 32-column output tiles over the batch."""
    return ((Wo + 31) // 32) * ((Ho + 15) // 16) * batch


def expected_fwd_kernel(case, fwd_math):
    """The forward kernel family nconv_plan must name for a LAYER_CASES-style entry launched without
    phase weights, from the case alone (nconv_fwd.hip plan_fwd restated; never calls the library):
    the matrix-core kernels under bf16x3 / bf16x9 for Cout 8, square kernel, stride 1, dilation 1,
    groups 1 and 8 -> 8 5x5 PLAIN / POOL2 or 16 -> 8 3x3 UPCAT; else the tiled exact-fp32 kernel
    for the DNET shapes; else the generic one."""
    _, mode, cin, cout, k, _, stride, dil, groups, *_ = case
    simple = stride == 1 and dil == 1 and groups == 1
    shape = (cin, cout, k)
    conv8 = shape == (8, 8, 5) and mode in (PLAIN, POOL2)
    upcat = shape == (16, 8, 3) and mode in (UPCAT_SKIP_FIRST, UPCAT_UP_FIRST)
    if simple and fwd_math in ("bf16x3", "bf16x9") and (conv8 or upcat):
        return "mfma_" + fwd_math
    head = shape == (1, 8, 5) and mode == THRESH
    last = shape == (8, 1, 1) and mode == PLAIN
    return "tiled_fp32" if simple and (conv8 or upcat or head or last) else "generic"


# ------------------------------------------------------------------------------------------------
# The element-wise gradient criterion: |got - ref| <= kappa * A + 1e-30 per element, ref the float64
# oracle on fp32-rounded operands, A the majorant below, kappa from tests/golden/bwd_bound_kappa.json
# (tools/bwd_kappa.py: the reference's own float32 run measured against the same float64 oracle).
# ------------------------------------------------------------------------------------------------
GRAD_LABELS = ("g_xa", "g_ca", "g_xb", "g_cb", "g_w", "g_b")
KAPPA_FLOOR = 2.0 ** -22
BF16X3_PER_PRODUCT = 1.1e-5  # include/nconv.h, NCONV_MATH_BF16X3
TILE = (16, 32)              # output tile of the tiled kernels (rows, columns)


def nconv2d_backward_majorant(x, c, w, b, gy, gcout, stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1, eps=R.EPS):
    """The closed form of oracle.nconv_ref.nconv2d_backward (here with dilation and groups) in float64,
    every factor replaced by its absolute value and every subtraction by an addition: per element
    the sum of the magnitudes of the terms a gradient is made of, so kappa * A is what a backward
    with relative error kappa per term may be off by.

        MN   = |gy| / (D+eps)
        MD   = |gy| (|y| + |b|) / (D+eps) + |gcout| / s
        A_xc = |W|^T (*) MN              A_x = A_xc |c|        A_c = A_xc |x| + |W|^T (*) MD
        A_w  = wgrad(|x c|, MN) + wgrad(|c|, MD) + sum |gcout| D / s^2          A_b = sum |gy|

    MD carries |y| + |b| rather than |N| / (D+eps): the backward recovers N / (D+eps) as y - b from
    the saved fp32 output, and that cancellation's rounding, relative to |y| and |b|,
    belongs in the budget. Returns (A_x, A_c, A_w, A_b) for the glued inputs x, c."""
    from torch.nn.grad import conv2d_input, conv2d_weight
    assert x.dtype == torch.float64
    geo = (stride, pad, dil, groups)
    aw, ab = w.abs(), b.abs().view(1, -1, 1, 1)
    D = F.conv2d(c, w, None, *geo)
    y = F.conv2d(x * c, w, None, *geo) / (D + eps) + b.view(1, -1, 1, 1)
    s = w.reshape(w.shape[0], -1).sum(-1).view(1, -1, 1, 1)
    inv = 1 / (D + eps).abs()
    MN = gy.abs() * inv
    MD = gy.abs() * (y.abs() + ab) * inv + gcout.abs() / s.abs()
    A_xc = conv2d_input(x.shape, aw, MN, *geo)
    A_x = A_xc * c.abs()
    A_c = A_xc * x.abs() + conv2d_input(c.shape, aw, MD, *geo)
    A_w = conv2d_weight((x * c).abs(), w.shape, MN, *geo) + conv2d_weight(c.abs(), w.shape, MD, *geo)
    A_w = A_w + (gcout.abs() * D.abs() / s ** 2).sum((0, 2, 3)).view(-1, 1, 1, 1)
    return A_x, A_c, A_w, gy.abs().sum((0, 2, 3))


def glue_adjoint(mode, xa, ca, xb, cb, t_x, t_c, thresh=0.01):
    """The glue's adjoint applied to (t_x, t_c), tensors shaped like the glued x and c: the max-pool
    scatters to its first-maximum argmax, the nearest upsample sums each low pixel's children, the
    concat splits. It is linear with 0 / 1 coefficients, so it carries gradients and majorants
    alike. Returns (for xa, ca, xb, cb), None where the layer has no such input."""
    if mode == PLAIN:
        return t_x, t_c, None, None
    if mode == THRESH:
        return t_x, None, None, None
    ins = [t.detach().clone().requires_grad_(True) if t is not None else None for t in (xa, ca, xb, cb)]
    x, c = glue(mode, *ins, thresh)
    live = [t for t in ins if t is not None]
    got = iter(torch.autograd.grad([x, c], live, [t_x, t_c]))
    return tuple(next(got) if t is not None else None for t in ins)


class BwdProblem:
    """One layer-backward comparison: fp32-rounded float64 operands, output gradients, geometry."""

    def __init__(self, name, mode, ops, gy, gc, geom):
        self.name, self.mode, self.ops, self.gy, self.gc, self.geom = name, mode, list(ops), gy, gc, geom
        self.cin_g, self.k = ops[4].shape[1], ops[4].shape[2]

    def grads(self, dtype=torch.float64):
        """Autograd of the oracle's own op sequence in dtype; the six gradients as float64."""
        leaves = [t.to(dtype).clone().requires_grad_(True) if t is not None else None for t in self.ops]
        ry, rc = oracle_layer(self.mode, *leaves, *self.geom)
        (ry * self.gy.to(dtype) + rc * self.gc.to(dtype)).sum().backward()
        return [None if t is None or t.grad is None else t.grad.double() for t in leaves]

    def majorant(self):
        xa, ca, xb, cb, w, b = self.ops
        with torch.no_grad():
            x, c = glue(self.mode, xa, ca, xb, cb)
            A_x, A_c, A_w, A_b = nconv2d_backward_majorant(x, c, w, b, self.gy, self.gc, *self.geom)
        return list(glue_adjoint(self.mode, xa, ca, xb, cb, A_x, A_c)) + [A_w, A_b]

    def kappa_ref(self):
        """Per tensor max_i |err_i| / A_i of the oracle's float32 run against its float64 run."""
        ref, f32, A = self.grads(), self.grads(torch.float32), self.majorant()
        return {lab: float(((g - r).abs() / (a + 1e-30)).max())
                for lab, r, g, a in zip(GRAD_LABELS, ref, f32, A) if r is not None}


def _outputs_like(p_ops, mode, geom):
    with torch.no_grad():
        return oracle_layer(mode, *p_ops, *geom)


def layer_bwd_problem(case):
    """test_layer_backward's operands (seed 4321, output gradients from seed 99), fp32-rounded."""
    name, mode, cin, cout, k, pad, stride, dil, groups, *_ = case
    ops = [r32(t) for t in build_case(case, 4321)]
    geom = ((stride, stride), (pad, pad), (dil, dil), groups)
    ry, rc = _outputs_like(ops, mode, geom)
    g = torch.Generator().manual_seed(99)
    gy = r32(torch.randn(ry.shape, generator=g, dtype=torch.float64))
    gc = r32(torch.randn(rc.shape, generator=g, dtype=torch.float64))
    return BwdProblem(name, mode, ops, gy, gc, geom)


def phase_bwd_problem(case):
    """test_upcat_phase_backward's operands (one generator, seed 23), fp32-rounded."""
    name, mode, pad, a_shape, b_shape = case
    g = torch.Generator().manual_seed(23)
    xa, ca = rand_pair(g, 2, *a_shape, dtype=torch.float64)
    xb, cb = rand_pair(g, 2, *b_shape, dtype=torch.float64)
    w = rand_weight(g, 8, 16, 3, 3, torch.float64)
    b = torch.rand(8, generator=g, dtype=torch.float64) * 0.1
    ops = [r32(t) for t in (xa, ca, xb, cb, w, b)]
    geom = ((1, 1), (pad, pad), (1, 1), 1)
    ry, rc = _outputs_like(ops, mode, geom)
    gy = r32(torch.randn(ry.shape, generator=g, dtype=torch.float64))
    gc = r32(torch.randn(rc.shape, generator=g, dtype=torch.float64))
    return BwdProblem(name, mode, ops, gy, gc, geom)


MODULE_SIZES = [(30, 44), (262, 70)]  # 262 rows: the two-row 5x5 weight gradient


def module_inputs(H, W):
    """test_nconv2d_module_train_step's data, confidence and output gradient (float64, unrounded)."""
    g = torch.Generator().manual_seed(5)
    x, c = rand_pair(g, 2, 8, H, W, dtype=torch.float64)
    gy = torch.randn(2, 8, H, W, generator=g, dtype=torch.float64)
    return x, c, gy


def module_bwd_problem(H, W, w, b):
    """The standalone NConv2d 8 -> 8 5x5 p2 training step, loss sum(y * gy + cout): w, b are the
    weights and bias the layer ran with (EnforcePos applied)."""
    x, c, gy = module_inputs(H, W)
    ops = [r32(t) for t in (x, c, None, None, w.double(), b.double())]
    gy = r32(gy)
    return BwdProblem(f"module_{H}x{W}", PLAIN, ops, gy, torch.ones_like(gy), ((1, 1), (2, 2), (1, 1), 1))


def module_init_weights():
    """The weight and bias of NConv2d(8, 8, (5, 5), "softplus", "p") under torch.manual_seed(3) with
    its EnforcePos hook applied, in fp32 on the CPU (the parameters the module test starts from)."""
    import nconv_pkg
    m = nconv_pkg.load()
    torch.manual_seed(3)
    layer = m.NConv2d(8, 8, (5, 5), "softplus", "p", padding=(2, 2))
    return R.softplus_pos(layer.weight.detach()), layer.bias.detach().clone()


@functools.lru_cache(maxsize=None)
def budget(kind, name):
    """(problem, float64 gradients, majorant) of a LAYER_CASES ("layer") or PHASE_CASES ("phase")
    entry, computed once and shared (read-only) by the tests that need it."""
    if kind == "layer":
        prob = layer_bwd_problem(next(c for c in LAYER_CASES if c[0] == name))
    else:
        prob = phase_bwd_problem(next(c for c in PHASE_CASES if c[0] == name))
    return prob, prob.grads(), prob.majorant()


def kappa(label, kref, cin_g, k, bwd_math="fp32"):
    """The bound's kappa from the reference's own kappa_ref: 4x for another summation order (box,
    phase and row-pair regroupings, fixed-order partial trees) and the cout * s / y - b recoveries.
    Input gradients: floored at 2^-22 (a lucky reference run sets no impossible bar) and capped at
    the a-priori dot-product bound (Cin/groups * K^2 + 8) * 2^-24. Weight and bias gradients sum
    over every pixel of the batch and have no useful a-priori cap. bf16x3 adds its per-product
    bound."""
    kap = 4 * kref
    if label not in ("g_w", "g_b"):
        kap = min(max(kap, KAPPA_FLOOR), (cin_g * k * k + 8) * 2.0 ** -24)
    return kap + (BF16X3_PER_PRODUCT if bwd_math == "bf16x3" else 0.0)


def elementwise_excess(got, ref, A, kap):
    """(worst err / (kappa A + 1e-30), its index, elements compared) of the criterion."""
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    ratio = (got - ref).abs() / (kap * A + 1e-30)
    finite = torch.isfinite(ratio)
    worst = int(torch.where(finite, ratio, torch.full_like(ratio, float("inf"))).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape))
    return float(ratio.flatten()[worst]), idx, int(finite.sum())


def assert_gradients_elementwise(what, problem, got, kappas, bwd_math="fp32", ref=None, A=None):
    """The element-wise criterion on the six gradients. got: float64 CPU tensors (None where the
    layer has no such input); kappas: {label: kappa_ref}. Every element is compared. Returns the
    worst err / (kappa A) per tensor."""
    ref = problem.grads() if ref is None else ref
    A = problem.majorant() if A is None else A
    worst, bad = {}, []
    for lab, r, a, g in zip(GRAD_LABELS, ref, A, got):
        if r is None:
            continue
        kap = kappa(lab, kappas[lab], problem.cin_g, problem.k, bwd_math)
        ratio, idx, n = elementwise_excess(g, r, a, kap)
        assert n == r.numel(), f"{what} {lab}: {r.numel() - n} elements not comparable"
        worst[lab] = ratio
        if ratio > 1:
            pos = f", tile position ({idx[-2] % TILE[0]}, {idx[-1] % TILE[1]})" if lab not in ("g_w", "g_b") else ""
            bad.append(f"{what} {lab} [{bwd_math}]: err / (kappa A) = {ratio:.3g} at {idx}{pos}; kappa {kap:.3e}, "
                       f"got {float(g[idx]):.9e}, ref {float(r[idx]):.9e}, A {float(a[idx]):.3e}")
    print(f"{what} [{bwd_math}] worst err/(kappa A): " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert not bad, "\n".join(bad)
    return worst


@functools.lru_cache(maxsize=None)
def _load_json(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as fh:
        return json.load(fh)


def load_kappa():
    return _load_json("bwd_bound_kappa.json")


# ------------------------------------------------------------------------------------------------
# The element-wise forward criterion: |got - ref| <= kappa * A + 1e-30 per element of y and cout,
# ref the float64 oracle on fp32-rounded operands (pool winners, the threshold mask and the nearest
# upsample are then decided on identical values: no element is left out), A the majorant below,
# kappa by the rule of kappa() above from tests/golden/fwd_bound_kappa.json (tools/fwd_kappa.py: the
# reference's own float32 run measured against the same float64 oracle).
# ------------------------------------------------------------------------------------------------
FWD_LABELS = ("y", "cout")


def nconv2d_forward_majorant(x, c, w, b, stride=(1, 1), pad=(0, 0), dil=(1, 1), groups=1, eps=R.EPS):
    """First-order error magnitudes of oracle.nconv_ref.nconv2d's two outputs in float64, every
    factor replaced by its absolute value and every subtraction by an addition. With
    Nabs = conv(|x c|, |w|), Dabs = conv(|c|, |w|), D = conv(c, w), s[o] = sum w[o], sabs[o] = sum |w[o]|:

        A_y = Nabs / |D+eps| * (1 + Dabs / |D+eps|) + |b|        (y = N / (D+eps) + b)
        A_c = Dabs / |s| * (1 + sabs / |s|)                      (cout = D / s, s summed in fp32 too)

    so kappa * A is what a forward with relative error kappa per term may be off by. (x, c) are the
    glue's outputs. Returns (A_y, A_c)."""
    assert x.dtype == torch.float64
    geo = (stride, pad, dil, groups)
    aw = w.abs()
    D = F.conv2d(c, w, None, *geo)
    Nabs = F.conv2d((x * c).abs(), aw, None, *geo)
    Dabs = F.conv2d(c.abs(), aw, None, *geo)
    s = w.reshape(w.shape[0], -1).sum(-1).view(1, -1, 1, 1).abs()
    sabs = aw.reshape(w.shape[0], -1).sum(-1).view(1, -1, 1, 1)
    inv = 1 / (D + eps).abs()
    A_y = Nabs * inv * (1 + Dabs * inv) + b.abs().view(1, -1, 1, 1)
    A_c = Dabs / s * (1 + sabs / s)
    return A_y, A_c


class FwdProblem:
    """One layer-forward comparison: fp32-rounded float64 operands and the geometry."""

    def __init__(self, name, mode, ops, geom):
        self.name, self.mode, self.ops, self.geom = name, mode, list(ops), geom
        self.cin_g, self.k = ops[4].shape[1], ops[4].shape[2]

    def outputs(self, dtype=torch.float64, eps=R.EPS):
        """(y, cout) of the oracle's own op sequence in dtype, as float64."""
        with torch.no_grad():
            ops = [None if t is None else t.to(dtype) for t in self.ops]
            x, c = glue(self.mode, *ops[:4])
            return tuple(t.double() for t in R.nconv2d(x, c, ops[4], ops[5], *self.geom, eps=eps))

    def majorant(self):
        xa, ca, xb, cb, w, b = self.ops
        with torch.no_grad():
            x, c = glue(self.mode, xa, ca, xb, cb)
            return nconv2d_forward_majorant(x, c, w, b, *self.geom)

    def kappa_ref(self, ref=None, A=None):
        """Per output max_i |err_i| / A_i of the oracle's float32 run against its float64 run."""
        ref = self.outputs() if ref is None else ref
        A = self.majorant() if A is None else A
        return {lab: float(((g - r).abs() / (a + 1e-30)).max())
                for lab, r, g, a in zip(FWD_LABELS, ref, self.outputs(torch.float32), A)}


def layer_fwd_problem(case, batch=2):
    """test_layer_forward's operands (seed 1234), fp32-rounded: the values the device receives."""
    name, mode, cin, cout, k, pad, stride, dil, groups, *_ = case
    ops = [r32(t) for t in build_case(case, 1234, batch)]
    return FwdProblem(name, mode, ops, ((stride, stride), (pad, pad), (dil, dil), groups))


def phase_fwd_inputs(case):
    """test_upcat_phase_forward's float64 operands (one generator, seed 11, batch 3), unrounded."""
    name, mode, pad, a_shape, b_shape = case
    g = torch.Generator().manual_seed(11)
    xa, ca = rand_pair(g, 3, *a_shape, dtype=torch.float64)
    xb, cb = rand_pair(g, 3, *b_shape, dtype=torch.float64)
    w = rand_weight(g, 8, 16, 3, 3, torch.float64)
    b = torch.rand(8, generator=g, dtype=torch.float64) * 0.1
    return xa, ca, xb, cb, w, b


def phase_fwd_problem(case):
    """test_upcat_phase_forward's operands, fp32-rounded."""
    name, mode, pad, *_ = case
    return FwdProblem(name, mode, [r32(t) for t in phase_fwd_inputs(case)], ((1, 1), (pad, pad), (1, 1), 1))


def fwd_problem(kind, name):
    """The FwdProblem of a LAYER_CASES ("layer"), PHASE_CASES ("phase") or FWD_SLICE_CASES ("slice")
    entry, by name."""
    if kind == "layer":
        return layer_fwd_problem(next(c for c in LAYER_CASES if c[0] == name))
    if kind == "phase":
        return phase_fwd_problem(next(c for c in PHASE_CASES if c[0] == name))
    cs, batch, case = next(e for e in FWD_SLICE_CASES if e[2][0] == name)
    return layer_fwd_problem(case, batch)


@functools.lru_cache(maxsize=None)
def fwd_budget(kind, name):
    """(problem, float64 outputs, majorant) of a forward case, computed once and shared (read-only)
    by the tests that need it: every fwd_math of a layer case, the CPU self-checks."""
    prob = fwd_problem(kind, name)
    return prob, prob.outputs(), prob.majorant()


def assert_outputs_elementwise(what, problem, got, kappas, fwd_math="fp32", ref=None, A=None):
    """The element-wise criterion on (y, cout). got: float64 CPU tensors; kappas: {label:
    kappa_ref}; fwd_math: the arithmetic of the kernel that ran (bf16x3 adds its per-product bound;
    bf16x9's products are exact and add nothing). Every element is compared. Prints and returns
    the worst err / (kappa A) per output."""
    ref = problem.outputs() if ref is None else ref
    A = problem.majorant() if A is None else A
    worst, bad = {}, []
    for lab, r, a, g in zip(FWD_LABELS, ref, A, got):
        kap = kappa(lab, kappas[lab], problem.cin_g, problem.k, fwd_math)
        ratio, idx, n = elementwise_excess(g, r, a, kap)
        assert n == r.numel(), f"{what} {lab}: {r.numel() - n} elements not comparable"
        worst[lab] = ratio
        if ratio > 1:
            bad.append(f"{what} {lab} [{fwd_math}]: err / (kappa A) = {ratio:.3g} at {idx}, tile position "
                       f"({idx[-2] % TILE[0]}, {idx[-1] % TILE[1]}); kappa {kap:.3e}, got {float(g[idx]):.9e}, "
                       f"ref {float(r[idx]):.9e}, A {float(a[idx]):.3e}")
    print(f"{what} [{fwd_math}] worst err/(kappa A): " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert not bad, "\n".join(bad)
    return worst


def load_fwd_kappa():
    return _load_json("fwd_bound_kappa.json")
