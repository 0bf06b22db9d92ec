"""References and inputs of the confidence-loss tests (test_confloss_cpu.py, test_gpu_confloss.py,
test_gpu_conf_train.py):

  rule_fp32         the rule of include/nconv.h (nconv_conf_loss_*) restated in numpy, operation by
                    operation in fp32 -- what the kernels must reproduce bit for bit per element
  published_loss    the published formula (Eldesokey, Felsberg, Khan, TPAMI 2019; ConfLossDecay) in torch,
                    in whatever dtype its inputs have (float64 in the tests, differentiated by autograd)
  loss_bound        the derived bound on |L_fp32 - L_float64|
  dnet_forward_with_confidence   the oracle's DNET forward returning the cropped confidence too
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nconv_ref as R

TILE_TERMS = 16 * 64  # the terms of one fp32 partial (conf_loss.hip: one 16 x 64 tile per workgroup)
f32 = np.float32


def rule_fp32(r, c, t, lam, err="smooth_l1", beta=1.0, gloss=1.0):
    """(terms, g_r, g_c) per element, fp32, every operation rounded once in the order the header fixes.
    r, c, t: float32 arrays of one shape; n = their size. The loss itself is a sum of `terms` (its
    summation order is the kernel's own; see loss_bound)."""
    r, c, t = (np.asarray(x, dtype=f32) for x in (r, c, t))
    lam, beta, gloss = f32(lam), f32(beta), f32(gloss)
    n = r.size
    v = t != 0
    d = r - t
    a = np.abs(d)
    if err == "smooth_l1":
        e = np.where(a < beta, ((f32(0.5) * a) * a) / beta, a - f32(0.5) * beta).astype(f32)
        de = np.where(a < beta, d / beta, np.where(d > 0, f32(1), f32(-1))).astype(f32)
    elif err == "l2":
        e = d * d
        de = f32(2) * d
    else:
        raise ValueError(err)
    one = f32(1.0)
    terms = np.where(v, e - (lam * c) * (one - e), f32(0)).astype(f32)
    k = gloss * (one / f32(n))
    g_r = np.where(v, (k * de) * (one + lam * c), f32(0)).astype(f32)
    g_c = np.where(v, -((k * lam) * (one - e)), f32(0)).astype(f32)
    for x in (e, de, terms, g_r, g_c):
        assert x.dtype == f32
    return terms, g_r, g_c


def published_loss(r, c, t, lam, err="smooth_l1", beta=1.0):
    """val = (t != 0); err = smooth_l1(r * val, t * val, 'none') (or the squared error);
    loss = mean(err - lam * (c * val - err * c * val))."""
    val = (t != 0).to(r.dtype)
    if err == "smooth_l1":
        e = F.smooth_l1_loss(r * val, t * val, reduction="none", beta=beta)
    else:
        e = (r * val - t * val) ** 2
    return (e - lam * (c * val - e * c * val)).mean()


def loss_bound(r, c, t, lam, err="smooth_l1", beta=1.0):
    """(8 + T) 2^-24 (1 / n) sum(e + lam c (1 + e)) over the valid pixels, in float64: at most 8
    roundings per term (d, e's three, lam c, 1 - e, their product, the difference), each relative
    to a quantity bounded by e + lam c (1 + e), plus a T-term fp32 sum (T = TILE_TERMS; the sums over
    tiles and images run in double, and the final rounding to fp32 is one of the 8)."""
    r, c, t = (torch.as_tensor(x).double() for x in (r, c, t))
    v = t != 0
    d = r - t
    a = d.abs()
    e = torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta) if err == "smooth_l1" else d * d
    mag = torch.where(v, e + lam * c.abs() * (1 + e), torch.zeros_like(e)).sum().item()
    return (8 + TILE_TERMS) * 2.0 ** -24 * mag / r.numel()


def loss_inputs(g, shape, beta=1.0):
    """(r, c, t) float32 tensors: t 30 % non-zero in (0, 80]; c in [0, 1] with exact 0 and 1; r near t with
    some |d| exactly beta, some d exactly 0, some far off (the linear branch)."""
    t = (torch.rand(shape, generator=g) * 79 + 1) * (torch.rand(shape, generator=g) < 0.3)
    c = torch.rand(shape, generator=g)
    u = torch.rand(shape, generator=g)
    c = torch.where(u < 0.1, torch.zeros_like(c), torch.where(u > 0.9, torch.ones_like(c), c))
    r = t + torch.randn(shape, generator=g) * 1.5
    u = torch.rand(shape, generator=g)
    t = torch.round(t * 8) / 8  # t and t +- beta exactly representable, so |d| == beta holds exactly
    r = torch.where(u < 0.1, t, r)
    r = torch.where((u >= 0.1) & (u < 0.15), t + beta, r)
    r = torch.where((u >= 0.15) & (u < 0.2), t - beta, r)
    r = torch.where((u >= 0.2) & (u < 0.25), t + 7.25, r)
    return r.float(), c.float(), t.float()


def dnet_forward_with_confidence(S, params, crop="literal", pool_idx=None):
    """R.dnet_forward composed from the same pieces (nconv2d, _pool, _crop), returning (depth,
    confidence): nconv7's outputs, both cropped by the same window. The depth is asserted equal to
    R.dnet_forward's."""
    def L(name, x, c):
        w, b = params[name]
        st, pad = R.DNET_GEOMETRY[name]
        return R.nconv2d(x, c, w, b, st, pad)

    pi = pool_idx or {}
    P = lambda t, k, i: R._pool(t, pi[k][i] if k in pi else None)  # noqa: E731
    c0 = (S > 0.01).to(S.dtype)
    x1, c1 = L("nconv1", S, c0)
    x1, c1 = L("nconv2", x1, c1)
    x2, c2 = L("nconv_down1", P(x1, "down1", 0), P(c1, "down1", 1))
    x3, c3 = L("nconv_down2", P(x2, "down2", 0), P(c2, "down2", 1))
    x4, c4 = L("nconv_down3", P(x3, "down3", 0), P(c3, "down3", 1))
    up = lambda t, ref: F.interpolate(t, ref.shape[2:], mode="nearest")  # noqa: E731
    x34, c34 = L("nconv4", torch.cat((x3, up(x4, c3)), 1), torch.cat((c3, up(c4, c3)), 1))
    x23, c23 = L("nconv5", torch.cat((x2, up(x34, c2)), 1), torch.cat((c2, up(c34, c2)), 1))
    xo, co = L("nconv6", torch.cat((up(x23, S), x1), 1), torch.cat((up(c23, S), c1), 1))
    xo, co = L("nconv7", xo, co)
    H, W = S.shape[2], S.shape[3]
    depth, conf = R._crop(xo, H, W, crop), R._crop(co, H, W, crop)
    assert torch.equal(depth.detach(), R.dnet_forward(S, params, crop, pool_idx).detach())
    return depth, conf
