"""Shared inputs, float64 reference and a-priori error budget of the depth-metrics tests (no tests
here). Everything is computed on the CPU from seeded fp32 inputs and cached per case."""
import functools
import math

import torch

NSUMS = 12
THRESHOLDS = (1.25, 1.5625, 1.953125)  # 1.25^k, exact in fp32
U = 2.0 ** -24


def _clamped(pred, clamp):
    """The clamp in fp32 (exact; torch.clamp keeps a NaN)."""
    lo, hi = (None, None) if clamp is None else clamp
    p = pred
    if lo:
        p = torch.clamp(p, min=lo)
    if hi:
        p = torch.clamp(p, max=hi)
    return p


def _valid(gt, gt_min=None, gt_max=None):
    v = gt > 0
    if gt_min:
        v &= gt >= torch.tensor(gt_min, dtype=torch.float32)
    if gt_max:
        v &= gt <= torch.tensor(gt_max, dtype=torch.float32)
    return v


def _near_threshold(pred, gt, valid, clamp):
    p, g = _clamped(pred, clamp).double(), gt.double()
    ok = valid & (p > 0)
    one = torch.ones_like(g)
    ratio = torch.maximum(torch.where(ok, p, one) / torch.where(ok, g, one),
                          torch.where(ok, g, one) / torch.where(ok, p, one))
    near = torch.zeros_like(ok)
    for t in THRESHOLDS:
        near |= (ratio / t - 1).abs() <= 1e-4
    return near & ok


def make_case(B, H, W, seed, density=0.3, gt_min=None, gt_max=None, clamp=None):
    """(pred, gt), fp32 (B, 1, H, W) on the CPU: gt = (rand * 79 + 1) * (rand < density);
    pred = gt * exp(U(-ln 2.5, ln 2.5)) at valid pixels, random elsewhere. Every valid pixel whose
    float64 ratio max(p/g, g/p) lies within relative 1e-4 of a delta threshold gets pred = gt (and,
    where a clamp then still leaves it there, gt = 0), so the delta counts do not depend on fp32
    rounding and must match exactly."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, 1, H, W)
    gt = (torch.rand(shape, generator=g) * 79 + 1) * (torch.rand(shape, generator=g) < density)
    u = (torch.rand(shape, generator=g) * 2 - 1) * math.log(2.5)
    other = torch.rand(shape, generator=g) * 80
    pred = torch.where(gt > 0, gt * torch.exp(u), other)
    near = _near_threshold(pred, gt, _valid(gt, gt_min, gt_max), clamp)
    pred = torch.where(near, gt, pred)
    near = _near_threshold(pred, gt, _valid(gt, gt_min, gt_max), clamp)
    gt = torch.where(near, torch.zeros_like(gt), gt)
    assert not _near_threshold(pred, gt, _valid(gt, gt_min, gt_max), clamp).any()
    return pred.contiguous(), gt.contiguous()


def _terms(pred, gt, gt_min=None, gt_max=None, clamp=None):
    """float64 per-pixel quantities from the fp32 inputs: valid, pos, p, g, e, d, l, ratio (the
    inverse / log / ratio terms set to harmless values outside pos)."""
    valid = _valid(gt, gt_min, gt_max)
    p, g = _clamped(pred, clamp).double(), gt.double()
    pos = valid & (p > 0)
    one = torch.ones_like(g)
    ps, gs = torch.where(pos, p, one), torch.where(pos, g, one)
    gv = torch.where(valid, g, one)
    return valid, pos, p, gv, p - g, 1 / ps - 1 / gs, ps.log() - gs.log(), torch.maximum(ps / gs, gs / ps), ps, gs


def reference_sums(pred, gt, gt_min=None, gt_max=None, clamp=None):
    """The twelve sums per image in float64, (B, 12), from the same fp32 inputs."""
    valid, pos, p, gv, e, d, l, ratio, ps, gs = _terms(pred, gt, gt_min, gt_max, clamp)
    zero = torch.zeros_like(e)

    def over(mask, x):
        return torch.where(mask, x, zero).flatten(1).sum(1)

    rows = [valid.flatten(1).sum(1).double(), pos.flatten(1).sum(1).double(),
            over(valid, e.abs()), over(valid, e * e), over(valid, e.abs() / gv), over(valid, e * e / gv),
            over(pos, d.abs()), over(pos, d * d), over(pos, l * l)]
    rows += [(pos & (ratio < t)).flatten(1).sum(1).double() for t in THRESHOLDS]
    return torch.stack(rows, dim=1)


def budget(pred, gt, gt_min=None, gt_max=None, clamp=None):
    """(B, 7): the bound on |S_gpu - S_64| for sums 2..8, u (16 S_64 + 4 C) with u = 2^-24 and C the
    sum of the per-pixel first-order magnitudes. 16: at most 12 fp32 additions on any term's path
    through a 1,024-pixel tile plus the double stage; 4: second-order terms and a 2-ulp logf.
    Asserts that the bound is not vacuous (<= 1e-4 S_64 wherever S_64 > 0)."""
    valid, pos, p, gv, e, d, l, ratio, ps, gs = _terms(pred, gt, gt_min, gt_max, clamp)
    zero = torch.zeros_like(e)
    ae, ad, al = e.abs(), d.abs(), l.abs()
    inv = 1 / ps + 1 / gs + ad
    logs = 2 * ps.log().abs() + 2 * gs.log().abs() + al
    c = [(valid, ae), (valid, 3 * e * e), (valid, 2 * ae / gv), (valid, 4 * e * e / gv),
         (pos, inv), (pos, 2 * ad * inv + d * d), (pos, 2 * al * logs + l * l)]
    C = torch.stack([torch.where(m, x, zero).flatten(1).sum(1) for m, x in c], dim=1)
    S = reference_sums(pred, gt, gt_min, gt_max, clamp)[:, 2:9]
    bound = U * (16 * S + 4 * C)
    assert (bound <= 1e-4 * S)[S > 0].all(), (bound / S).max()
    return bound


@functools.lru_cache(maxsize=None)
def case(B, H, W, seed, gt_min=None, gt_max=None, clamp=None):
    """(pred, gt, reference sums (B, 12), budget (B, 7)) of a seeded case; computed once, shared and
    not to be modified."""
    kw = dict(gt_min=gt_min, gt_max=gt_max, clamp=clamp)
    pred, gt = make_case(B, H, W, seed, **kw)
    return pred, gt, reference_sums(pred, gt, **kw), budget(pred, gt, **kw)


def check_rows(got, ref, bound, what=""):
    """got (B, 12) against the reference: sums 2..8 within the budget, the counts exactly equal."""
    got = got.detach().cpu()
    counts = [0, 1, 9, 10, 11]
    assert torch.equal(got[:, counts], ref[:, counts]), (what, got[:, counts], ref[:, counts])
    err = (got[:, 2:9] - ref[:, 2:9]).abs()
    assert (err <= bound).all(), (what, err / bound.clamp(min=1e-300), err, bound)
