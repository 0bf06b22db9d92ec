"""References, bounds and inputs of the cross-view consistency tests (test_consistency_cpu.py,
test_gpu_consistency.py):

  rule_fp32       nconv_depth_consistency's rule of include/nconv.h restated in numpy, every operation an explicit
                  float32 step, on top of warp_cases.rule_fp32 (validity, u, v, the blend and its derivative are
                  the view warp's) -- what the kernel must reproduce bit for bit
  loss_rule_fp32  nconv_geo_consistency_loss_*'s rule likewise: the terms, n_g, the loss by reduce_tree and g_depth
  composition     both composed from torch ops in whatever dtype is asked for: a meshgrid, matrix products,
                  F.grid_sample(align_corners=True) on the source depth, a masked mean, autograd (float64: the
                  reference; float32: what kappa is measured from)
  majorants       first-order running error bounds of the fp32 rule per element, in float64: every operation
                  adds U |result| to the propagated error of its operands (class Err); the bilinear sample
                  propagates the coordinates' error through the taps' slopes, as warp_cases.majorants does
  scenes          random smooth scenes with holes, and the analytic wall-and-rectangle scene rendered by exact ray
                  casting in float64, with the decision expected on every pixel away from the silhouettes
  measure_kappa   torch's float32 run of the composition against float64 in units of the majorants;
                  `python tests/consistency_cases.py --write` writes tests/golden/consistency_bound_kappa.json
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import reduce_tree as RT
import warp_cases as W

f32 = np.float32
U = W.U
KAPPA_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consistency_bound_kappa.json")
Z_MIN = 1e-3


# ------------------------------------------------------------------------------------------------
# the fp32 rules
# ------------------------------------------------------------------------------------------------
def _col(a):
    return np.asarray(a, dtype=f32)[:, None, None]


def _view_fp32(depth, k, src, m, mask, z_min, z_max):
    """One source through the view warp's restatement, and what it does not hand out recomputed by the same
    float32 steps: c, c' and the four taps. src: (B, Hs, Ws)."""
    z = np.asarray(depth, dtype=f32)
    src = np.asarray(src, dtype=f32)
    B, H, Wd = z.shape
    Hs, Ws = src.shape[1:]
    r = W.rule_fp32(z, k, src[:, None], m, mask, g_warped=np.ones((B, 1, H, Wd), dtype=f32), z_min=z_min, z_max=z_max)
    kb, mb = W._batched(k, B, (3, 3)), W._batched(m, B, (3, 4))
    fx, fy, cx, cy = _col(kb[:, 0, 0]), _col(kb[:, 1, 1]), _col(kb[:, 0, 2]), _col(kb[:, 1, 2])
    M2 = [_col(mb[:, 2, q]) for q in range(4)]
    jj = np.arange(Wd, dtype=f32)[None, None, :]
    ii = np.arange(H, dtype=f32)[None, :, None]
    with np.errstate(all="ignore"):
        tx, ty = jj - cx, ii - cy
        x, y = (tx * z) / fx, (ty * z) / fy
        c = ((M2[0] * x + M2[1] * y) + M2[2] * z) + M2[3]
        X, Y = tx / fx + np.zeros_like(z), ty / fy + np.zeros_like(z)
        dc = (M2[0] * X + M2[1] * Y) + M2[2]
        valid = r["valid"]
        us, vs = np.where(valid, r["u"], f32(0)), np.where(valid, r["v"], f32(0))
        j0, i0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
        j1, i1 = np.minimum(j0 + 1, Ws - 1), np.minimum(i0 + 1, Hs - 1)
        bi = np.arange(B)[:, None, None]
        taps = [src[bi, i0, j0], src[bi, i0, j1], src[bi, i1, j0], src[bi, i1, j1]]
        zmax = f32(W.FLT_MAX) if z_max == 0.0 else f32(z_max)
        tvalid = np.ones(z.shape, dtype=bool)
        for t in taps:
            tvalid &= (t > f32(z_min)) & (t <= zmax)
        pvalid = (z > f32(z_min)) & (z <= zmax)
        if mask is not None:
            pvalid = pvalid & (np.asarray(mask) != 0)
    # where the pixel is valid `warped` is the blend itself; elsewhere every use of it is masked
    return {"valid": valid, "tvalid": tvalid, "pvalid": pvalid, "u": r["u"], "v": r["v"], "c": c.astype(f32),
            "dc": dc.astype(f32), "zs": r["warped"][:, 0], "dzs": r["g_depth_warp"], "z": z}


def rule_fp32(depth, k, src_depths, k_srcs, ms, m_backs, px_tol=1.0, rel_tol=0.01, min_views=1, mask=None,
              z_min=Z_MIN, z_max=0.0):
    """fused (B, H, W) float32, count and views uint8, reproj and reldiff (B, S, H, W) float32, and cons (B, S, H, W)
    bool. depth (B, H, W); src_depths a list of (B, Hs, Ws); k, k_srcs[s] (3, 3) or (B, 3, 3); ms[s], m_backs[s]
    (3, 4) or (B, 3, 4); mask (B, H, W) or None."""
    z = np.asarray(depth, dtype=f32)
    B, H, Wd = z.shape
    S = len(src_depths)
    jj = np.arange(Wd, dtype=f32)[None, None, :]
    ii = np.arange(H, dtype=f32)[None, :, None]
    tol2 = f32(px_tol) * f32(px_tol)
    acc = z.copy()
    n = np.zeros(z.shape, dtype=np.int64)
    bits = np.zeros(z.shape, dtype=np.int64)
    reproj = np.zeros((B, S, H, Wd), dtype=f32)
    reldiff = np.zeros((B, S, H, Wd), dtype=f32)
    cons_all = np.zeros((B, S, H, Wd), dtype=bool)
    pvalid = None
    for s in range(S):
        g = _view_fp32(z, k, src_depths[s], ms[s], mask, z_min, z_max)
        pvalid = g["pvalid"]
        ks, mb = W._batched(k_srcs[s], B, (3, 3)), W._batched(m_backs[s], B, (3, 4))
        fxs, fys, cxs, cys = _col(ks[:, 0, 0]), _col(ks[:, 1, 1]), _col(ks[:, 0, 2]), _col(ks[:, 1, 2])
        Mb = [[_col(mb[:, r, q]) for q in range(4)] for r in range(3)]
        with np.errstate(all="ignore"):
            zs = g["zs"]
            xs = ((g["u"] - cxs) * zs) / fxs
            ys = ((g["v"] - cys) * zs) / fys
            a2, b2, c2 = (((Mb[r][0] * xs + Mb[r][1] * ys) + Mb[r][2] * zs) + Mb[r][3] for r in range(3))
            u2, v2 = a2 / c2, b2 / c2
            du, dv = u2 - jj, v2 - ii
            d2 = (du * du) + (dv * dv)
            rz = np.abs(c2 - z)
            seen = g["valid"] & g["tvalid"] & (c2 > 0)
            cons = seen & (d2 <= tol2) & (rz <= f32(rel_tol) * z)
            acc = np.where(cons, acc + c2, acc).astype(f32)
            n += cons
            bits |= cons.astype(np.int64) << s
            reproj[:, s] = np.where(seen, d2, f32(np.inf))
            reldiff[:, s] = np.where(seen, rz / z, f32(np.inf))
            cons_all[:, s] = cons
    with np.errstate(all="ignore"):
        fused = np.where(pvalid & (n >= min_views), acc / (n + 1).astype(f32), f32(0)).astype(f32)
    return {"fused": fused, "count": n.astype(np.uint8), "views": bits.astype(np.uint8), "reproj": reproj,
            "reldiff": reldiff, "cons": cons_all, "pvalid": pvalid}


def loss_rule_fp32(depth, k, src_depth, m, mask=None, gloss=1.0, z_min=Z_MIN, z_max=0.0):
    """terms (B, H, W) float32 (= the diff plane), counted (bool), n_g, loss (the stated tree, float32) and
    g_depth (B, H, W) float32."""
    g = _view_fp32(depth, k, src_depth, m, mask, z_min, z_max)
    ok = g["valid"] & g["tvalid"]
    one = f32(1.0)
    with np.errstate(all="ignore"):
        num = g["c"] - g["zs"]
        den = g["c"] + g["zs"]
        diff = np.abs(num) / den
        terms = np.where(ok, diff, f32(0)).astype(f32)
        n_g = int(ok.sum())
        kk = f32(gloss) * (one / f32(max(n_g, 1)))
        sg = np.where(num > 0, one, np.where(num < 0, f32(-1), f32(0))).astype(f32)
        dc, dzs = g["dc"], g["dzs"]
        quot = (((dc - dzs) * den) - (num * (dc + dzs))) / (den * den)
        g_depth = np.where(ok, (kk * sg) * quot, f32(0)).astype(f32)
    return {"terms": terms, "counted": ok, "n_g": n_g, "loss": RT.loss(terms, float(max(n_g, 1)), RT.ROWS),
            "g_depth": g_depth, "num": num}


# ------------------------------------------------------------------------------------------------
# the torch composition
# ------------------------------------------------------------------------------------------------
def _T(a, dtype):
    return torch.as_tensor(np.array(a)).to(dtype)


def _project(z, k, m, dtype):
    B, H, Wd = z.shape
    ii, jj = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(Wd, dtype=dtype), indexing="ij")
    col = lambda a: a[:, None, None]  # noqa: E731
    x = (jj - col(k[:, 0, 2])) * z / col(k[:, 0, 0])
    y = (ii - col(k[:, 1, 2])) * z / col(k[:, 1, 1])
    P = torch.stack((x, y, z, torch.ones_like(z)), dim=1)               # (B, 4, H, W)
    abc = torch.einsum("brq,bqhw->brhw", m, P)                          # the matrix product
    return abc[:, 0], abc[:, 1], abc[:, 2], ii, jj


def _sample(src, u, v, valid, dtype):
    """zs by grid_sample and whether all four taps are depths (gathered at floor / floor + 1, clamped)."""
    B, Hs, Ws = src.shape
    gx, gy = 2 * u / max(Ws - 1, 1) - 1, 2 * v / max(Hs - 1, 1) - 1
    grid = torch.where(valid[..., None], torch.stack((gx, gy), dim=-1), torch.zeros(*u.shape, 2, dtype=dtype))
    return F.grid_sample(src[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]


def _tvalid(src, u, v, valid, z_min, zmax):
    B, Hs, Ws = src.shape
    us, vs = torch.where(valid, u, torch.zeros_like(u)), torch.where(valid, v, torch.zeros_like(v))
    j0, i0 = us.floor().long(), vs.floor().long()
    j1, i1 = (j0 + 1).clamp(max=Ws - 1), (i0 + 1).clamp(max=Hs - 1)
    bi = torch.arange(B)[:, None, None]
    ok = torch.ones_like(valid)
    for t in (src[bi, i0, j0], src[bi, i0, j1], src[bi, i1, j0], src[bi, i1, j1]):
        ok = ok & (t > z_min) & (t <= zmax)
    return ok


def composition(depth, k, src_depths, k_srcs, ms, m_backs, px_tol=1.0, rel_tol=0.01, min_views=1, mask=None,
                gloss=1.0, z_min=Z_MIN, z_max=0.0, dtype=torch.float64):
    """Both features as a user composes them from torch ops, in `dtype`: rule_fp32's keys, and per source s the
    loss's terms_s, counted_s, n_g_s, loss_s, g_depth_s (autograd). A hole of the source is filled with a valid
    depth before sampling so that no NaN reaches a masked product; such pixels are not tvalid."""
    z0 = _T(depth, dtype)
    B, H, Wd = z0.shape
    S = len(src_depths)
    zmax = W.FLT_MAX if z_max == 0.0 else z_max
    zmin = float(f32(z_min))
    pvalid = torch.isfinite(z0) & (z0 > zmin) & (z0 <= zmax)
    if mask is not None:
        pvalid = pvalid & torch.as_tensor(np.asarray(mask) != 0)
    kt = _T(W._batched(k, B, (3, 3)), dtype)
    acc = torch.where(pvalid, z0, torch.zeros_like(z0))
    n = torch.zeros(z0.shape, dtype=torch.long)
    bits = torch.zeros(z0.shape, dtype=torch.long)
    out = {"reproj": np.zeros((B, S, H, Wd)), "reldiff": np.zeros((B, S, H, Wd)),
           "cons": np.zeros((B, S, H, Wd), dtype=bool), "seen": np.zeros((B, S, H, Wd), dtype=bool),
           "u": np.zeros((B, S, H, Wd)), "v": np.zeros((B, S, H, Wd))}
    inf = torch.full_like(z0, float("inf"))
    for s in range(S):
        src0 = _T(src_depths[s], dtype)
        Hs, Ws = src0.shape[1:]
        hole = ~(torch.isfinite(src0) & (src0 > zmin) & (src0 <= zmax))
        src = torch.where(hole, torch.ones_like(src0), src0)
        m, mb = _T(W._batched(ms[s], B, (3, 4)), dtype), _T(W._batched(m_backs[s], B, (3, 4)), dtype)
        ks = _T(W._batched(k_srcs[s], B, (3, 3)), dtype)
        z = torch.where(pvalid, z0, torch.ones_like(z0)).requires_grad_(True)
        a, b, c, ii, jj = _project(z, kt, m, dtype)
        front = c > 0
        cc = torch.where(front, c, torch.ones_like(c))
        u, v = a / cc, b / cc
        valid = pvalid & front & (u >= 0) & (u <= Ws - 1) & (v >= 0) & (v <= Hs - 1)
        zs = _sample(src, u, v, valid, dtype)
        tv = _tvalid(src0, u.detach(), v.detach(), valid, zmin, zmax)
        ok = valid & tv
        zsafe = torch.where(ok, zs, torch.ones_like(zs))
        col = lambda t: t[:, None, None]  # noqa: E731
        xs = (u - col(ks[:, 0, 2])) * zsafe / col(ks[:, 0, 0])
        ys = (v - col(ks[:, 1, 2])) * zsafe / col(ks[:, 1, 1])
        P = torch.stack((xs, ys, zsafe, torch.ones_like(zsafe)), dim=1)
        back = torch.einsum("brq,bqhw->brhw", mb, P)
        c2 = back[:, 2]
        seen = ok & (c2 > 0)
        c2s = torch.where(seen, c2, torch.ones_like(c2))
        u2, v2 = back[:, 0] / c2s, back[:, 1] / c2s
        d2 = (u2 - jj) ** 2 + (v2 - ii) ** 2
        rz = (c2s - z).abs()
        cons = seen & (d2 <= px_tol * px_tol) & (rz <= float(f32(rel_tol)) * z)
        acc = torch.where(cons, acc + c2s, acc)
        n = n + cons
        bits = bits | (cons.long() << s)
        out["reproj"][:, s] = torch.where(seen, d2, inf).detach().numpy()
        out["reldiff"][:, s] = torch.where(seen, rz / z, inf).detach().numpy()
        out["cons"][:, s], out["seen"][:, s] = cons.numpy(), seen.numpy()
        out["u"][:, s], out["v"][:, s] = u.detach().numpy(), v.detach().numpy()
        # the loss of this source
        diff = torch.where(ok, (c - zsafe).abs() / (c + zsafe), torch.zeros_like(c))
        n_g = int(ok.sum())
        loss = diff.sum() / max(n_g, 1)
        (g,) = torch.autograd.grad(loss * gloss, z)
        out[f"terms_{s}"], out[f"counted_{s}"], out[f"n_g_{s}"] = diff.detach().numpy(), ok.numpy(), n_g
        out[f"loss_{s}"], out[f"g_depth_{s}"] = loss.item(), g.numpy()
        out[f"num_{s}"] = (c - zsafe).detach().numpy()
    fused = torch.where(pvalid & (n >= min_views), acc / (n + 1).to(dtype), torch.zeros_like(acc))
    out.update(fused=fused.detach().numpy(), count=n.numpy().astype(np.uint8), views=bits.numpy().astype(np.uint8),
               pvalid=pvalid.numpy())
    return out


# ------------------------------------------------------------------------------------------------
# majorants: running first-order error bounds of the fp32 rule, in float64
# ------------------------------------------------------------------------------------------------
class Err:
    """A float64 value with a first-order bound e on the fp32 rule's error in it: an operation propagates its
    operands' bounds by the operation's partial derivatives and adds U |result| for its own rounding. Inputs
    (fp32 numbers, pixel indices) are exact: e = 0. A product also keeps the second-order term e_a e_b: d2 is a
    sum of squares of differences that are themselves near 0, where it is the leading one."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        o = Err.of(o)
        v = self.v - o.v
        return Err(v, self.e + o.e + U * np.abs(v))

    def __mul__(self, o):
        o = Err.of(o)
        v = self.v * o.v
        return Err(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(v))

    def __truediv__(self, o):
        o = Err.of(o)
        v = self.v / o.v
        return Err(v, (self.e + np.abs(v) * o.e) / np.abs(o.v) + U * np.abs(v))

    def abs(self):
        return Err(np.abs(self.v), self.e)


def _dot(r, x, y, z):
    return ((Err.of(r[0]) * x + Err.of(r[1]) * y) + Err.of(r[2]) * z) + Err.of(r[3])


def majorants(depth, k, src_depth, k_src, m, m_back, ok, gloss_kk=None):
    """{reproj, reldiff, z2, term, g_depth}: float64 (B, H, W) bounds on the fp32 rule's error of one source, on
    the pixels `ok` (elsewhere 0). The bilinear sample: err zs = |dIu| e_u + |dIv| e_v + 8 U max|tap| (w0u, w0v, six
    products and three sums less the shared ones, as warp_cases.majorants); its slopes dIu, dIv carry
    |D2| e_v + 8 U max|tap| and |D2| e_u + 8 U max|tap|, D2 the slopes' own slope."""
    z64 = np.asarray(depth, dtype=np.float64)
    B, H, Wd = z64.shape
    src = np.asarray(src_depth, dtype=np.float64)
    Hs, Ws = src.shape[1:]
    ok = np.asarray(ok, dtype=bool)
    col = lambda a: np.asarray(a, dtype=np.float64)[:, None, None]  # noqa: E731
    kb = W._batched(k, B, (3, 3))
    ks = W._batched(k_src, B, (3, 3))
    mm, mb = W._batched(m, B, (3, 4)), W._batched(m_back, B, (3, 4))
    jj = np.arange(Wd, dtype=np.float64)[None, None, :] + np.zeros((B, H, 1))
    ii = np.arange(H, dtype=np.float64)[None, :, None] + np.zeros((B, 1, Wd))
    with np.errstate(all="ignore"):
        z = Err(np.where(ok, z64, 1.0))
        tx, ty = Err(jj) - col(kb[:, 0, 2]), Err(ii) - col(kb[:, 1, 2])
        x, y = (tx * z) / col(kb[:, 0, 0]), (ty * z) / col(kb[:, 1, 1])
        M = [[col(mm[:, r, q]) for q in range(4)] for r in range(3)]
        a, b, c = (_dot(M[r], x, y, z) for r in range(3))
        u, v = a / c, b / c
        uc, vc = np.clip(np.where(ok, u.v, 0.0), 0, Ws - 1), np.clip(np.where(ok, v.v, 0.0), 0, Hs - 1)
        j0, i0 = np.floor(uc).astype(np.int64), np.floor(vc).astype(np.int64)
        j1, i1 = np.minimum(j0 + 1, Ws - 1), np.minimum(i0 + 1, Hs - 1)
        wu, wv = uc - j0, vc - i0
        bi = np.arange(B)[:, None, None]
        srcz = np.where(np.isfinite(src), src, 0.0)
        a00, a01, a10, a11 = srcz[bi, i0, j0], srcz[bi, i0, j1], srcz[bi, i1, j0], srcz[bi, i1, j1]
        amax = np.maximum(np.maximum(np.abs(a00), np.abs(a01)), np.maximum(np.abs(a10), np.abs(a11)))
        top, bot = (1 - wu) * a00 + wu * a01, (1 - wu) * a10 + wu * a11
        dIu, dIv = (1 - wv) * (a01 - a00) + wv * (a11 - a10), bot - top
        D2 = np.abs((a11 - a10) - (a01 - a00))
        zs = Err((1 - wv) * top + wv * bot, np.abs(dIu) * u.e + np.abs(dIv) * v.e + 8 * U * amax)
        # the way back
        xs = ((u - col(ks[:, 0, 2])) * zs) / col(ks[:, 0, 0])
        ys = ((v - col(ks[:, 1, 2])) * zs) / col(ks[:, 1, 1])
        Mb = [[col(mb[:, r, q]) for q in range(4)] for r in range(3)]
        a2, b2, c2 = (_dot(Mb[r], xs, ys, zs) for r in range(3))
        du, dv = a2 / c2 - Err(jj), b2 / c2 - Err(ii)
        d2 = (du * du) + (dv * dv)
        rz = (c2 - z).abs()
        rel = rz / z
        # the loss
        num, den = c - zs, c + zs
        term = num.abs() / den
        out = {"reproj": d2.e, "reldiff": rel.e, "z2": c2.e, "term": term.e}
        if gloss_kk is not None:
            X, Y = tx / col(kb[:, 0, 0]), ty / col(kb[:, 1, 1])
            dp = [(Err.of(M[r][0]) * X + Err.of(M[r][1]) * Y) + Err.of(M[r][2]) for r in range(3)]
            dub, dvb = (dp[0] - u * dp[2]) / c, (dp[1] - v * dp[2]) / c
            EdIu = Err(dIu, D2 * v.e + 8 * U * amax)
            EdIv = Err(dIv, D2 * u.e + 8 * U * amax)
            dzs = (EdIu * dub) + (EdIv * dvb)
            quot = (((dp[2] - dzs) * den) - (num * (dp[2] + dzs))) / (den * den)
            g = Err(gloss_kk, 2 * U * abs(gloss_kk)) * quot
            out["g_depth"] = g.e
    return {key: np.where(ok, val, 0.0) for key, val in out.items()}


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _smooth(g, B, H, Wd, amp):
    coarse = torch.rand(B, 1, 4, 6, generator=g) * amp
    return F.interpolate(coarse, size=(max(H, 2), max(Wd, 2)), mode="bilinear",
                         align_corners=True)[:, 0, :H, :Wd].contiguous().numpy().astype(f32)


def inverse_rigid(p):
    R, t = p[:, :3], p[:, 3]
    return np.concatenate((R.T, -(R.T @ t)[:, None]), axis=1)


def scene(seed, B, size, src_size=None, S=2, per_image=True, with_mask=False, sparse=False, holes=True):
    """A dict of float32 arrays for S sources: depth (B, H, W) around 10 m with 0.1 m of relief and (holes) a few
    0, NaN, inf and negative pixels; src_depths [S] of (B, Hs, Ws), the same wall seen from a camera a few
    decimetres away with its own relief, so that part of the pixels agree within rel_tol = 0.01 and part do not
    (sparse: a third of the source pixels are holes, a few NaN); k, k_srcs, ms, m_backs ((B, 3, 4) or (3, 4));
    poses (float64); mask (B, H, W) uint8 or None."""
    H, Wd = size
    Hs, Ws = src_size or size
    g = torch.Generator().manual_seed(seed)
    depth = (10.0 + _smooth(g, B, H, Wd, 0.1)).astype(f32)
    if holes and H * Wd >= 64:
        r = torch.rand(B, H, Wd, generator=g).numpy()
        depth[r < 0.02] = 0.0
        depth[(r >= 0.02) & (r < 0.03)] = np.nan
        depth[(r >= 0.03) & (r < 0.04)] = np.inf
        depth[(r >= 0.04) & (r < 0.05)] = -3.0
    f = 0.9 * max(Wd, 2)
    k = W.intrinsics(H, Wd, f)
    ksrc = W.intrinsics(Hs, Ws, f * Ws / Wd)
    out = {"depth": depth, "k": k.astype(f32), "src_depths": [], "k_srcs": [], "ms": [], "m_backs": [], "poses": []}
    for s in range(S):
        sign = 1.0 if s % 2 == 0 else -1.0
        poses = [W.rigid(0.002 * (b + 1) * sign, -0.003 * (s + 1), 0.001,
                         (sign * (0.10 + 0.04 * b), -0.03 * (s + 1), sign * (0.30 - 0.08 * b))) for b in range(B)]
        if not per_image:
            poses = [poses[0]] * B
        tz = np.array([p[2, 3] for p in poses], dtype=f32)[:, None, None]
        sd = (10.0 + tz + _smooth(g, B, Hs, Ws, 0.1)).astype(f32)
        if sparse:
            r = torch.rand(B, Hs, Ws, generator=g).numpy()
            sd[r < 0.3] = 0.0
            sd[(r >= 0.3) & (r < 0.32)] = np.nan
        ms = np.stack([ksrc @ p for p in poses]).astype(f32)
        mbs = np.stack([k @ inverse_rigid(p) for p in poses]).astype(f32)
        out["src_depths"].append(sd)
        out["k_srcs"].append(ksrc.astype(f32))
        out["ms"].append(ms if per_image else ms[0])
        out["m_backs"].append(mbs if per_image else mbs[0])
        out["poses"].append(np.stack(poses))
    out["mask"] = (torch.rand(B, H, Wd, generator=g) > 0.1).numpy().astype(np.uint8) if with_mask else None
    return out


# the analytic scene: a fronto-parallel wall at 8 m and a rectangle at 2 m in front of it; the source camera
# 0.5 m to the side, both cameras looking along z
WALL_Z, RECT_Z, BASELINE = 8.0, 2.0, 0.5
RECT = (-0.3, 0.3, -0.25, 0.25)  # x0, x1, y0, y1 in metres, in the target camera's frame
BAND = 2.0                        # pixels kept away from a silhouette edge, in either view


def _render(k, H, Wd, cam_x):
    """Depth by exact ray casting from a camera at (cam_x, 0, 0), and each pixel's distance in pixels to the
    rectangle's silhouette in that view (float64)."""
    fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    jj, ii = np.meshgrid(np.arange(Wd, dtype=np.float64), np.arange(H, dtype=np.float64))
    # the silhouette in this view: the rectangle's corners projected
    u0, u1 = cx + fx * (RECT[0] - cam_x) / RECT_Z, cx + fx * (RECT[1] - cam_x) / RECT_Z
    v0, v1 = cy + fy * RECT[2] / RECT_Z, cy + fy * RECT[3] / RECT_Z
    inside = (jj >= u0) & (jj <= u1) & (ii >= v0) & (ii <= v1)
    depth = np.where(inside, RECT_Z, WALL_Z)
    return depth, (u0, u1, v0, v1)


def _edge_distance(u, v, box):
    """The distance (max norm, pixels) of (u, v) to the boundary of the box (u0, u1, v0, v1)."""
    u0, u1, v0, v1 = box
    du = np.minimum(np.abs(u - u0), np.abs(u - u1))
    dv = np.minimum(np.abs(v - v0), np.abs(v - v1))
    in_u, in_v = (u >= u0) & (u <= u1), (v >= v0) & (v <= v1)
    inside = in_u & in_v
    d_in = np.minimum(du, dv)
    d_out = np.maximum(np.where(in_u, 0.0, du), np.where(in_v, 0.0, dv))
    return np.where(inside, d_in, d_out)


def analytic_scene(H=64, Wd=96, f=80.0, B=2):
    """The wall-and-rectangle scene: depth and src_depth (B, H, W) float32 rendered in float64 (2 and 8 are exact in
    fp32), k = k_src, m, m_back, and per target pixel the expected decision where it is safe to state one:
      expect    1 consistent, 0 not consistent, -1 no statement (within BAND pixels of a silhouette edge or of the
                source frame's border, in either view)
      kind      "seen" wall pixels the source sees, "hidden" wall pixels behind the rectangle in the source,
                "left" pixels whose projection leaves the source frame, "rect" the rectangle's own pixels"""
    k = W.intrinsics(H, Wd, f)
    fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    tgt, box_t = _render(k, H, Wd, 0.0)
    src, box_s = _render(k, H, Wd, BASELINE)
    pose = W.rigid(t=(-BASELINE, 0.0, 0.0))  # target camera frame -> source camera frame
    jj, ii = np.meshgrid(np.arange(Wd, dtype=np.float64), np.arange(H, dtype=np.float64))
    us = jj - fx * BASELINE / tgt        # the projection into the source: a shift by the disparity
    vs = ii + 0.0
    far_t = _edge_distance(jj, ii, box_t) >= BAND
    far_s = _edge_distance(us, vs, box_s) >= BAND + 1.0   # the taps reach one pixel further
    in_frame = (us >= BAND) & (us <= Wd - 1 - BAND) & (vs >= 0) & (vs <= H - 1)
    out_frame = (us <= -BAND) | (us >= Wd - 1 + BAND)
    wall = tgt == WALL_Z
    behind = (us >= box_s[0]) & (us <= box_s[1]) & (vs >= box_s[2]) & (vs <= box_s[3])  # the source sees the rectangle
    kind = np.full((H, Wd), "", dtype=object)
    safe = far_t & far_s
    kind[wall & safe & in_frame & ~behind] = "seen"
    kind[wall & safe & in_frame & behind] = "hidden"
    kind[far_t & out_frame] = "left"
    kind[~wall & safe & in_frame] = "rect"
    expect = np.full((H, Wd), -1, dtype=np.int64)
    expect[(kind == "seen") | (kind == "rect")] = 1
    expect[(kind == "hidden") | (kind == "left")] = 0
    rep = lambda a: np.broadcast_to(a, (B, *a.shape)).copy()  # noqa: E731
    return {"depth": rep(tgt.astype(f32)), "src_depths": [rep(src.astype(f32))], "k": k.astype(f32),
            "k_srcs": [k.astype(f32)], "ms": [(k @ pose).astype(f32)], "m_backs": [(k @ inverse_rigid(pose)).astype(f32)],
            "poses": [pose], "mask": None, "expect": rep(expect), "kind": rep(kind)}


# ------------------------------------------------------------------------------------------------
# kappa
# ------------------------------------------------------------------------------------------------
# (name, seed, B, size, src_size, S, per_image, with_mask, sparse): the GPU tests' shapes
CPU_CASES = [("17x65_from_19x70_s2", 1, 2, (17, 65), (19, 70), 2, True, False, False),
             ("45x67_s1_shared_mask_sparse", 2, 2, (45, 67), None, 1, False, True, True),
             ("64x96_s4", 3, 2, (64, 96), None, 4, True, True, False)]
OUTPUTS = ("reproj", "reldiff", "fused", "loss", "g_depth")
GLOSS = 1.0


def case_inputs(name):
    _, seed, B, size, src_size, S, per_image, with_mask, sparse = next(c for c in CPU_CASES if c[0] == name)
    return scene(seed, B, size, src_size, S, per_image, with_mask, sparse)


def _args(x):
    return (x["depth"], x["k"], x["src_depths"], x["k_srcs"], x["ms"], x["m_backs"])


def case_budget(name):
    """(inputs, float64 reference, per source the majorants and the keep masks) of a CPU case. A pixel is kept for
    source s where the float64 reference counts it and its u, v are farther than warp_cases.EDGE from every
    integer (the bilinear blend's kinks); for g_depth also |num| >= EDGE (the sign flips at 0)."""
    x = case_inputs(name)
    ref = composition(*_args(x), mask=x["mask"], gloss=GLOSS)
    S = len(x["src_depths"])
    near = lambda w: np.abs(w - np.rint(w)) < W.EDGE  # noqa: E731
    per = []
    for s in range(S):
        ok = ref["seen"][:, s] & ~near(ref["u"][:, s]) & ~near(ref["v"][:, s])
        kk = GLOSS / max(ref[f"n_g_{s}"], 1)
        A = majorants(x["depth"], x["k"], x["src_depths"][s], x["k_srcs"][s], x["ms"][s], x["m_backs"][s],
                      ref[f"counted_{s}"], kk)
        per.append({"A": A, "keep": ok, "keep_g": ok & (np.abs(ref[f"num_{s}"]) >= W.EDGE)})
    return x, ref, per


def fused_majorant(ref, per):
    """fused = (z + sum of the consistent z2) / (n + 1): the z2's bounds, n + 1 roundings of the sum and the
    division's, on pixels whose decisions are the reference's."""
    n = ref["count"].astype(np.float64)
    e = sum(np.where(ref["cons"][:, s], p["A"]["z2"], 0.0) for s, p in enumerate(per))
    return e / (n + 1) + (n + 2) * U * np.abs(ref["fused"])


def loss_majorant(ref, per, s):
    """the mean of the terms' bounds and nconv_photo_loss's summation bound (warp_cases.loss_bound)."""
    n = max(ref[f"n_g_{s}"], 1)
    return per[s]["A"]["term"].sum() / n + W.loss_bound(ref[f"terms_{s}"], n, ref[f"loss_{s}"])


def ratios(got, got_loss, ref, per, same):
    """max over the kept elements of |got - ref| / majorant per output. got: rule_fp32's dict (or the float32
    composition's); got_loss: per source {"loss", "g_depth"}; same: the pixels on which got's decisions are the
    reference's, per source (B, S, H, W)."""
    r = {key: 0.0 for key in OUTPUTS}
    tiny = 1e-300
    with np.errstate(invalid="ignore"):  # inf - inf off the kept pixels
        return _ratios(got, got_loss, ref, per, same, r, tiny)


def _ratios(got, got_loss, ref, per, same, r, tiny):
    for s, p in enumerate(per):
        keep = p["keep"] & same[:, s]
        for key in ("reproj", "reldiff"):
            err = np.abs(np.asarray(got[key][:, s], dtype=np.float64) - ref[key][:, s])[keep]
            r[key] = max(r[key], float((err / (p["A"][key][keep] + tiny)).max(initial=0.0)))
        r["loss"] = max(r["loss"], abs(float(got_loss[s]["loss"]) - ref[f"loss_{s}"]) / loss_majorant(ref, per, s))
        kg = p["keep_g"] & same[:, s]
        err = np.abs(np.asarray(got_loss[s]["g_depth"], dtype=np.float64) - ref[f"g_depth_{s}"])[kg]
        r["g_depth"] = max(r["g_depth"], float((err / (p["A"]["g_depth"][kg] + tiny)).max(initial=0.0)))
    allsame = same.all(axis=1) & np.all([p["keep"] | ~ref["seen"][:, s] for s, p in enumerate(per)], axis=0)
    keep = allsame & ref["pvalid"] & (np.asarray(got["count"]) == ref["count"])
    err = np.abs(np.asarray(got["fused"], dtype=np.float64) - ref["fused"])[keep]
    r["fused"] = float((err / (fused_majorant(ref, per)[keep] + tiny)).max(initial=0.0))
    return r


def composition32(x):
    """(the float32 composition's dict, its per-source losses, the pixels where its decisions are float64's)."""
    c32 = composition(*_args(x), mask=x["mask"], gloss=GLOSS, dtype=torch.float32)
    S = len(x["src_depths"])
    return c32, [{"loss": c32[f"loss_{s}"], "g_depth": c32[f"g_depth_{s}"]} for s in range(S)]


def measure_kappa():
    """{case: {output: {"kappa_ref", "kappa"}}}: torch's own float32 run of the composition against the float64
    one in units of the majorant, and 4 x that (the project's convention)."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        table = {}
        for name, *_ in CPU_CASES:
            x, ref, per = case_budget(name)
            c32, l32 = composition32(x)
            same = (c32["seen"] == ref["seen"]) & (c32["cons"] == ref["cons"])
            r = ratios(c32, l32, ref, per, same)
            table[name] = {key: {"kappa_ref": float(f"{v:.4g}"), "kappa": float(f"{4 * v:.4g}")} for key, v in r.items()}
        return table
    finally:
        torch.set_num_threads(nthreads)


def load_kappa():
    with open(KAPPA_JSON) as fh:
        return json.load(fh)


def kappa_for(table):
    """The kappa the checks apply per output: the largest over the measured cases."""
    return {key: max(table[name][key]["kappa"] for name in table) for key in OUTPUTS}


if __name__ == "__main__":
    t = measure_kappa()
    print(json.dumps(t, indent=1))
    if "--write" in sys.argv:
        with open(KAPPA_JSON, "w") as fh:
            json.dump(t, fh, indent=1)
            fh.write("\n")
