"""References, bounds and inputs of the SSIM photometric loss's tests (test_ssim_cpu.py, test_gpu_ssim.py):

  rule_fp32      the rule of include/nconv.h (nconv_photo_ssim_loss_*) restated in numpy on top of
                 warp_cases.rule_fp32 (the warp, the L1 terms, g_depth from g_s), every operation an explicit
                 float32 step -- what the kernels must reproduce bit for bit
  composition    the same loss composed from torch ops in whatever dtype is asked for: F.grid_sample
                 (align_corners=True), F.avg_pool2d(3, 1) on the interior, the window-validity product and the
                 two masked means; differentiated by autograd (float64: the reference; float32: what kappa is
                 measured from)
  majorants      first-order float64 majorants of the fp32 rule's error per element (Lw's terms, g_depth)
  measure_kappa  torch's float32 run of the composition against float64 in units of the majorants;
                 `python tests/ssim_cases.py --write` writes tests/golden/ssim_bound_kappa.json
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import reduce_tree as RT
import warp_cases as WC

f32 = np.float32
U = WC.U
EDGE = WC.EDGE
KAPPA_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_bound_kappa.json")
OUTPUTS = ("terms_w", "g_depth")


def constants(data_range):
    """c1, c2 formed in double and rounded once to fp32."""
    R = float(data_range)
    return f32((0.01 * R) ** 2), f32((0.03 * R) ** 2)


def _shifts(p, H, W):
    """The nine (B, .., H, W) views of a plane padded by one pixel, in raster order."""
    return [p[..., di:di + H, dj:dj + W] for di in range(3) for dj in range(3)]


def _seq(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _pad(a, value=0):
    width = [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)]
    return np.pad(a, width, constant_values=value)


def windows(valid):
    """(B, H, W) bool: all nine pixels of the 3 x 3 neighbourhood valid, outside the image not valid."""
    H, W = valid.shape[-2:]
    return np.logical_and.reduce(_shifts(_pad(valid, False), H, W))


# ------------------------------------------------------------------------------------------------
# the fp32 rule
# ------------------------------------------------------------------------------------------------
def ssim_fp32(x, y, c1, c2):
    """The window arithmetic of the rule on (B, C, H, W) float32 planes, every pixel taken as a centre (the
    planes padded by zeros: a centre without a window computes garbage that the caller masks). A dict of
    float32 arrays: mux, muy, A1, A2, B1, B2, D, ssim, t."""
    H, W = x.shape[-2:]
    xs, ys = _shifts(_pad(x), H, W), _shifts(_pad(y), H, W)
    nine, two, one, half = f32(9.0), f32(2.0), f32(1.0), f32(0.5)
    with np.errstate(all="ignore"):
        Sx, Sy = _seq(xs), _seq(ys)
        Sxx, Syy = _seq([a * a for a in xs]), _seq([b * b for b in ys])
        Sxy = _seq([a * b for a, b in zip(xs, ys)])
        mux, muy = Sx / nine, Sy / nine
        mxx, myy, mxy = mux * mux, muy * muy, mux * muy
        vx, vy, vxy = Sxx / nine - mxx, Syy / nine - myy, Sxy / nine - mxy
        A1, A2 = two * mxy + c1, two * vxy + c2
        B1, B2 = (mxx + myy) + c1, (vx + vy) + c2
        D = B1 * B2
        ssim = (A1 * A2) / D
        t = (one - ssim) * half
    out = {"mux": mux, "muy": muy, "A1": A1, "A2": A2, "B1": B1, "B2": B2, "D": D, "ssim": ssim, "t": t}
    assert all(v.dtype == f32 for v in out.values())
    return out


def rule_fp32(depth, k, src, m, mask=None, tgt=None, alpha=0.85, data_range=255.0, gloss=1.0, z_min=0.0, z_max=0.0):
    """A dict: valid, win (B, H, W) bool, n_v, n_w, terms (the L1 terms), terms_w (the SSIM terms), Lv, Lw, L
    (float32, summed in the stated tree) and g_depth (B, H, W) float32. Inputs as warp_cases.rule_fp32's."""
    base = WC.rule_fp32(depth, k, src, m, mask, tgt, None, gloss, z_min, z_max)
    valid, x = base["valid"], base["warped"]
    y = np.asarray(tgt, dtype=f32)
    B, C, H, W = x.shape
    alpha, gl = f32(alpha), f32(gloss)
    c1, c2 = constants(data_range)
    one, two, nine, half, zero = f32(1.0), f32(2.0), f32(9.0), f32(0.5), f32(0.0)
    win = windows(valid)
    n_v, n_w = int(valid.sum()), int(win.sum())
    s = ssim_fp32(x, y, c1, c2)
    with np.errstate(all="ignore"):
        t = s["t"]
        e = np.where(t < 0, zero, np.where(t > 1, one, t)).astype(f32)
        termw = e[:, 0] if C == 1 else (e[:, 0] + e[:, 1]) + e[:, 2]
        terms_w = np.where(win, termw, zero).astype(f32)
        passes = win[:, None] & (t >= 0) & (t <= 1)
        cp = (two * s["A1"]) / (nine * s["D"])
        bp = -((two * s["ssim"]) / (nine * s["B2"]))
        sm = s["ssim"] * s["mux"]
        ap = (two * ((((s["muy"] * (s["A2"] - s["A1"])) / s["D"]) - (sm / s["B1"])) + (sm / s["B2"]))) / nine
        box = lambda v: _seq([np.zeros_like(v)] + _shifts(_pad(np.where(passes, v, zero).astype(f32)), H, W))  # noqa: E731
        SA, SB, SC = box(ap), box(bp), box(cp)
        den_v, den_w = f32(C) * f32(max(n_v, 1)), f32(C) * f32(max(n_w, 1))
        kl = (gl * (one - alpha)) * (one / den_v)
        kq = (alpha * half) * (gl * (one / den_w))
        d = x - y
        sign = np.where(d > 0, one, np.where(d < 0, f32(-1), zero)).astype(f32)
        g_x = -(kq * ((SA + SB * x) + SC * y))
        g_s = (kl * sign + g_x).astype(f32)
    g_depth = WC.rule_fp32(depth, k, src, m, mask, None, g_s, 1.0, z_min, z_max)["g_depth_warp"]
    Lv = RT.loss(base["terms"], float(base["den"]), RT.ROWS)
    Lw = RT.loss(terms_w, float(C * max(n_w, 1)), RT.ROWS)
    L = alpha * Lw + (one - alpha) * Lv
    out = {"valid": valid, "win": win, "n_v": n_v, "n_w": n_w, "terms": base["terms"], "terms_w": terms_w,
           "Lv": Lv, "Lw": Lw, "L": L, "g_depth": g_depth, "u": base["u"], "v": base["v"], "warped": x, "t": t,
           "g_depth_photo": base["g_depth_photo"], "den": base["den"]}
    assert terms_w.dtype == f32 and g_depth.dtype == f32 and isinstance(L, f32)
    return out


# ------------------------------------------------------------------------------------------------
# the torch composition
# ------------------------------------------------------------------------------------------------
def composition(depth, k, src, m, mask=None, tgt=None, alpha=0.85, data_range=255.0, gloss=1.0, z_min=0.0,
                z_max=0.0, dtype=torch.float64):
    """The loss as a user composes it from torch ops, in `dtype`; g_depth and jac (d warped / d z per channel)
    from autograd. Inputs as rule_fp32's."""
    T = lambda a: torch.as_tensor(np.array(a)).to(dtype)  # noqa: E731
    z0, src, tgt = T(depth), T(src), T(tgt)
    B, H, W = z0.shape
    C, Hs, Ws = src.shape[1:]
    k = T(WC._batched(k, B, (3, 3)))
    m = T(WC._batched(m, B, (3, 4)))
    zmax = WC.FLT_MAX if z_max == 0.0 else z_max
    pvalid = torch.isfinite(z0) & (z0 > z_min) & (z0 <= zmax)
    z = torch.where(pvalid, z0, torch.ones_like(z0)).requires_grad_(True)
    ii, jj = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    col = lambda a: a[:, None, None]  # noqa: E731
    x = (jj - col(k[:, 0, 2])) * z / col(k[:, 0, 0])
    y = (ii - col(k[:, 1, 2])) * z / col(k[:, 1, 1])
    abc = [col(m[:, r, 0]) * x + col(m[:, r, 1]) * y + col(m[:, r, 2]) * z + col(m[:, r, 3]) for r in range(3)]
    front = abc[2] > 0
    c = torch.where(front, abc[2], torch.ones_like(z))
    u, v = abc[0] / c, abc[1] / c
    valid = pvalid & front & (u >= 0) & (u <= Ws - 1) & (v >= 0) & (v <= Hs - 1)
    if mask is not None:
        valid = valid & torch.as_tensor(np.asarray(mask) != 0)
    gx = 2 * u / max(Ws - 1, 1) - 1
    gy = 2 * v / max(Hs - 1, 1) - 1
    grid = torch.where(valid[..., None], torch.stack((gx, gy), dim=-1), torch.zeros(B, H, W, 2, dtype=dtype))
    vf = valid.to(dtype)[:, None]
    warped = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * vf
    n_v = int(valid.sum())
    loss_v = ((warped - tgt).abs() * vf).sum() / (C * max(n_v, 1))
    terms_w = torch.zeros(B, H, W, dtype=dtype)
    tt = torch.full((B, C, H, W), 0.5, dtype=dtype)
    win = torch.zeros(B, H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        c1, c2 = (float(v_) for v_ in constants(data_range))
        pool = lambda a: F.avg_pool2d(a, 3, 1)  # noqa: E731
        mu_x, mu_y = pool(warped), pool(tgt)
        s_x, s_y, s_xy = pool(warped * warped) - mu_x * mu_x, pool(tgt * tgt) - mu_y * mu_y, pool(warped * tgt) - mu_x * mu_y
        ssim = ((2 * mu_x * mu_y + c1) * (2 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_x + s_y + c2))
        t = (1 - ssim) / 2
        wv = -F.max_pool2d(-vf, 3, 1)                      # the product of the nine validities
        e = torch.clamp(t, 0, 1) * wv
        terms_w = F.pad(e.sum(1), (1, 1, 1, 1))
        tt = F.pad(t.detach(), (1, 1, 1, 1), value=0.5)
        win = F.pad(wv[:, 0] > 0.5, (1, 1, 1, 1))
    n_w = int(win.sum())
    loss_w = terms_w.sum() / (C * max(n_w, 1))
    loss = alpha * loss_w + (1 - alpha) * loss_v
    (g,) = torch.autograd.grad(loss * gloss, z, retain_graph=True)
    jac = [torch.autograd.grad(warped[:, ch].sum(), z, retain_graph=True)[0].numpy() for ch in range(C)]
    return {"valid": valid.numpy(), "win": win.numpy(), "n_v": n_v, "n_w": n_w, "u": u.detach().numpy(),
            "v": v.detach().numpy(), "warped": warped.detach().numpy(), "terms_w": terms_w.detach().numpy(),
            "t": tt.numpy(), "loss": loss.item(), "loss_v": loss_v.item(), "loss_w": loss_w.item(),
            "g_depth": g.numpy(), "jac": np.stack(jac, axis=1)}


# ------------------------------------------------------------------------------------------------
# majorants
# ------------------------------------------------------------------------------------------------
def _chain(x, y, Aw, c1, c2):
    """Float64 window quantities of every centre and first-order error majorants of the fp32 rule's, given the
    absolute error majorant Aw of x (y is exact). With m the mean over the window:
      a sequential sum of nine terms and the division by 9      -> 9 U m|.| (10 U for sums of products)
      mux: m(Aw) + 9 U m|x|            Exx = Sxx / 9: 2 m(|x| Aw) + 10 U m(x^2)   Exy: m(|y| Aw) + 10 U m|xy|
      a product p q -> |q| e_p + |p| e_q + U |p q|;  a sum or difference -> e_p + e_q + U |result|
      a quotient p / q -> e_p / |q| + |p / q| (e_q / |q| + U)
    applied operation by operation to vx, vy, vxy, A1, A2, B1, B2, D, ssim and to a, b, c in the header's order.
    Every path of the input error is taken with its worst sign (no cancellation between paths is assumed)."""
    H, W = x.shape[-2:]
    mean = lambda a: sum(_shifts(_pad(a), H, W)) / 9.0  # noqa: E731
    with np.errstate(all="ignore"):
        mux, muy = mean(x), mean(y)
        e_mux, e_muy = mean(Aw) + 9 * U * mean(np.abs(x)), 9 * U * mean(np.abs(y))
        Exx, Eyy, Exy = mean(x * x), mean(y * y), mean(x * y)
        e_Exx = 2 * mean(np.abs(x) * Aw) + 10 * U * Exx
        e_Eyy = 10 * U * Eyy
        e_Exy = mean(np.abs(y) * Aw) + 10 * U * mean(np.abs(x * y))
        mxx, myy, mxy = mux * mux, muy * muy, mux * muy
        e_mxx, e_myy = 2 * np.abs(mux) * e_mux + U * mxx, 2 * np.abs(muy) * e_muy + U * myy
        e_mxy = np.abs(muy) * e_mux + np.abs(mux) * e_muy + U * np.abs(mxy)
        vx, vy, vxy = Exx - mxx, Eyy - myy, Exy - mxy
        e_vx, e_vy = e_Exx + e_mxx + U * np.abs(vx), e_Eyy + e_myy + U * np.abs(vy)
        e_vxy = e_Exy + e_mxy + U * np.abs(vxy)
        A1, A2, B1, B2 = 2 * mxy + c1, 2 * vxy + c2, mxx + myy + c1, vx + vy + c2
        e_A1, e_A2 = 2 * e_mxy + U * np.abs(A1), 2 * e_vxy + U * np.abs(A2)
        e_B1 = e_mxx + e_myy + U * (mxx + myy) + U * np.abs(B1)
        e_B2 = e_vx + e_vy + U * np.abs(vx + vy) + U * np.abs(B2)
        D = B1 * B2
        e_D = np.abs(B2) * e_B1 + np.abs(B1) * e_B2 + U * np.abs(D)
        N = A1 * A2
        e_N = np.abs(A2) * e_A1 + np.abs(A1) * e_A2 + U * np.abs(N)
        ssim = N / D
        e_ssim = e_N / np.abs(D) + np.abs(ssim) * (e_D / np.abs(D) + U)
        cp = 2 * A1 / (9 * D)
        e_c = (2 * e_A1) / np.abs(9 * D) + np.abs(cp) * (e_D / np.abs(D) + 3 * U)
        bp = -2 * ssim / (9 * B2)
        e_b = (2 * e_ssim) / np.abs(9 * B2) + np.abs(bp) * (e_B2 / np.abs(B2) + 3 * U)
        dA = A2 - A1
        e_dA = e_A1 + e_A2 + U * np.abs(dA)
        p1 = muy * dA / D
        e_p1 = (e_muy * np.abs(dA) + np.abs(muy) * e_dA + U * np.abs(muy * dA)) / np.abs(D) + \
            np.abs(p1) * (e_D / np.abs(D) + U)
        sm = ssim * mux
        e_sm = e_ssim * np.abs(mux) + np.abs(ssim) * e_mux + U * np.abs(sm)
        p2, p3 = sm / B1, sm / B2
        e_p2 = e_sm / np.abs(B1) + np.abs(p2) * (e_B1 / np.abs(B1) + U)
        e_p3 = e_sm / np.abs(B2) + np.abs(p3) * (e_B2 / np.abs(B2) + U)
        ap = 2 * (p1 - p2 + p3) / 9
        e_a = 2 * (e_p1 + e_p2 + e_p3 + U * np.abs(p1 - p2) + U * np.abs(p1 - p2 + p3)) / 9 + 2 * U * np.abs(ap)
    return {"ssim": ssim, "e_ssim": e_ssim, "a": ap, "b": bp, "c": cp, "e_a": e_a, "e_b": e_b, "e_c": e_c}


def majorants(x_in, ref, alpha, data_range, gloss=1.0):
    """{"terms_w": (B, H, W), "g_depth": (B, H, W)} float64 majorants of the fp32 rule's first-order error
    against the float64 reference `ref` (composition's dict) for the inputs x_in (warp_inputs' dict):
      terms_w  0.5 (sum_q |d ssim / d x_q| A_warped(q) + the window arithmetic's own error (_chain with Aw = 0))
               + 0.5 U |1 - ssim| per channel, + 2 U term for the channel sums
      g_depth  warp_cases.majorants' A_g for the reference's g_s (the error of the warp's own derivative), plus
               sum_ch e(g_s[ch]) |d warped[ch] / d z|, with
               e(SA) = sum over the windows of e_a + 9 U sum |a|, likewise SB, SC (a, b, c by _chain with Aw)
               e(g_x) = kq (e(SA) + e(SB) |x| + |SB| A_warped + e(SC) |y| + U (|SB x| + |SC y| + |SA + SB x| + |inner|))
                        + 4 U |g_x|
               e(g_s) = e(g_x) + 3 U |kl| + U |g_s|
    0 where the reference has no window (terms_w) or the pixel is not valid (g_depth)."""
    valid, win = ref["valid"], ref["win"]
    x, y = ref["warped"], np.asarray(x_in["tgt"], dtype=np.float64)
    B, C, H, W = x.shape
    c1, c2 = (float(v) for v in constants(data_range))
    Aw, _ = WC.majorants(x_in["depth"], x_in["k"], x_in["src"], x_in["m"], valid)
    own, full = _chain(x, y, np.zeros_like(x), c1, c2), _chain(x, y, Aw, c1, c2)
    w4 = np.broadcast_to(win[:, None], x.shape)
    t = 0.5 * (1 - full["ssim"])
    passes = w4 & (t >= 0) & (t <= 1)
    z = lambda a: np.where(passes, a, 0.0)  # noqa: E731
    box = lambda a: sum(_shifts(_pad(z(a)), H, W))  # noqa: E731
    with np.errstate(all="ignore"):
        # d ssim_p / d x_q summed over q with A_warped(q): q = p + (di, dj)
        xs, ys, As = _shifts(_pad(x), H, W), _shifts(_pad(y), H, W), _shifts(_pad(Aw), H, W)
        prop = sum(np.abs(full["a"] + full["b"] * xq + full["c"] * yq) * Aq for xq, yq, Aq in zip(xs, ys, As))
        per = 0.5 * (prop + own["e_ssim"]) + 0.5 * U * np.abs(1 - full["ssim"])
        A_t = np.where(win, per.sum(1) + 2 * U * np.clip(t, 0, 1).sum(1), 0.0)
        SA, SB, SC = box(full["a"]), box(full["b"]), box(full["c"])
        e_SA = box(full["e_a"]) + 9 * U * box(np.abs(full["a"]))
        e_SB = box(full["e_b"]) + 9 * U * box(np.abs(full["b"]))
        e_SC = box(full["e_c"]) + 9 * U * box(np.abs(full["c"]))
        n_v, n_w = ref["n_v"], ref["n_w"]
        kl = gloss * (1 - alpha) / (C * max(n_v, 1))
        kq = alpha * 0.5 * gloss / (C * max(n_w, 1))
        inner = SA + SB * x + SC * y
        g_x = -kq * inner
        g_s = kl * np.sign(x - y) + g_x
        e_gx = kq * (e_SA + e_SB * np.abs(x) + np.abs(SB) * Aw + e_SC * np.abs(y)
                     + U * (np.abs(SB * x) + np.abs(SC * y) + np.abs(SA + SB * x) + np.abs(inner))) + 4 * U * np.abs(g_x)
        e_gs = e_gx + 3 * U * abs(kl) + U * np.abs(g_s)
        _, A_warp = WC.majorants(x_in["depth"], x_in["k"], x_in["src"], x_in["m"], valid, np.abs(g_s))
        A_g = np.where(valid, A_warp + (e_gs * np.abs(ref["jac"])).sum(1), 0.0)
    return {"terms_w": A_t, "g_depth": A_g}


def comparable(ref, x_in, alpha):
    """The pixels away from the gradient's discontinuities: valid, the pixel's own u and v farther than EDGE from
    every integer, |x - y| >= EDGE in every channel (the L1 sign; alpha < 1), and no window that holds the pixel
    with t within EDGE of the clamp's edges 0 and 1. Returns ({output: keep}, {output: omitted share})."""
    valid, win = ref["valid"], ref["win"]
    H, W = valid.shape[-2:]
    near = lambda w: np.abs(w - np.rint(w)) < EDGE  # noqa: E731
    keep = valid & ~near(ref["u"]) & ~near(ref["v"])
    if alpha < 1:
        keep = keep & (np.abs(ref["warped"] - x_in["tgt"]).min(axis=1) >= EDGE)
    t = ref["t"]
    edge = (win[:, None] & ((np.abs(t) < EDGE) | (np.abs(t - 1) < EDGE))).any(axis=1)
    keep = keep & ~np.logical_or.reduce(_shifts(_pad(edge, False), H, W))
    return ({"terms_w": win, "g_depth": keep},
            {"terms_w": 0.0, "g_depth": 1.0 - keep.sum() / max(int(valid.sum()), 1)})


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
# (name, seed, B, C, size, src_size, per_image_m, with_mask, data_range): frames in [0, R]
CPU_CASES = [("17x65_from_19x70_c3_r255", 1, 2, 3, (17, 65), (19, 70), True, False, 255.0),
             ("45x67_c1_shared_m_mask_r1", 2, 2, 1, (45, 67), None, False, True, 1.0),
             ("64x96_c3_r255", 3, 2, 3, (64, 96), None, True, True, 255.0)]
ALPHA = 0.85


def ssim_inputs(seed, B, C, size, src_size=None, per_image_m=True, with_mask=False, data_range=1.0):
    """warp_cases.warp_inputs with the frames scaled to [0, data_range]; plus data_range."""
    x = WC.warp_inputs(seed, B, C, size, src_size, per_image_m, with_mask)
    x["src"] = (x["src"] * f32(data_range)).astype(f32)
    x["tgt"] = (x["tgt"] * f32(data_range)).astype(f32)
    x["data_range"] = float(data_range)
    return x


def call_args(x):
    return (x["depth"], x["k"], x["src"], x["m"], x["mask"], x["tgt"])


def case_inputs(name):
    _, seed, B, C, size, src_size, per_image, with_mask, R = next(c for c in CPU_CASES if c[0] == name)
    return ssim_inputs(seed, B, C, size, src_size, per_image, with_mask, R)


def case_budget(name):
    """(inputs, float64 reference, keep masks, omitted shares, majorants) of a CPU case."""
    x = case_inputs(name)
    ref = composition(*call_args(x), alpha=ALPHA, data_range=x["data_range"])
    keep, omit = comparable(ref, x, ALPHA)
    return x, ref, keep, omit, majorants(x, ref, ALPHA, x["data_range"])


def ratios(got, ref, keep, A):
    """max over the kept elements of |got - ref| / A, per output."""
    out = {}
    for key in OUTPUTS:
        err = np.abs(np.asarray(got[key], dtype=np.float64) - ref[key])[keep[key]]
        out[key] = float((err / (A[key][keep[key]] + 1e-300)).max())
    return out


def measure_kappa():
    """{case: {output: {"kappa_ref", "kappa"}}}: torch's own float32 run of the composition against the
    float64 one in units of the majorant, and 4 x that (the project's convention)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        table = {}
        for name, *_ in CPU_CASES:
            x, ref, keep, omit, A = case_budget(name)
            got = composition(*call_args(x), alpha=ALPHA, data_range=x["data_range"], dtype=torch.float32)
            r = ratios(got, ref, keep, A)
            table[name] = {key: {"kappa_ref": float(f"{v:.4g}"), "kappa": float(f"{4 * v:.4g}")} for key, v in r.items()}
        return table
    finally:
        torch.set_num_threads(n)


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
