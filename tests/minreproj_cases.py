"""References, bounds and inputs of the minimum-reprojection loss's tests (test_minreproj_cpu.py,
test_gpu_minreproj.py):

  min_rule_fp32  the rule of include/nconv.h (nconv_photo_min_loss_*) restated in numpy on top of
                 warp_cases.rule_fp32 (the warp, the L1 terms, g_depth from g_s) and ssim_cases.ssim_fp32 (the
                 window arithmetic), every operation an explicit float32 step -- what the kernels must reproduce
                 bit for bit
  composition    the same loss composed from torch ops in whatever dtype is asked for: F.grid_sample,
                 F.avg_pool2d(3, 1), the per-pixel sum, a gather over the sources and autograd. It is FED the
                 restatement's winner plane (which also says which pixels are masked), so it is smooth in the
                 depth and the comparison needs no tie exclusion of its own
  majorants      first-order float64 majorants of the fp32 rule's error (E per source and pixel, g_depth), from
                 ssim_cases.majorants' pieces
  measure_kappa  torch's float32 run of the composition against float64 in units of the majorants;
                 `python tests/minreproj_cases.py --write` writes tests/golden/minreproj_bound_kappa.json
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import reduce_tree as RT
import ssim_cases as SC
import warp_cases as WC

f32 = np.float32
U = WC.U
KAPPA_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minreproj_bound_kappa.json")
OUTPUTS = ("E", "g_depth")
MASKED, NONE = 254, 255


# ------------------------------------------------------------------------------------------------
# the fp32 rule
# ------------------------------------------------------------------------------------------------
def _channel_sum(e):
    return e[:, 0] if e.shape[1] == 1 else (e[:, 0] + e[:, 1]) + e[:, 2]


def _error_fp32(x, y, ok, alpha, c1, c2):
    """(E, comparable, ssim dict or None) of one source: x (B, C, H, W) float32 with its validity ok (B, H, W)."""
    one, zero = f32(1.0), f32(0.0)
    with np.errstate(all="ignore"):
        tl = _channel_sum(np.abs(x - y))
        if alpha == 0:
            return tl.astype(f32), ok, None
        s = SC.ssim_fp32(x, y, c1, c2)
        t = s["t"]
        e = np.where(t < 0, zero, np.where(t > 1, one, t)).astype(f32)
        tw = _channel_sum(e)
        E = alpha * tw + (one - alpha) * tl
    assert E.dtype == f32
    return E, SC.windows(ok), s


def _take(has, E, best, comparable):
    """The replacement rule: the first comparable source, a smaller error, or a NaN over a number."""
    with np.errstate(all="ignore"):
        return comparable & (~has | (E < best) | (np.isnan(E) & ~np.isnan(best)))


def min_rule_fp32(depth, k, srcs, ms, mask=None, tgt=None, alpha=0.85, data_range=255.0, automask=True, gloss=1.0,
                  z_min=0.0, z_max=0.0):
    """A dict: winner (B, H, W) uint8 (s, 254 masked, 255 none), has, kept (bool), n_c, n_m, best, E (S, B, H, W),
    comparable (S, B, H, W), Imin, terms, error, L (float32, the stated tree) and g_depth (B, H, W) float32.
    srcs, ms: lists of S arrays; the other inputs as warp_cases.rule_fp32's."""
    S = len(srcs)
    assert 1 <= S <= 4 and len(ms) == S
    y = np.asarray(tgt, dtype=f32)
    B, C, H, W = y.shape
    alpha, gl = f32(alpha), f32(gloss)
    c1, c2 = SC.constants(data_range)
    one, two, nine, half, zero = f32(1.0), f32(2.0), f32(9.0), f32(0.5), f32(0.0)
    base = [WC.rule_fp32(depth, k, srcs[s], ms[s], mask, tgt, None, gloss, z_min, z_max) for s in range(S)]
    per = [_error_fp32(base[s]["warped"], y, base[s]["valid"], alpha, c1, c2) for s in range(S)]
    has = np.zeros((B, H, W), dtype=bool)
    best = np.zeros((B, H, W), dtype=f32)
    win = np.full((B, H, W), -1, dtype=np.int64)
    for s in range(S):
        E, comparable, _ = per[s]
        take = _take(has, E, best, comparable)
        best, win, has = np.where(take, E, best).astype(f32), np.where(take, s, win), has | take
    masked = np.zeros((B, H, W), dtype=bool)
    imin = np.zeros((B, H, W), dtype=f32)
    if automask:
        hasi = np.zeros((B, H, W), dtype=bool)
        for s in range(S):
            x = np.asarray(srcs[s], dtype=f32)
            assert x.shape == y.shape, "auto-masking needs sources of the target's size"
            I, comparable, _ = _error_fp32(x, y, np.ones((B, H, W), dtype=bool), alpha, c1, c2)
            take = _take(hasi, I, imin, comparable)
            imin, hasi = np.where(take, I, imin).astype(f32), hasi | take
        with np.errstate(all="ignore"):
            masked = has & hasi & (imin <= best)
    kept = has & ~masked
    n_c, n_m = int(has.sum()), int(masked.sum())
    terms = np.where(kept, best, zero).astype(f32)
    L = RT.loss(terms, float(C * max(n_c, 1)), RT.ROWS)
    winner = np.where(~has, NONE, np.where(masked, MASKED, win)).astype(np.uint8)
    with np.errstate(all="ignore"):
        error = np.where(kept, best / f32(C), zero).astype(f32)
        den = f32(C) * f32(max(n_c, 1))
        kl = (gl * (one - alpha)) * (one / den)
        kq = (alpha * half) * (gl * (one / den))
        g_depth = None
        for s in range(S):
            x = base[s]["warped"]
            won = winner == s
            d = x - y
            sign = np.where(d > 0, one, np.where(d < 0, f32(-1), zero)).astype(f32)
            l1 = np.where(won[:, None], kl * sign, zero).astype(f32)
            if alpha == 0:
                g_x = np.zeros_like(x)
            else:
                q = per[s][2]
                t = q["t"]
                passes = (won & per[s][1])[:, None] & (t >= 0) & (t <= 1)
                cp = (two * q["A1"]) / (nine * q["D"])
                bp = -((two * q["ssim"]) / (nine * q["B2"]))
                sm = q["ssim"] * q["mux"]
                ap = (two * ((((q["muy"] * (q["A2"] - q["A1"])) / q["D"]) - (sm / q["B1"])) + (sm / q["B2"]))) / nine
                box = lambda v: SC._seq([np.zeros_like(v)] + SC._shifts(  # noqa: E731
                    SC._pad(np.where(passes, v, zero).astype(f32)), H, W))
                SA, SB, SCc = box(ap), box(bp), box(cp)
                g_x = -(kq * ((SA + SB * x) + SCc * y))
            g_s = (l1 + g_x).astype(f32)
            t_s = WC.rule_fp32(depth, k, srcs[s], ms[s], mask, None, g_s, 1.0, z_min, z_max)["g_depth_warp"]
            g_depth = t_s if s == 0 else (g_depth + t_s).astype(f32)
    out = {"winner": winner, "has": has, "kept": kept, "masked": masked, "n_c": n_c, "n_m": n_m, "best": best,
           "E": np.stack([p[0] for p in per]), "comparable": np.stack([p[1] for p in per]), "Imin": imin,
           "terms": terms, "error": error, "L": L, "g_depth": g_depth,
           "valid": np.stack([b["valid"] for b in base])}
    assert terms.dtype == f32 and g_depth.dtype == f32 and error.dtype == f32 and isinstance(L, f32)
    return out


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def min_inputs(seed, B, C, size, src_size=None, S=2, per_image_m=True, with_mask=False, data_range=255.0):
    """ssim_cases.ssim_inputs (depth, k, tgt, mask and source 0) plus S - 1 further sources with poses of their
    own: a backward motion for the odd ones, so that the sources lose different parts of the border. A dict
    with srcs and ms (lists of S arrays) in place of src and m."""
    x = SC.ssim_inputs(seed, B, C, size, src_size, per_image_m, with_mask, data_range)
    H, W = size
    Hs, Ws = src_size or size
    g = torch.Generator().manual_seed(seed + 7919)
    ks = WC.intrinsics(Hs, Ws, 0.9 * max(W, 2) * Ws / W)
    srcs, ms = [x.pop("src")], [x.pop("m")]
    for s in range(1, S):
        srcs.append((torch.rand(B, C, Hs, Ws, generator=g).numpy() * f32(data_range)).astype(f32))
        sign = -1.0 if s % 2 else 1.0
        poses = [WC.rigid(0.004 * (b + 1) * (1 - s), -0.006 + 0.005 * s, 0.003 - 0.002 * s,
                          (0.12 + 0.05 * b - 0.2 * s, -0.04 + 0.03 * s, sign * (0.45 - 0.1 * b))) for b in range(B)]
        m = np.stack([ks @ p for p in poses]).astype(f32)
        ms.append(m if per_image_m else m[0])
    x["srcs"], x["ms"] = srcs, ms
    return x


def call_args(x):
    return (x["depth"], x["k"], x["srcs"], x["ms"], x["mask"], x["tgt"])


# ------------------------------------------------------------------------------------------------
# the torch composition, fed the winner plane
# ------------------------------------------------------------------------------------------------
def composition(depth, k, srcs, ms, mask=None, tgt=None, winner=None, alpha=0.85, data_range=255.0, gloss=1.0,
                z_min=0.0, z_max=0.0, dtype=torch.float64):
    """The loss as a user composes it from torch ops, in `dtype`: per source F.grid_sample (align_corners=True),
    F.avg_pool2d(3, 1) on the interior and the per-pixel sum E_s; then, INSTEAD of torch.min, a gather of E by
    the given winner plane (min_rule_fp32's: s, 254 masked, 255 none) and the mean over the pixels with a
    winner, differentiated by autograd. With the selection fixed the loss is smooth in the depth. Returns E
    (S, B, H, W; 0 where not comparable), comparable, g_depth and, per source, SC.composition's dict of the
    quantities the majorants need (valid, win, u, v, warped, t, jac, n_v, n_w)."""
    T = lambda a: torch.as_tensor(np.array(a)).to(dtype)  # noqa: E731
    z0, tgt = T(depth), T(tgt)
    B, H, W = z0.shape
    C = tgt.shape[1]
    S = len(srcs)
    kk = T(WC._batched(k, B, (3, 3)))
    zmax = WC.FLT_MAX if z_max == 0.0 else z_max
    pvalid = torch.isfinite(z0) & (z0 > z_min) & (z0 <= zmax)
    z = torch.where(pvalid, z0, torch.ones_like(z0)).requires_grad_(True)
    ii, jj = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    col = lambda a: a[:, None, None]  # noqa: E731
    x = (jj - col(kk[:, 0, 2])) * z / col(kk[:, 0, 0])
    y = (ii - col(kk[:, 1, 2])) * z / col(kk[:, 1, 1])
    c1, c2 = (float(v_) for v_ in SC.constants(data_range))
    pool = lambda a: F.avg_pool2d(a, 3, 1)  # noqa: E731
    Es, comps, per = [], [], []
    for s in range(S):
        src = T(srcs[s])
        Hs, Ws = src.shape[2:]
        m = T(WC._batched(ms[s], B, (3, 4)))
        abc = [col(m[:, r, 0]) * x + col(m[:, r, 1]) * y + col(m[:, r, 2]) * z + col(m[:, r, 3]) for r in range(3)]
        front = abc[2] > 0
        c = torch.where(front, abc[2], torch.ones_like(z))
        u, v = abc[0] / c, abc[1] / c
        valid = pvalid & front & (u >= 0) & (u <= Ws - 1) & (v >= 0) & (v <= Hs - 1)
        if mask is not None:
            valid = valid & torch.as_tensor(np.asarray(mask) != 0)
        gx, gy = 2 * u / max(Ws - 1, 1) - 1, 2 * v / max(Hs - 1, 1) - 1
        grid = torch.where(valid[..., None], torch.stack((gx, gy), dim=-1), torch.zeros(B, H, W, 2, dtype=dtype))
        vf = valid.to(dtype)[:, None]
        warped = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * vf
        tl = ((warped - tgt).abs() * vf).sum(1)
        tt = torch.full((B, C, H, W), 0.5, dtype=dtype)
        win = torch.zeros(B, H, W, dtype=torch.bool)
        tw = torch.zeros(B, H, W, dtype=dtype)
        if alpha != 0 and H >= 3 and W >= 3:
            mu_x, mu_y = pool(warped), pool(tgt)
            s_x, s_y = pool(warped * warped) - mu_x * mu_x, pool(tgt * tgt) - mu_y * mu_y
            s_xy = pool(warped * tgt) - mu_x * mu_y
            ssim = ((2 * mu_x * mu_y + c1) * (2 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_x + s_y + c2))
            t = (1 - ssim) / 2
            wv = -F.max_pool2d(-vf, 3, 1)                      # the product of the nine validities
            tw = F.pad((torch.clamp(t, 0, 1) * wv).sum(1), (1, 1, 1, 1))
            tt = F.pad(t.detach(), (1, 1, 1, 1), value=0.5)
            win = F.pad(wv[:, 0] > 0.5, (1, 1, 1, 1))
        comparable = valid if alpha == 0 else win
        E = tl if alpha == 0 else alpha * tw + (1 - alpha) * tl
        Es.append(E * comparable.to(dtype))
        comps.append(comparable)
        jac = [torch.autograd.grad(warped[:, ch].sum(), z, retain_graph=True)[0].numpy() for ch in range(C)]
        per.append({"valid": valid.numpy(), "win": win.numpy(), "u": u.detach().numpy(), "v": v.detach().numpy(),
                    "warped": warped.detach().numpy(), "t": tt.numpy(), "jac": np.stack(jac, axis=1)})
    E = torch.stack(Es)
    wn = torch.as_tensor(np.asarray(winner).astype(np.int64))
    kept = wn < S
    n_c = int((wn != NONE).sum())
    best = torch.gather(E, 0, torch.where(kept, wn, torch.zeros_like(wn))[None])[0]
    loss = (best * kept.to(dtype)).sum() / (C * max(n_c, 1))
    (g,) = torch.autograd.grad(loss * gloss, z)
    for p in per:
        p["n_v"] = p["n_w"] = n_c
    return {"E": E.detach().numpy(), "comparable": torch.stack(comps).numpy(), "loss": loss.item(), "n_c": n_c,
            "g_depth": g.numpy(), "per": per}


# ------------------------------------------------------------------------------------------------
# majorants and the comparable pixels
# ------------------------------------------------------------------------------------------------
def majorants(x, ref, alpha, gloss=1.0):
    """{"E": (S, B, H, W), "g_depth": (B, H, W)} float64 majorants of the fp32 rule's first-order error against
    the float64 reference `ref` (composition's dict), from ssim_cases.majorants and warp_cases.majorants per
    source (with both of their denominators this loss's C max(n_c, 1)):
      E        alpha A(terms_w) + (1 - alpha) (sum_ch A_warped + 3 U tl) + 3 U |E|: the two products and the sum
      g_depth  the sum over the sources of ssim_cases' A_g, which bounds the error of ALL of a source's windows
               and of the L1 sign of ALL its valid pixels -- the windows and pixels that source did not win add
               nothing here, so this is a majorant with room -- plus U |partial sum| per addition."""
    S = len(x["srcs"])
    A_E, A_g = [], 0.0
    for s in range(S):
        p = ref["per"][s]
        xin = {"depth": x["depth"], "k": x["k"], "src": x["srcs"][s], "m": x["ms"][s], "tgt": x["tgt"]}
        A_w, _ = WC.majorants(x["depth"], x["k"], x["srcs"][s], x["ms"][s], p["valid"])
        tl = np.abs(p["warped"] - x["tgt"]).sum(1)
        a_l1 = A_w.sum(1) + 3 * U * tl
        if alpha == 0:
            A_E.append(np.where(ref["comparable"][s], a_l1 + U * tl, 0.0))
            _, a_g = WC.majorants(x["depth"], x["k"], x["srcs"][s], x["ms"][s], p["valid"],
                                  np.full(x["tgt"].shape, gloss / (x["tgt"].shape[1] * max(ref["n_c"], 1))))
        else:
            m = SC.majorants(xin, p, alpha, x["data_range"], gloss)
            a = alpha * m["terms_w"] + (1 - alpha) * a_l1 + 3 * U * np.abs(ref["E"][s])
            A_E.append(np.where(ref["comparable"][s], a, 0.0))
            a_g = m["g_depth"]
        A_g = A_g + a_g
    return {"E": np.stack(A_E), "g_depth": A_g + (S - 1) * U * np.abs(ref["g_depth"])}


def comparable(x, ref, alpha):
    """({output: keep}, {output: omitted share}): E where the source is comparable; g_depth at the pixels that
    are, for every source in which they are valid, away from that source's discontinuities
    (ssim_cases.comparable: integer crossings of u and v, x == y, clamp edges of the windows that hold them)."""
    S = len(x["srcs"])
    anyv = np.zeros(ref["g_depth"].shape, dtype=bool)
    keep = np.ones(ref["g_depth"].shape, dtype=bool)
    for s in range(S):
        p = ref["per"][s]
        ks, _ = SC.comparable(p, {"tgt": x["tgt"]}, alpha)
        keep &= ~p["valid"] | ks["g_depth"]
        anyv |= p["valid"]
    keep &= anyv
    return ({"E": ref["comparable"], "g_depth": keep},
            {"E": 0.0, "g_depth": 1.0 - keep.sum() / max(int(anyv.sum()), 1)})


def identity64(x, alpha):
    """(I (S, B, H, W), A_I) in float64: the unwarped sources' errors and the majorant of the fp32 rule's error
    of them (the window arithmetic alone, ssim_cases._chain with an exact x; the L1 sum's roundings); inf where
    I is not defined (the one-pixel frame at alpha != 0)."""
    y = np.asarray(x["tgt"], dtype=np.float64)
    B, C, H, W = y.shape
    c1, c2 = (float(v) for v in SC.constants(x["data_range"]))
    inner = SC.windows(np.ones((B, H, W), dtype=bool))
    I, A = [], []
    for src in x["srcs"]:
        xs = np.asarray(src, dtype=np.float64)
        tl = np.abs(xs - y).sum(1)
        if alpha == 0:
            I.append(tl), A.append(4 * U * tl)
            continue
        with np.errstate(all="ignore"):
            ch = SC._chain(xs, y, np.zeros_like(xs), c1, c2)
            t = np.clip(0.5 * (1 - ch["ssim"]), 0, 1)
            tw = t.sum(1)
            a_tw = (0.5 * ch["e_ssim"] + 0.5 * U * np.abs(1 - ch["ssim"])).sum(1) + 2 * U * tw
            e = alpha * tw + (1 - alpha) * tl
            a = alpha * a_tw + (1 - alpha) * 4 * U * tl + 3 * U * np.abs(e)
        I.append(np.where(inner, e, np.inf)), A.append(np.where(inner, a, np.inf))
    return np.stack(I), np.stack(A)


# (name, seed, B, C, size, S, per_image_m, with_mask, data_range, automask): frames in [0, R]
CPU_CASES = [("17x65_c3_s2_r255", 1, 2, 3, (17, 65), 2, True, False, 255.0, True),
             ("45x67_c1_s3_shared_m_mask_r1", 2, 2, 1, (45, 67), 3, False, True, 1.0, True),
             ("64x96_c3_s2_r255_plain", 3, 2, 3, (64, 96), 2, True, True, 255.0, False)]
ALPHA = 0.85


def case_inputs(name):
    _, seed, B, C, size, S, per_image, with_mask, R, _ = next(c for c in CPU_CASES if c[0] == name)
    return min_inputs(seed, B, C, size, None, S, per_image, with_mask, R)


def case_budget(name):
    """(inputs, the fp32 rule, float64 reference fed the rule's winner plane, keep masks, omitted shares,
    majorants) of a CPU case."""
    automask = next(c for c in CPU_CASES if c[0] == name)[9]
    x = case_inputs(name)
    rule = min_rule_fp32(*call_args(x), alpha=ALPHA, data_range=x["data_range"], automask=automask)
    ref = composition(*call_args(x), winner=rule["winner"], alpha=ALPHA, data_range=x["data_range"])
    keep, omit = comparable(x, ref, ALPHA)
    return x, rule, ref, keep, omit, majorants(x, ref, ALPHA)


def ratios(got, ref, keep, A):
    """max over the kept elements of |got - ref| / A, per output."""
    out = {}
    for key in OUTPUTS:
        err = np.abs(np.asarray(got[key], dtype=np.float64) - ref[key])[keep[key]]
        out[key] = float((err / (A[key][keep[key]] + 1e-300)).max())
    return out


def measure_kappa():
    """{case: {output: {"kappa_ref", "kappa"}}}: torch's own float32 run of the composition (fed the same winner
    plane) against the float64 one in units of the majorant, and 4 x that (the project's convention): the
    procedure of ssim_cases.measure_kappa."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        table = {}
        for name, *_ in CPU_CASES:
            x, rule, ref, keep, omit, A = case_budget(name)
            got = composition(*call_args(x), winner=rule["winner"], alpha=ALPHA, data_range=x["data_range"],
                              dtype=torch.float32)
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
