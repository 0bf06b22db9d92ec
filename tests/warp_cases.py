"""References, bounds and inputs of the view-warp tests (test_warp_cpu.py, test_gpu_warp.py):

  rule_fp32      the rule of include/nconv.h (nconv_view_warp_*, nconv_photo_loss_*) restated in numpy, every
                 operation an explicit float32 step -- what the kernels must reproduce bit for bit
  composition    the same term composed from torch ops in whatever dtype is asked for: a meshgrid, the matrix
                 product, F.grid_sample(align_corners=True) on normalised coordinates and a masked mean;
                 differentiated by autograd (float64: the reference; float32: what kappa is measured from)
  majorants      first-order float64 majorants of the fp32 rule's error per element (warped, g_depth)
  comparable     the pixels away from the bilinear gradient's discontinuities
  loss_bound     the summation bound of the fused loss against the float64 sum of its own fp32 terms
  measure_kappa  torch's float32 run of the composition against float64 in units of the majorants;
                 `python tests/warp_cases.py --write` writes tests/golden/warp_bound_kappa.json
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
U = 2.0 ** -24                     # the unit round-off of fp32
TILE_TERMS = 16 * 64               # the terms of one fp32 partial (view_warp.hip: one 16 x 64 tile per workgroup)
FLT_MAX = float(np.finfo(np.float32).max)
EDGE = 1e-3                        # pixels whose float64 u or v is this close to an integer or the border are left out
KAPPA_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_bound_kappa.json")


# ------------------------------------------------------------------------------------------------
# the fp32 rule
# ------------------------------------------------------------------------------------------------
def _batched(x, B, shape):
    x = np.asarray(x, dtype=f32)
    return np.broadcast_to(x, (B, *shape)) if x.ndim == 2 else x


def rule_fp32(depth, k, src, m, mask=None, tgt=None, g_warped=None, gloss=1.0, z_min=0.0, z_max=0.0):
    """A dict of float32 arrays: warped (B, C, H, W), valid (B, H, W) bool, u, v, and, with g_warped,
    g_depth_warp (B, H, W); with tgt, terms (B, H, W), n_v, den and g_depth_photo. depth (B, H, W), k (3, 3)
    or (B, 3, 3), src (B, C, Hs, Ws), m (3, 4) or (B, 3, 4), mask (B, H, W) or None, tgt (B, C, H, W)."""
    z = np.asarray(depth, dtype=f32)
    src = np.asarray(src, dtype=f32)
    B, H, W = z.shape
    C, Hs, Ws = src.shape[1:]
    k, m = _batched(k, B, (3, 3)), _batched(m, B, (3, 4))
    col = lambda a: np.asarray(a, dtype=f32)[:, None, None]  # noqa: E731
    fx, fy, cx, cy = col(k[:, 0, 0]), col(k[:, 1, 1]), col(k[:, 0, 2]), col(k[:, 1, 2])
    M = [[col(m[:, r, q]) for q in range(4)] for r in range(3)]
    jj = np.arange(W, dtype=f32)[None, None, :]
    ii = np.arange(H, dtype=f32)[None, :, None]
    one = f32(1.0)
    with np.errstate(all="ignore"):
        tx = jj - cx
        ty = ii - cy
        x = (tx * z) / fx
        y = (ty * z) / fy
        zmax = f32(FLT_MAX) if z_max == 0.0 else f32(z_max)
        pvalid = (z > f32(z_min)) & (z <= zmax)

        def dot(r):
            return ((r[0] * x + r[1] * y) + r[2] * z) + r[3]

        a, bb, c = dot(M[0]), dot(M[1]), dot(M[2])
        u = a / c
        v = bb / c
        valid = pvalid & (c > 0) & (u >= 0) & (u <= f32(Ws - 1)) & (v >= 0) & (v <= f32(Hs - 1))
        if mask is not None:
            valid = valid & (np.asarray(mask) != 0)
        us, vs = np.where(valid, u, f32(0)), np.where(valid, v, f32(0))
        fu, fv = np.floor(us), np.floor(vs)
        j0, i0 = fu.astype(np.int64), fv.astype(np.int64)
        j1, i1 = np.minimum(j0 + 1, Ws - 1), np.minimum(i0 + 1, Hs - 1)
        wu, wv = us - fu, vs - fv
        w0u, w0v = one - wu, one - wv
        # the derivatives of u and v with respect to z
        X = tx / fx + np.zeros_like(z)
        Y = ty / fy + np.zeros_like(z)
        ap, bp, cp = ((M[r][0] * X + M[r][1] * Y) + M[r][2] for r in range(3))
        du = (ap - u * cp) / c
        dv = (bp - v * cp) / c
        bi = np.arange(B)[:, None, None]
        out = {"valid": valid, "u": u, "v": v}
        warped = np.zeros((B, C, H, W), dtype=f32)
        S, dIu, dIv = [], [], []
        for ch in range(C):
            p = src[:, ch]
            a00, a01, a10, a11 = p[bi, i0, j0], p[bi, i0, j1], p[bi, i1, j0], p[bi, i1, j1]
            top = w0u * a00 + wu * a01
            bot = w0u * a10 + wu * a11
            s = w0v * top + wv * bot
            S.append(s)
            dIu.append(w0v * (a01 - a00) + wv * (a11 - a10))
            dIv.append(bot - top)
            warped[:, ch] = np.where(valid, s, f32(0))
        out["warped"] = warped

        def g_depth(gs):
            t = [gs[ch] * (dIu[ch] * du + dIv[ch] * dv) for ch in range(C)]
            g = t[0] if C == 1 else (t[0] + t[1]) + t[2]
            return np.where(valid, g, f32(0)).astype(f32)

        if g_warped is not None:
            gw = np.asarray(g_warped, dtype=f32)
            out["g_depth_warp"] = g_depth([gw[:, ch] for ch in range(C)])
        if tgt is not None:
            tgt = np.asarray(tgt, dtype=f32)
            d = [S[ch] - tgt[:, ch] for ch in range(C)]
            e = [np.abs(x_) for x_ in d]
            term = e[0] if C == 1 else (e[0] + e[1]) + e[2]
            out["terms"] = np.where(valid, term, f32(0)).astype(f32)
            n_v = int(valid.sum())
            den = f32(C) * f32(max(n_v, 1))
            kk = f32(gloss) * (one / den)
            sign = [np.where(x_ > 0, one, np.where(x_ < 0, f32(-1), f32(0))).astype(f32) for x_ in d]
            out["n_v"], out["den"] = n_v, den
            out["g_depth_photo"] = g_depth([kk * sg for sg in sign])
    for key, val in out.items():
        if isinstance(val, np.ndarray) and key != "valid":
            assert val.dtype == f32, key
    return out


# ------------------------------------------------------------------------------------------------
# the torch composition
# ------------------------------------------------------------------------------------------------
def composition(depth, k, src, m, mask=None, tgt=None, g_warped=None, gloss=1.0, z_min=0.0, z_max=0.0,
                dtype=torch.float64):
    """The term as a user composes it from torch ops, in `dtype`. The same keys as rule_fp32, the
    gradients from autograd; plus loss. Inputs as rule_fp32's (arrays or tensors)."""
    T = lambda a: torch.as_tensor(np.array(a)).to(dtype)  # noqa: E731
    z0 = T(depth)
    src = T(src)
    B, H, W = z0.shape
    C, Hs, Ws = src.shape[1:]
    k = T(_batched(k, B, (3, 3)))
    m = T(_batched(m, B, (3, 4)))
    zmax = FLT_MAX if z_max == 0.0 else z_max
    pvalid = torch.isfinite(z0) & (z0 > z_min) & (z0 <= zmax)
    # a pixel without a valid depth computes with 1: its value and gradient are masked below
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
    out = {"valid": valid.numpy(), "u": u.detach().numpy(), "v": v.detach().numpy(),
           "warped": warped.detach().numpy()}
    if g_warped is not None:
        (g,) = torch.autograd.grad((warped * T(g_warped)).sum(), z, retain_graph=True)
        out["g_depth_warp"] = g.numpy()
    if tgt is not None:
        n_v = int(valid.sum())
        loss = ((warped - T(tgt)).abs() * vf).sum() / (C * max(n_v, 1))
        (g,) = torch.autograd.grad(loss * gloss, z)
        out["n_v"], out["loss"], out["g_depth_photo"] = n_v, loss.item(), g.numpy()
    return out


# ------------------------------------------------------------------------------------------------
# majorants and the comparable pixels
# ------------------------------------------------------------------------------------------------
def _geometry64(depth, k, src, m):
    z = np.asarray(depth, dtype=np.float64)
    src = np.asarray(src, dtype=np.float64)
    B, H, W = z.shape
    k = _batched(k, B, (3, 3)).astype(np.float64)
    m = _batched(m, B, (3, 4)).astype(np.float64)
    col = lambda a: a[:, None, None]  # noqa: E731
    fx, fy, cx, cy = col(k[:, 0, 0]), col(k[:, 1, 1]), col(k[:, 0, 2]), col(k[:, 1, 2])
    M = [[col(m[:, r, q]) for q in range(4)] for r in range(3)]
    jj = np.arange(W, dtype=np.float64)[None, None, :]
    ii = np.arange(H, dtype=np.float64)[None, :, None]
    return z, src, fx, fy, jj - cx, ii - cy, M


def majorants(depth, k, src, m, valid, g_s=None):
    """(A_warped (B, C, H, W), A_g (B, H, W) or None) in float64: first-order majorants of the fp32 rule's
    rounding error, 0 outside `valid`. With E_u, E_v the rounding majorants of u and v (in units of U):
      a = dot(m[0], P): 3 roundings in x and y, 3 products, 3 sums -> 7 U a_maj, a_maj = sum |m[0][q] P[q]|
      u = a / c                                                   -> E_u = (7 a_maj + 7 |u| c_maj) / |c| + |u|
      s: w0u, w0v (one rounding each), six products, three sums   -> 8 U max|tap|
      A_warped = U (|dIu| E_u + |dIv| E_v + 8 max|tap|)           the image slope times the coordinates' error
    and for g = sum_ch g_s (dIu du + dIv dv), with D2 = (a11 - a10) - (a01 - a00) the slopes' own slope:
      err dIu = U (|D2| E_v + 8 max|tap|),  err dIv = U (|D2| E_u + 8 max|tap|)
      a' = (m00 X + m01 Y) + m02: 2 roundings in X, Y, 2 products, 2 sums -> 5 U a'_maj
      N = a' - u c'      -> U (5 a'_maj + E_u |c'| + 5 |u| c'_maj + |u c'| + |N|)
      du = N / c         -> E_du = err N / |c| + |du| (7 c_maj / |c| + 1)
      A_g = U sum_ch |g_s| (err dIu |du| + |dIu| E_du + err dIv |dv| + |dIv| E_dv + 9 (|dIu du| + |dIv dv|))
    the 9: two products, the sum, the product with g_s, two channel sums and g_s's own three roundings."""
    z, src, fx, fy, tx, ty, M = _geometry64(depth, k, src, m)
    B, H, W = z.shape
    C, Hs, Ws = src.shape[1:]
    ok = np.asarray(valid, dtype=bool)
    with np.errstate(all="ignore"):
        zz = np.where(ok, z, 1.0)
        x, y = tx * zz / fx, ty * zz / fy
        P = (x, y, zz, np.ones_like(zz))
        dot = [sum(M[r][q] * P[q] for q in range(4)) for r in range(3)]
        maj = [sum(np.abs(M[r][q] * P[q]) for q in range(4)) for r in range(3)]
        c = np.where(ok, dot[2], 1.0)
        u, v = np.where(ok, dot[0] / c, 0.0), np.where(ok, dot[1] / c, 0.0)
        E_u = (7 * maj[0] + 7 * np.abs(u) * maj[2]) / np.abs(c) + np.abs(u)
        E_v = (7 * maj[1] + 7 * np.abs(v) * maj[2]) / np.abs(c) + np.abs(v)
        uc, vc = np.clip(u, 0, Ws - 1), np.clip(v, 0, Hs - 1)
        j0, i0 = np.floor(uc).astype(np.int64), np.floor(vc).astype(np.int64)
        j1, i1 = np.minimum(j0 + 1, Ws - 1), np.minimum(i0 + 1, Hs - 1)
        wu, wv = uc - j0, vc - i0
        X, Y = tx / fx + 0 * zz, ty / fy + 0 * zz
        dp = [M[r][0] * X + M[r][1] * Y + M[r][2] for r in range(3)]
        dpm = [np.abs(M[r][0] * X) + np.abs(M[r][1] * Y) + np.abs(M[r][2]) for r in range(3)]

        def d_uv(r, w, E_w):
            N = dp[r] - w * dp[2]
            eN = 5 * dpm[r] + E_w * np.abs(dp[2]) + 5 * np.abs(w) * dpm[2] + np.abs(w * dp[2]) + np.abs(N)
            d = N / c
            return d, eN / np.abs(c) + np.abs(d) * (7 * maj[2] / np.abs(c) + 1)

        du, E_du = d_uv(0, u, E_u)
        dv, E_dv = d_uv(1, v, E_v)
        bi = np.arange(B)[:, None, None]
        A_w = np.zeros((B, C, H, W))
        A_g = None if g_s is None else np.zeros((B, H, W))
        for ch in range(C):
            p = src[:, ch]
            a00, a01, a10, a11 = p[bi, i0, j0], p[bi, i0, j1], p[bi, i1, j0], p[bi, i1, j1]
            amax = np.maximum(np.maximum(np.abs(a00), np.abs(a01)), np.maximum(np.abs(a10), np.abs(a11)))
            top, bot = (1 - wu) * a00 + wu * a01, (1 - wu) * a10 + wu * a11
            dIu = (1 - wv) * (a01 - a00) + wv * (a11 - a10)
            dIv = bot - top
            D2 = np.abs((a11 - a10) - (a01 - a00))
            A_w[:, ch] = np.where(ok, U * (np.abs(dIu) * E_u + np.abs(dIv) * E_v + 8 * amax), 0.0)
            if g_s is not None:
                e_dIu, e_dIv = D2 * E_v + 8 * amax, D2 * E_u + 8 * amax
                per = (e_dIu * np.abs(du) + np.abs(dIu) * E_du + e_dIv * np.abs(dv) + np.abs(dIv) * E_dv
                       + 9 * (np.abs(dIu * du) + np.abs(dIv * dv)))
                A_g += np.where(ok, U * np.abs(np.asarray(g_s, dtype=np.float64)[:, ch]) * per, 0.0)
    return A_w, A_g


def comparable(ref, src_hw, tgt_gap=None):
    """The pixels where the float64 reference's gradient is continuous: valid, u and v farther than EDGE
    from every integer (which includes the borders 0, Ws - 1 and Hs - 1), and, for the photometric
    gradient, |s - tgt| above tgt_gap's threshold in every channel (the sign flips at 0). Returns
    (keep (B, H, W) bool, the omitted share of the valid pixels)."""
    valid = ref["valid"]
    near = lambda w: np.abs(w - np.rint(w)) < EDGE  # noqa: E731
    keep = valid & ~near(ref["u"]) & ~near(ref["v"])
    if tgt_gap is not None:
        keep = keep & (tgt_gap >= EDGE)
    return keep, 1.0 - keep.sum() / max(int(valid.sum()), 1)


def loss_bound(terms, den, L):
    """|L_kernel - sum64(terms) / den| for the kernel's summation of its own fp32 terms: a fp32 sum of
    T = TILE_TERMS non-negative terms in any order is within (T - 1) U / (1 - (T - 1) U) of itself; the
    sums over tiles and images and the division run in double (2^-40 of slack), and the result is rounded
    to fp32 once."""
    S = float(np.asarray(terms, dtype=np.float64).sum())
    g = (TILE_TERMS - 1) * U / (1 - (TILE_TERMS - 1) * U)
    return (g + 2.0 ** -40) * S / float(den) + U * abs(L) * (1 + 2 * g)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def rigid(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    """A (3, 4) float64 [R | t], R = Rz Ry Rx (radians)."""
    cx_, sx = np.cos(rx), np.sin(rx)
    cy_, sy = np.cos(ry), np.sin(ry)
    cz, sz = np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.concatenate((Rz @ Ry @ Rx, np.asarray(t, dtype=np.float64)[:, None]), axis=1)


def intrinsics(H, W, f):
    return np.array([[f, 0, (W - 1) / 2 + 0.25], [0, f * 1.03, (H - 1) / 2 - 0.5], [0, 0, 1]], dtype=np.float64)


def warp_inputs(seed, B, C, size, src_size=None, per_image_m=True, with_mask=False, holes=True):
    """A dict of float32 arrays: depth (B, H, W) smoothly varying in about [5, 17] with (holes) a few 0, NaN
    and inf pixels, k (3, 3), src (B, C, Hs, Ws) and tgt (B, C, H, W) in [0, 1], m (B, 3, 4) or (3, 4) for
    a forward motion with a small rotation (a few pixels of flow, part of the border leaving the source),
    mask (B, H, W) uint8 with a tenth zero, or None, and g_warped (B, C, H, W)."""
    H, W = size
    Hs, Ws = src_size or size
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 1, 4, 6, generator=g) * 12 + 5
    depth = F.interpolate(coarse, size=(max(H, 2), max(W, 2)), mode="bilinear", align_corners=True)[:, 0, :H, :W]
    depth = depth.contiguous().numpy().astype(f32)
    if holes and H * W >= 64:
        r = torch.rand(B, H, W, generator=g).numpy()
        depth[r < 0.02] = 0.0
        depth[(r >= 0.02) & (r < 0.03)] = np.nan
        depth[(r >= 0.03) & (r < 0.04)] = np.inf
        depth[(r >= 0.04) & (r < 0.05)] = -3.0
    f = 0.9 * max(W, 2)
    k = intrinsics(H, W, f)
    ks = intrinsics(Hs, Ws, f * Ws / W)
    poses = [rigid(0.004 * (b + 1), -0.006, 0.003, (0.12 + 0.05 * b, -0.04, 0.45 - 0.1 * b)) for b in range(B)]
    ms = np.stack([ks @ p for p in poses]).astype(f32)
    src = torch.rand(B, C, Hs, Ws, generator=g).numpy().astype(f32)
    tgt = torch.rand(B, C, H, W, generator=g).numpy().astype(f32)
    g_warped = (torch.rand(B, C, H, W, generator=g) * 2 - 1).numpy().astype(f32)
    mask = (torch.rand(B, H, W, generator=g) > 0.1).numpy().astype(np.uint8) if with_mask else None
    return {"depth": depth, "k": k.astype(f32), "src": src, "tgt": tgt, "m": ms if per_image_m else ms[0],
            "mask": mask, "g_warped": g_warped}


# the inputs of the CPU comparison and of kappa: (name, seed, B, C, size, src_size, per_image_m, with_mask)
CPU_CASES = [("17x65_from_19x70_c3", 1, 2, 3, (17, 65), (19, 70), True, False),
             ("45x67_c1_shared_m_mask", 2, 2, 1, (45, 67), None, False, True),
             ("64x96_c3", 3, 2, 3, (64, 96), None, True, True)]
OUTPUTS = ("warped", "g_depth_warp", "g_depth_photo")


def case_inputs(name):
    _, seed, B, C, size, src_size, per_image, with_mask = next(c for c in CPU_CASES if c[0] == name)
    return warp_inputs(seed, B, C, size, src_size, per_image, with_mask)


def case_budget(name):
    """(inputs, float64 reference, keep masks, omitted shares and majorants per output) of a CPU case."""
    x = case_inputs(name)
    args = (x["depth"], x["k"], x["src"], x["m"], x["mask"], x["tgt"], x["g_warped"])
    ref = composition(*args)
    B, C = x["src"].shape[:2]
    gap = np.abs(ref["warped"] - x["tgt"]).min(axis=1)
    keep_w, omit_w = comparable(ref, x["src"].shape[2:])
    keep_p, omit_p = comparable(ref, x["src"].shape[2:], gap)
    kk = 1.0 / (C * max(ref["n_v"], 1))
    A_w, A_gw = majorants(x["depth"], x["k"], x["src"], x["m"], ref["valid"], x["g_warped"])
    _, A_gp = majorants(x["depth"], x["k"], x["src"], x["m"], ref["valid"], np.full(x["tgt"].shape, kk))
    keep = {"warped": np.broadcast_to(keep_w[:, None], A_w.shape), "g_depth_warp": keep_w, "g_depth_photo": keep_p}
    omit = {"warped": omit_w, "g_depth_warp": omit_w, "g_depth_photo": omit_p}
    return x, args, ref, keep, omit, {"warped": A_w, "g_depth_warp": A_gw, "g_depth_photo": A_gp}


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
            x, args, ref, keep, omit, A = case_budget(name)
            r = ratios(composition(*args, dtype=torch.float32), ref, keep, A)
            table[name] = {key: {"kappa_ref": float(f"{v:.4g}"), "kappa": float(f"{4 * v:.4g}")} for key, v in r.items()}
        return table
    finally:
        torch.set_num_threads(n)


def load_kappa():
    with open(KAPPA_JSON) as fh:
        return json.load(fh)


def kappa_for(table):
    """The kappa the GPU and CPU checks apply per output: the largest over the measured cases."""
    return {key: max(table[name][key]["kappa"] for name in table) for key in OUTPUTS}


if __name__ == "__main__":
    t = measure_kappa()
    print(json.dumps(t, indent=1))
    if "--write" in sys.argv:
        with open(KAPPA_JSON, "w") as fh:
            json.dump(t, fh, indent=1)
            fh.write("\n")
