"""References, bounds and inputs of the smoothness-loss tests (test_smooth_cpu.py, test_gpu_smooth.py):

  E, edge_weights_rule   the rule of include/nconv.h (nconv_edge_weights) restated in numpy, every operation an
                         explicit float32 step: the range reduction, the Horner polynomial, the power of two
  rule_fp32              nconv_smooth_loss_* likewise, the sums in the tree of csrc/wave_ops.h (reduce_tree.py)
                         -- what the kernels must reproduce bit for bit
  composition            the same term composed from torch ops in whatever dtype is asked for (slices, abs,
                         exp, means), differentiated by autograd (float64: the reference; float32: what kappa
                         is measured from)
  majorants              first-order float64 majorants of the fp32 rule's error (the loss, g_depth per element)
  comparable             the gradient's elements none of whose terms sits on the sign's discontinuity
  e_error                the largest relative error of E against float64 exp(-x) over the reachable arguments
  measure_kappa          torch's float32 run of the composition against float64 in units of the majorants;
                         `python tests/smooth_cases.py --write` writes tests/golden/smooth_bound_kappa.json
"""
import json
import os
import re
import sys

import numpy as np
import torch

import reduce_tree as RT

f32 = np.float32
U = 2.0 ** -24
TREE_ADDS = 3 + 6 + 3              # the fp32 additions a term passes through: thread, butterfly, waves
HERE = os.path.dirname(os.path.abspath(__file__))
KAPPA_JSON = os.path.join(HERE, "golden", "smooth_bound_kappa.json")
HEADER = os.path.join(os.path.dirname(HERE), "include", "nconv.h")

# ------------------------------------------------------------------------------------------------
# E(x): exp(-x), x >= 0
# ------------------------------------------------------------------------------------------------
LOG2E = f32(1.44269504)
COEF = [f32(c) for c in (1.0, 0.693147182, 0.240226507, 0.0555041097, 0.00961812865, 0.00133335579, 0.000154035297)]


def E(x):
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        y0 = x * LOG2E
        y = np.where(y0 < f32(126), y0, f32(126)).astype(f32)
        n = np.rint(y)
        r = n - y
        p = np.full_like(r, COEF[6])
        for c in COEF[5::-1]:
            p = p * r
            p = p + c
        ni = np.minimum(n.astype(np.int32), 125)
        scale = ((127 - ni) << 23).astype(np.int32).view(f32)
        e = p * scale
    out = np.where(n > f32(125), f32(0), e)
    assert out.dtype == f32
    return out


def e_arguments(alpha):
    """The float32 arguments alpha g reaches for g in [0, 255]: every g an 8-bit frame produces (k and k / 3
    for integer k), and of every binade from the smallest subnormal up 4096 evenly spaced significands with
    both ends, cut at alpha 255."""
    alpha = f32(alpha)
    top = alpha * f32(255)
    g = np.concatenate((np.arange(256, dtype=f32), np.arange(766, dtype=f32) / f32(3.0)))
    xs = [alpha * g, np.array([0.0, top], dtype=f32), (np.arange(1, 1 << 12, dtype=np.int32)).view(f32)]
    frac = np.concatenate((np.arange(0, 1 << 23, 1 << 11, dtype=np.int64), [(1 << 23) - 1]))
    for e in range(1, 255):
        xs.append(((e << 23) + frac).astype(np.int32).view(f32))
    x = np.concatenate(xs)
    return np.unique(x[x <= top])


def e_error(alpha):
    """max |E(x) - exp(-x)| / exp(-x) in float64 over e_arguments(alpha) where E(x) is not flushed to 0; the
    flushed arguments must be those whose exp(-x) is below 2^-125."""
    x = e_arguments(alpha)
    got = E(x).astype(np.float64)
    want = np.exp(-x.astype(np.float64))
    live = got != 0
    assert (want[~live] < 2.0 ** -125).all() and live[x <= 86].all()
    return float((np.abs(got[live] - want[live]) / want[live]).max())


def header_e_errors():
    """{'1/255': str, '1': str} as written beside the rule in include/nconv.h."""
    with open(HEADER) as fh:
        text = fh.read()
    m = re.search(r"E_MAX_REL_ERR\s+alpha = 1/255:\s*(\S+)\s+alpha = 1:\s*(\S+?)[\s,;]", text)
    return {"1/255": m.group(1), "1": m.group(2)}


def edge_weights_rule(img, alpha=1.0 / 255.0):
    """img (B, C, H, W) -> float32 (B, 2, H, W)."""
    I = np.asarray(img, dtype=f32)
    B, C, H, W = I.shape
    alpha = f32(alpha)
    out = np.ones((B, 2, H, W), dtype=f32)
    with np.errstate(all="ignore"):
        for p, (hi, lo) in enumerate(((I[..., :, 1:], I[..., :, :-1]), (I[..., 1:, :], I[..., :-1, :]))):
            d = np.abs(hi - lo)
            g = d[:, 0] if C == 1 else ((d[:, 0] + d[:, 1]) + d[:, 2]) / f32(3.0)
            w = E(alpha * g)
            if p == 0:
                out[:, 0, :, :W - 1] = w
            else:
                out[:, 1, :H - 1, :] = w
    return out


# ------------------------------------------------------------------------------------------------
# the fp32 rule
# ------------------------------------------------------------------------------------------------
def _terms_along(d, M, w, order, xp=np):
    """The terms along the last axis, centred: (c, t, omega, ops) of shape d's, c False where there is no
    term. ops = the sum of the operands' magnitudes. w None: omega None. Works on numpy arrays of any dtype."""
    c = np.zeros(d.shape, dtype=bool)
    t = np.zeros_like(d)
    ops = np.zeros_like(d)
    om = None if w is None else np.ones_like(d)
    W = d.shape[-1]
    with np.errstate(all="ignore"):
        if order == 1 and W >= 2:
            c[..., :-1] = M[..., :-1] & M[..., 1:]
            t[..., :-1] = d[..., 1:] - d[..., :-1]
            ops[..., :-1] = np.abs(d[..., 1:]) + np.abs(d[..., :-1])
            if w is not None:
                om[..., :-1] = w[..., :-1]
        elif order == 2 and W >= 3:
            c[..., 1:-1] = M[..., :-2] & M[..., 1:-1] & M[..., 2:]
            two = d.dtype.type(2)
            t[..., 1:-1] = (d[..., :-2] + d[..., 2:]) - two * d[..., 1:-1]
            ops[..., 1:-1] = np.abs(d[..., :-2]) + np.abs(d[..., 2:]) + two * np.abs(d[..., 1:-1])
            if w is not None:
                w0, w1 = w[..., :-2], w[..., 1:-1]
                om[..., 1:-1] = np.where(w1 < w0, w1, w0)
    return c, t, om, ops


def _shift(q, axis, by):
    """q moved by `by` along axis, +0 shifted in: out[p] = q[p - by]."""
    out = np.zeros_like(q)
    n = q.shape[axis]
    if abs(by) >= n:
        return out
    src = [slice(None)] * q.ndim
    dst = [slice(None)] * q.ndim
    src[axis] = slice(0, n - by) if by > 0 else slice(-by, n)
    dst[axis] = slice(by, n) if by > 0 else slice(0, n + by)
    out[tuple(dst)] = q[tuple(src)]
    return out


def _sum64(terms):
    part = RT.tile_partials(terms, RT.ROWS)
    acc = np.float64(0.0)
    for b in range(part.shape[0]):
        acc += RT.image_sum(part[b])
    return acc


def rule_fp32(depth, weights=None, order=1, mask=None, gloss=1.0):
    """A dict: sx, sy (B, H, W) float32 terms at their centre pixels, cx, cy bool, tx, ty, n_x, n_y, L
    (float32, the stated tree) and g_depth (B, H, W). depth (B, H, W), weights (B, 2, H, W) or None, mask
    (B, H, W) or None."""
    d = np.asarray(depth, dtype=f32)
    B, H, W = d.shape
    M = np.ones(d.shape, dtype=bool) if mask is None else (np.asarray(mask) != 0)
    w = None if weights is None else np.asarray(weights, dtype=f32)
    T = lambda a: None if a is None else np.swapaxes(a, 1, 2)  # noqa: E731
    cx, tx, ox, _ = _terms_along(d, M, None if w is None else w[:, 0], order)
    cy, ty, oy, _ = (T(a) for a in _terms_along(T(d), T(M), None if w is None else T(w[:, 1]), order))
    out = {"cx": cx, "cy": cy, "tx": tx, "ty": ty}
    one = f32(1.0)
    with np.errstate(all="ignore"):
        s, q, n = {}, {}, {}
        for key, c, t, om in (("x", cx, tx, ox), ("y", cy, ty, oy)):
            e = np.abs(t)
            s[key] = np.where(c, e if om is None else om * e, f32(0)).astype(f32)
            n[key] = int(c.sum())
            k = f32(gloss) * (one / f32(max(n[key], 1)))
            sg = np.where(t > 0, one, np.where(t < 0, f32(-1), f32(0))).astype(f32)
            kw = np.full_like(t, k) if om is None else k * om
            q[key] = np.where(c, kw * sg, f32(0)).astype(f32)
        qx, qy = q["x"], q["y"]
        if order == 1:
            g = ((_shift(qx, 2, 1) - qx) + _shift(qy, 1, 1)) - qy
        else:
            two = f32(2.0)
            g = (((_shift(qx, 2, 1) + _shift(qx, 2, -1)) - two * qx) + (_shift(qy, 1, 1) + _shift(qy, 1, -1))) - two * qy
        L = f32(_sum64(s["x"]) / np.float64(max(n["x"], 1)) + _sum64(s["y"]) / np.float64(max(n["y"], 1)))
    out.update(sx=s["x"], sy=s["y"], n_x=n["x"], n_y=n["y"], L=L, g_depth=g.astype(f32), qx=qx, qy=qy)
    for key in ("sx", "sy", "g_depth", "tx", "ty"):
        assert out[key].dtype == f32, key
    return out


# ------------------------------------------------------------------------------------------------
# the torch composition
# ------------------------------------------------------------------------------------------------
def edge_weights_composition(img, alpha=1.0 / 255.0, dtype=torch.float64):
    I = torch.as_tensor(np.array(img)).to(dtype)
    B, C, H, W = I.shape
    out = torch.ones(B, 2, H, W, dtype=dtype)
    out[:, 0, :, :W - 1] = torch.exp(-alpha * (I[..., :, 1:] - I[..., :, :-1]).abs().mean(1))
    out[:, 1, :H - 1, :] = torch.exp(-alpha * (I[..., 1:, :] - I[..., :-1, :]).abs().mean(1))
    return out.numpy()


def composition(depth, weights=None, order=1, mask=None, gloss=1.0, dtype=torch.float64):
    """The term as a user composes it from torch ops, in `dtype`: {'L', 'g_depth', 'n_x', 'n_y'}."""
    d = torch.as_tensor(np.array(depth)).to(dtype).requires_grad_(True)
    B, H, W = d.shape
    M = torch.ones(d.shape, dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask) != 0)
    w = None if weights is None else torch.as_tensor(np.array(weights)).to(dtype)
    L = 0.0
    n = []
    for axis in (2, 1):
        sl = lambda a, lo, hi: a.narrow(axis, lo, a.shape[axis] + hi - lo)  # noqa: E731  a[lo : size + hi]
        size = d.shape[axis]
        if size <= order:
            n.append(0)
            continue
        wa = None if w is None else w[:, 0 if axis == 2 else 1]
        if order == 1:
            t = sl(d, 1, 0) - sl(d, 0, -1)
            c = sl(M, 1, 0) & sl(M, 0, -1)
            om = None if wa is None else sl(wa, 0, -1)
        else:
            t = sl(d, 0, -2) + sl(d, 2, 0) - 2 * sl(d, 1, -1)
            c = sl(M, 0, -2) & sl(M, 1, -1) & sl(M, 2, 0)
            om = None if wa is None else torch.minimum(sl(wa, 0, -2), sl(wa, 1, -1))
        e = t.abs() if om is None else om * t.abs()
        cnt = int(c.sum())
        n.append(cnt)
        L = L + (e * c.to(dtype)).sum() / max(cnt, 1)
    if not torch.is_tensor(L):
        return {"L": 0.0, "g_depth": np.zeros((B, H, W)), "n_x": n[0], "n_y": n[1]}
    (g,) = torch.autograd.grad(L * gloss, d)
    return {"L": L.item(), "g_depth": g.numpy(), "n_x": n[0], "n_y": n[1]}


# ------------------------------------------------------------------------------------------------
# majorants and the comparable elements
# ------------------------------------------------------------------------------------------------
def _terms64(depth, weights, order, mask):
    d = np.asarray(depth, dtype=np.float64)
    M = np.ones(d.shape, dtype=bool) if mask is None else (np.asarray(mask) != 0)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    T = lambda a: None if a is None else np.swapaxes(a, 1, 2)  # noqa: E731
    x = _terms_along(d, M, None if w is None else w[:, 0], order)
    y = tuple(T(a) for a in _terms_along(T(d), T(M), None if w is None else T(w[:, 1]), order))
    return x, y


def _gather(a, axis, order):
    """The sum over the terms a pixel takes part in of |coefficient| a: order 1 the terms at p - 1 and p,
    order 2 those at p - 1, p (twice) and p + 1."""
    if order == 1:
        return _shift(a, axis, 1) + a
    return _shift(a, axis, 1) + 2 * a + _shift(a, axis, -1)


def majorants(depth, weights=None, order=1, mask=None, gloss=1.0):
    """(A_L, A_g (B, H, W), keep (B, H, W) bool, zero_terms) in float64.
      t: one rounding (order 1) or two (order 2), each at most U ops, ops the operands' magnitudes summed;
      s = omega |t|: one more -> err s <= U omega (2 ops + |t|)
      the sum: a term passes through TREE_ADDS fp32 additions, then double -> TREE_ADDS U S
      A_L = sum over both directions of (sum err s + TREE_ADDS U S) / n, + U |L| for the final rounding
      q = (k omega) sign: k = gloss (1 / n) two roundings, k omega one -> 3 U |q|; g adds its 4 (order 1) or
      6 (order 2) signed q in 3 or 5 additions, each at most U sum |coef q|
      A_g = U (3 + adds) sum |coef q|
    keep: the elements all of whose terms have |t| exactly 0 or above 4 U ops (the sign is the reference's);
    zero_terms: how many counted terms are exactly 0."""
    (cx, tx, ox, px), (cy, ty, oy, py) = _terms64(depth, weights, order, mask)
    A_L, L = 0.0, 0.0
    A_g = np.zeros(tx.shape)
    bad_any = np.zeros(tx.shape, dtype=bool)
    zeros = 0
    adds = 3 if order == 1 else 5
    for axis, c, t, om, ops in ((2, cx, tx, ox, px), (1, cy, ty, oy, py)):
        om = np.ones_like(t) if om is None else om
        n = max(int(c.sum()), 1)
        S = float((om * np.abs(t))[c].sum())
        A_L += (U * float((np.abs(om) * (2 * ops + np.abs(t)))[c].sum()) + TREE_ADDS * U * S) / n
        L += S / n
        q = np.where(c, np.abs(gloss) / n * np.abs(om) * (t != 0), 0.0)
        A_g += U * (3 + adds) * _gather(q, axis, order)
        bad = c & (t != 0) & ~(np.abs(t) > 4 * U * ops)
        bad_any |= _gather(bad.astype(np.float64), axis, order) > 0
        zeros += int((c & (t == 0)).sum())
    return A_L + U * abs(L), A_g, ~bad_any, zeros


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def smooth_depth(B, H, W, seed=0):
    """10 + 6 sin(i / 7) + 5 cos(j / 11) + U(-0.05, 0.05), a 5 x 20 patch (where it fits) exactly 12.0."""
    g = torch.Generator().manual_seed(seed)
    i = np.arange(H, dtype=np.float64)[:, None]
    j = np.arange(W, dtype=np.float64)[None, :]
    noise = (torch.rand(B, H, W, generator=g, dtype=torch.float64) * 0.1 - 0.05).numpy()
    d = (10 + 6 * np.sin(i / 7) + 5 * np.cos(j / 11) + noise).astype(f32)
    if H >= 8 and W >= 24:
        d[:, 3:8, 4:24] = f32(12.0)
    return d


def smooth_inputs(B, H, W, seed=0, with_w=False, with_mask=False, C=3):
    """{'depth', 'weights', 'mask', 'rgb'}: the weights are the rule's of an 8-bit-valued random frame with a
    few hard edges, a tenth of the mask is 0."""
    g = torch.Generator().manual_seed(1000 + seed)
    rgb = torch.randint(0, 256, (B, C, H, W), generator=g).float().numpy()
    rgb[..., W // 2:] = np.minimum(rgb[..., W // 2:], 40)
    mask = (torch.rand(B, H, W, generator=g) > 0.1).numpy().astype(np.uint8) if with_mask else None
    weights = edge_weights_rule(rgb, 1.0 / 255.0) if with_w else None
    return {"depth": smooth_depth(B, H, W, seed), "weights": weights, "mask": mask, "rgb": rgb}


# (name, B, H, W, order, with_w, with_mask)
CPU_CASES = [("33x130_o1_w", 2, 33, 130, 1, True, False), ("33x130_o2_w_mask", 2, 33, 130, 2, True, True),
             ("17x65_o1_mask", 2, 17, 65, 1, False, True), ("17x65_o2", 2, 17, 65, 2, False, False)]
OUTPUTS = ("L", "g_depth")
GLOSS = 0.7

# the shapes of the GPU comparison: degenerate ones, one row or column past a 16 x 64 tile, exactly one tile
GPU_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 5), (1, 1, 5, 1), (1, 1, 2, 2), (1, 1, 3, 3), (2, 1, 17, 65), (2, 1, 33, 130),
              (3, 1, 16, 64)]


def case_budget(name):
    """(args, float64 reference, majorants) of a CPU case; args = (depth, weights, order, mask, gloss)."""
    _, B, H, W, order, with_w, with_mask = next(c for c in CPU_CASES if c[0] == name)
    x = smooth_inputs(B, H, W, seed=H + order, with_w=with_w, with_mask=with_mask)
    args = (x["depth"], x["weights"], order, x["mask"], GLOSS)
    return args, composition(*args), majorants(*args)


def ratios(got, ref, maj):
    """|got - ref| / A per output, the gradient's over the kept elements."""
    A_L, A_g, keep, _ = maj
    err = np.abs(np.asarray(got["g_depth"], dtype=np.float64) - ref["g_depth"])[keep]
    return {"L": abs(float(got["L"]) - ref["L"]) / A_L, "g_depth": float((err / (A_g[keep] + 1e-300)).max())}


def measure_kappa():
    """{case: {output: {"kappa_ref", "kappa"}}}: torch's own float32 run of the composition against the
    float64 one in units of the majorant, and 4 x that (the project's convention, warp_bound_kappa.json)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        table = {}
        for name, *_ in CPU_CASES:
            args, ref, maj = case_budget(name)
            r = ratios(composition(*args, dtype=torch.float32), ref, maj)
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
    print("E_MAX_REL_ERR", {a: f"{e_error(v):.3e}" for a, v in (("1/255", 1.0 / 255.0), ("1", 1.0))})
    if "--write" in sys.argv:
        with open(KAPPA_JSON, "w") as fh:
            json.dump(t, fh, indent=1)
            fh.write("\n")
