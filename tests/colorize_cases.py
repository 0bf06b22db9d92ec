"""The numpy restatement of nconv_depth_colorize (include/nconv.h) and the shapes its tests sweep.

colorize_ref follows the entry point's rules literally, in fp32 throughout:
  1. a pixel is empty iff its value is not finite or <= floor (floor None: -inf)
  2. lo, hi: the minimum and maximum of the image's non-empty source pixels, or vmin, vmax
  3. s = 255.0f / (hi - lo), one fp32 division
  4. idx = clamp((int)rintf((v - lo) * s), 0, 255), two fp32 roundings before the rint, ties to even; the
     clamp is made on the float (a NaN product gives 0)
  5. hi <= lo: idx 0 for every non-empty pixel; an image without a non-empty pixel is all empty
  6. radius r: a pixel shows the smallest non-empty value of its (2r + 1)^2 window clipped at the border,
     empty if the window holds none; the range still comes from the source plane
  7. uint8 (B, H, W, 3): table[idx] for a non-empty pixel (channels reversed with order 'bgr'), else the
     background pixel as it is, else `empty` (reversed with 'bgr')
"""
import numpy as np

F = np.float32

# the sweep of tests/test_gpu_colorize.py: images smaller than the window, one lane, a ragged last group
# of four, more than one row of lanes; rows below and above the two a wave takes
WIDTHS = (1, 3, 4, 5, 17, 67)
HEIGHTS = (1, 2, 9)
BATCHES = (1, 3)
RADII = (0, 1, 2, 4)
CMAPS = ("inferno", "magma", "viridis", "turbo", "gray")


def splat_min(v, ok, r):
    """Per pixel the smallest non-empty value of its (2r + 1)^2 window and whether there is one.
    v: (H, W) fp32, ok: (H, W) bool."""
    H, W = v.shape
    cand = np.where(ok, v, F(np.inf))
    best = np.full((H, W), F(np.inf), dtype=F)
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
            if i0 >= i1 or j0 >= j1:
                continue
            best[i0:i1, j0:j1] = np.minimum(best[i0:i1, j0:j1], cand[i0 + di:i1 + di, j0 + dj:j1 + dj])
    return best, best < F(np.inf)


def color_index(v, lo, hi):
    """idx of rule 3-5 for the fp32 array v (every entry a non-empty value)."""
    lo, hi = F(lo), F(hi)
    if hi <= lo:
        return np.zeros(v.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        s = F(255.0) / F(hi - lo)
        d = (v.astype(F) - lo).astype(F)
        q = np.rint((d * s).astype(F))
    q = np.where(q > 0, q, F(0.0))
    q = np.where(q < 255, q, F(255.0))
    return q.astype(np.int64)


def colorize_ref(depth, table, vmin=None, vmax=None, floor=None, radius=0, background=None, empty=(0, 0, 0),
                 order="rgb"):
    """depth: (B, H, W) fp32 array; table: (256, 3) uint8 R, G, B; background: (B, H, W, 3) uint8 or None."""
    depth = np.asarray(depth)
    assert depth.dtype == F and depth.ndim == 3 and (vmin is None) == (vmax is None)
    table = np.asarray(table, dtype=np.uint8)
    if order == "bgr":
        table, empty = table[:, ::-1], tuple(empty)[::-1]
    B, H, W = depth.shape
    fl = F(-np.inf) if floor is None else F(floor)
    out = np.empty((B, H, W, 3), dtype=np.uint8)
    for b in range(B):
        v = depth[b]
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(v) & (v > fl)
        if vmin is not None:
            lo, hi = F(vmin), F(vmax)
        elif ok.any():
            lo, hi = v[ok].min(), v[ok].max()
        else:
            lo = hi = F(0.0)
        shown, has = splat_min(v, ok, radius) if radius else (v, ok)
        idx = np.zeros((H, W), dtype=np.int64)
        idx[has] = color_index(shown[has], lo, hi)
        img = table[idx]
        none = background[b] if background is not None else np.broadcast_to(np.array(empty, dtype=np.uint8), (H, W, 3))
        out[b] = np.where(has[..., None], img, none)
    return out


def plane(rng, B, H, W, fill=0.6, special=True):
    """(B, H, W) fp32 test planes: depths in (0.5, 80), a share 1 - fill zeroed (a sparse plane), and,
    with special, NaN, +-inf, negatives and -0.0 scattered through them."""
    v = rng.uniform(0.5, 80.0, (B, H, W)).astype(F)
    v[rng.random((B, H, W)) > fill] = 0.0
    if special:
        flat = v.reshape(-1)
        for val in (np.nan, np.inf, -np.inf, -3.5, -0.0):
            flat[rng.integers(0, flat.size, max(1, flat.size // 16))] = val
    return v


def custom_table(rng):
    return rng.integers(0, 256, (256, 3)).astype(np.uint8)
