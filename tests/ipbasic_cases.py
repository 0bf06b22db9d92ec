"""The numpy reference of the IP-Basic baseline (csrc/ipbasic.hip, nconv_depth_ipbasic) and the seeded
planes of its tests.

The rule of include/nconv.h restated stage by stage in float32, so the GPU tests compare bit for bit.
T = 0.1f; in the inverted domain a pixel is valid iff v > T and empty iff v < T.
    invert       v0 = max_depth - d where d is finite, d > T and max_depth - d > T, else +0.0
    dilate       the max over the in-image pixels of the footprint (full / cross / diamond, odd size)
    erode5       the min over the in-image pixels of the full 5 x 5 window
    fill         empty(v) ? dilate(v, full, size) : v
    extrapolate  every pixel above its column's first valid row takes that row's value
    median5      the 13th smallest of the 5 x 5 window, coordinates clamped to the image
    gauss5       (((w0 a0 + w1 a1) + w2 a2) + w3 a3) + w4 a4 along rows, then along columns, reflect-101
    finish       valid(v) ? max_depth - v : +0.0, the input samples bit for bit with keep_samples
Every window is gathered tap by tap from shifted copies of the plane: nothing here is separable, tiled
or in place, which is what the kernel does."""
import numpy as np

F32 = np.float32
T = F32(0.1)
W5 = tuple(F32(w) for w in (0.0625, 0.25, 0.375, 0.25, 0.0625))

# The kernel's tile is 64 rows x 64 columns (csrc/ipbasic.hip: kTH, kTW).
TILE = (64, 64)
TH, TW = TILE
# an image smaller than every halo, a partial tile in each direction, and at least one interior seam in
# each direction
SHAPES = ((1, 1, 1), (2, 5, 7), (3, 37, 71), (1, 40, 136), (2, 71, 139), (1, TH + 1, TW + 1), (1, 2 * TH + 3, TW - 1))
DENSITIES = (0.05, 0.6)
KERNELS = (("diamond", 5), ("cross", 7), ("full", 3), ("diamond", 7))
DEFAULTS = dict(max_depth=100.0, kernel=("diamond", 5), extrapolate=False, median=True, blur="gaussian",
                keep_samples=False)
# A covering set of the option product: every value of every option, and every value of every option
# beside both values of extrapolate.
OPTION_SETS = tuple(dict(DEFAULTS, **o) for o in (
    dict(),
    dict(extrapolate=True),
    dict(kernel=("cross", 7), median=False, keep_samples=True),
    dict(kernel=("cross", 7), median=False, keep_samples=True, extrapolate=True),
    dict(kernel=("full", 3), blur=None),
    dict(kernel=("full", 3), blur=None, extrapolate=True),
    dict(kernel=("diamond", 7), median=False, blur=None, max_depth=80.0),
    dict(kernel=("diamond", 7), keep_samples=True, extrapolate=True, max_depth=80.0),
))


def valid(v):
    return v > T


def empty(v):
    return v < T


def sample_of(d, max_depth):
    d = np.asarray(d, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > T) & ((F32(max_depth) - d) > T)


def invert(d, max_depth):
    d = np.asarray(d, dtype=F32)
    with np.errstate(invalid="ignore"):
        v = F32(max_depth) - d
    return np.where(sample_of(d, max_depth), v, F32(0)).astype(F32)


def footprint(shape, size):
    """The offsets (dy, dx) of a kernel."""
    r = size // 2
    keep = {"full": lambda dy, dx: True, "cross": lambda dy, dx: dy == 0 or dx == 0,
            "diamond": lambda dy, dx: abs(dy) + abs(dx) <= r}[shape]
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if keep(dy, dx)]


def _windowed(v, offsets, outside, op):
    """op over the taps of `offsets`, a pixel outside the image standing as `outside` (op's neutral)."""
    B, H, W = v.shape
    r = max(max(abs(dy), abs(dx)) for dy, dx in offsets)
    pad = np.full((B, H + 2 * r, W + 2 * r), outside, dtype=F32)
    pad[:, r:r + H, r:r + W] = v
    out = np.full((B, H, W), outside, dtype=F32)
    for dy, dx in offsets:
        out = op(out, pad[:, r + dy:r + dy + H, r + dx:r + dx + W])
    return out


def dilate(v, shape, size):
    # every value is >= 0 and the centre is always a tap, so 0 outside the image takes no part
    return _windowed(v, footprint(shape, size), F32(0), np.maximum)


def erode5(v):
    return _windowed(v, footprint("full", 5), F32(np.inf), np.minimum)


def fill(v, size):
    return np.where(empty(v), dilate(v, "full", size), v)


def extrapolate(v):
    B, H, W = v.shape
    ok = valid(v)
    top = np.where(ok.any(axis=1), ok.argmax(axis=1), 0)  # (B, W)
    at_top = np.take_along_axis(v, top[:, None, :], axis=1)  # (B, 1, W)
    rows = np.arange(H)[None, :, None]
    return np.where(rows < top[:, None, :], at_top, v).astype(F32), top.astype(np.int32)


_extrapolate = extrapolate  # ipbasic_ref's option of the same name shadows it there


def median5(v):
    B, H, W = v.shape
    ys = np.clip(np.arange(-2, H + 2), 0, H - 1)
    xs = np.clip(np.arange(-2, W + 2), 0, W - 1)
    pad = v[:, ys][:, :, xs]
    taps = np.stack([pad[:, dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)], axis=0)
    return np.sort(taps, axis=0)[12]


def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def _gauss_axis(v, axis):
    n = v.shape[axis]
    idx = [np.array([reflect101(i + k - 2, n) for i in range(n)]) for k in range(5)]
    a = [np.take(v, ix, axis=axis) for ix in idx]
    s = W5[0] * a[0] + W5[1] * a[1]
    s = s + W5[2] * a[2]
    s = s + W5[3] * a[3]
    s = s + W5[4] * a[4]
    assert s.dtype == F32
    return s


def gauss5(v):
    return _gauss_axis(_gauss_axis(v, 2), 1)


def finish(v, d, max_depth, keep_samples):
    out = np.where(valid(v), F32(max_depth) - v, F32(0)).astype(F32)
    if keep_samples:
        out = np.where(sample_of(d, max_depth), np.asarray(d, dtype=F32), out)
    return out


def ipbasic_ref(d, max_depth=100.0, kernel=("diamond", 5), extrapolate=False, median=True, blur="gaussian",
                keep_samples=False, stages=False):
    """The completed planes (B, H, W) float32; with stages a dict of every intermediate plane as well."""
    d = np.asarray(d, dtype=F32)
    assert d.ndim == 3
    s = {}
    s["v0"] = invert(d, max_depth)
    s["v1"] = dilate(s["v0"], *kernel)
    s["v2"] = erode5(dilate(s["v1"], "full", 5))
    s["v3"] = fill(s["v2"], 7)
    if extrapolate:
        s["v3e"], s["top"] = _extrapolate(s["v3"])
        s["v4"] = fill(s["v3e"], 31)
    else:
        s["v4"] = s["v3"]
    s["v5"] = median5(s["v4"]) if median else s["v4"]
    if blur in ("gaussian",):
        s["v6"] = np.where(valid(s["v5"]), gauss5(s["v5"]), s["v5"])
    else:
        assert blur in (None, "none")
        s["v6"] = s["v5"]
    s["out"] = finish(s["v6"], d, max_depth, keep_samples)
    for k, v in s.items():
        assert k == "top" or v.dtype == F32, k
    return s if stages else s["out"]


def specials(max_depth=100.0):
    with np.errstate(all="ignore"):
        return np.array([np.nan, np.inf, -np.inf, -0.0, -3.0, T, 0.05, max_depth, F32(max_depth) - F32(0.05)], dtype=F32)


def plane(B, H, W, seed, density=0.05, max_depth=100.0, with_specials=True):
    """A sparse plane (B, H, W) float32: a share `density` of the pixels holds a depth in 0.5..90, the
    rest 0. For H >= 37 the top 20 rows are empty, as in a KITTI plane; for W >= 71 a block of 40 columns
    is empty, so that empty pixels survive the 31 x 31 fill. About 1 % of the pixels (at least one) are
    specials: NaN, +-inf, -0.0, -3, 0.1f exactly, 0.05, max_depth and max_depth - 0.05."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 90.0, (B, H, W)).astype(F32)
    z[rng.random((B, H, W)) >= density] = 0
    if H >= 37:
        z[:, :20] = 0
    if W >= 71:
        x0 = int(rng.integers(0, W - 40 + 1))
        z[:, :, x0:x0 + 40] = 0
    if with_specials:
        vals = specials(max_depth)
        n = max(1, B * H * W // 100)
        at = rng.choice(B * H * W, size=n, replace=False)
        z.reshape(-1)[at] = vals[rng.integers(0, len(vals), n)]
    return z


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
