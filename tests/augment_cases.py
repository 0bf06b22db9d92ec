"""The numpy reference of nconv_frame_augment (include/nconv.h states the rule) and the inputs the augment
tests share: the draw of one image (params_ref), the whole call (augment_ref) with one explicit fp32
rounding per operation, and source builders that plant NaN, +-inf, -0.0 and denormals in the planes."""
import math

import numpy as np

from sparsify_cases import philox4x32_10

F32 = np.float32
U32 = np.uint32
RANDOM, CENTER, MIN, MAX = 0, 1, 2, 3
MODES = {"random": RANDOM, "center": CENTER, "min": MIN, "max": MAX}

# the GPU sweep: (H, W) -> (h, w)
GEOMETRIES = (((7, 13), (5, 9)), ((7, 13), (7, 13)), ((7, 13), (1, 1)), ((6, 16), (4, 8)), ((5, 11), (5, 3)),
              ((9, 20), (3, 17)))


def flip_threshold(p):
    return min(max(int(math.floor(float(p) * 4294967296.0)), 0), 1 << 32)


def _offset(mode, word, full, part):
    if mode == RANDOM:
        return (int(word) * (full - part + 1)) >> 32
    if mode == CENTER:
        return (full - part) // 2
    return full - part if mode == MAX else 0


def _gain(amp, x):
    u = F32(int(x) >> 8) * F32(2.0 ** -24)
    s = F32(F32(2.0) * u) - F32(1.0)
    t = F32(F32(amp) * s)
    return F32(F32(1.0) + t)


def params_ref(seed, draw, b, H, W, h, w, modes=(RANDOM, RANDOM), flip=0.5, brightness=0.0, contrast=0.0, color=0.0):
    """(y0, x0, flip, gains (5,) fp32 {g_b, g_c, gain_0, gain_1, gain_2}) of image b. flip: a probability."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    wd = [int(v) for v in philox4x32_10(b, 0, int(draw) & 0xFFFFFFFF, 1, *key)]
    jt = [int(v) for v in philox4x32_10(b, 1, int(draw) & 0xFFFFFFFF, 1, *key)]
    y0, x0 = _offset(modes[0], wd[0], H, h), _offset(modes[1], wd[1], W, w)
    fl = int(wd[2] < flip_threshold(flip))
    if F32(brightness) == 0 and F32(contrast) == 0 and F32(color) == 0:
        gains = np.ones(5, dtype=F32)
    else:
        gains = np.array([_gain(brightness, jt[0]), _gain(contrast, jt[1]), _gain(color, wd[3]), _gain(color, jt[2]),
                          _gain(color, jt[3])], dtype=F32)
    return y0, x0, fl, gains


def jitter_ref(v, g_b, gain, g_c, pivot=127.5, rgb_max=255.0):
    """The six operations on an fp32 array, one rounding each; the clamp by comparisons."""
    with np.errstate(all="ignore"):
        a = (v * F32(g_b)).astype(F32)
        a = (a * F32(gain)).astype(F32)
        a = (a - F32(pivot)).astype(F32)
        a = (a * F32(g_c)).astype(F32)
        a = (a + F32(pivot)).astype(F32)
        a = np.where(a > 0, a, F32(0.0))
        return np.where(a < F32(rgb_max), a, F32(rgb_max)).astype(F32)


def window(x, y0, x0, h, w, flip):
    """x[..., y0:y0 + h, x0:x0 + w], mirrored left to right under flip: a copy of the bits."""
    v = x[..., y0:y0 + h, x0:x0 + w]
    return np.ascontiguousarray(v[..., ::-1] if flip else v)


def augment_ref(size, rgb=None, planes=(), mask=None, k=None, *, src_size=None, B=None, seed=0, draw=0,
                modes=(RANDOM, RANDOM), flip=0.5, brightness=0.0, contrast=0.0, color=0.0, pivot=127.5,
                rgb_max=255.0):
    """rgb (B, 3, H, W) fp32, planes a dict name -> (B, H, W) fp32, mask (H, W) or (B, H, W) uint8, k
    (B, 3, 3) fp32. Returns a dict: 'rgb' (B, 3, h, w), every plane and 'mask' (B, h, w), 'k', 'params'
    (B, 4) int32 and 'gains' (B, 5) fp32."""
    h, w = size
    planes = dict(planes)
    if src_size is None:
        src_size = next(t for t in (rgb, *planes.values(), mask) if t is not None).shape[-2:]
    H, W = src_size
    if B is None:
        batched = (rgb, *planes.values(), k, mask if mask is not None and mask.ndim == 3 else None)
        B = next((t.shape[0] for t in batched if t is not None), 1)
    jitter = not (F32(brightness) == 0 and F32(contrast) == 0 and F32(color) == 0)
    out = {"params": np.zeros((B, 4), dtype=np.int32), "gains": np.zeros((B, 5), dtype=F32)}
    if rgb is not None:
        out["rgb"] = np.zeros((B, 3, h, w), dtype=F32)
    for n in planes:
        out[n] = np.zeros((B, h, w), dtype=F32)
    if mask is not None:
        out["mask"] = np.zeros((B, h, w), dtype=np.uint8)
    if k is not None:
        out["k"] = np.array(k, dtype=F32, copy=True)
    for b in range(B):
        y0, x0, fl, gains = params_ref(seed, draw, b, H, W, h, w, modes, flip, brightness, contrast, color)
        out["params"][b] = (y0, x0, fl, 0)
        out["gains"][b] = gains
        if rgb is not None:
            v = window(rgb[b], y0, x0, h, w, fl)
            if jitter:
                v = np.stack([jitter_ref(v[c], gains[0], gains[2 + c], gains[1], pivot, rgb_max) for c in range(3)])
            out["rgb"][b] = v
        for n, p in planes.items():
            out[n][b] = window(p[b], y0, x0, h, w, fl)
        if mask is not None:
            out["mask"][b] = window(mask if mask.ndim == 2 else mask[b], y0, x0, h, w, fl)
        if k is not None:
            cx1 = F32(k[b, 0, 2]) - F32(x0)
            cy1 = F32(k[b, 1, 2]) - F32(y0)
            out["k"][b, 0, 2] = F32(w - 1) - cx1 if fl else cx1
            out["k"][b, 1, 2] = cy1
    return out


def same_bits(got, ref):
    """got == ref bit for bit (fp32 compared as uint32, so NaN payloads and the sign of zero count)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    if got.dtype == F32:
        got, ref = got.view(U32), ref.view(U32)
    return bool((got == ref).all())


SPECIALS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF,
                     0x7F7FFFFF], dtype=U32).view(F32)  # NaNs with payloads, +-inf, -0.0, denormals, FLT_MAX


def plane(B, H, W, seed=0, density=0.6, specials=True):
    """(B, H, W) fp32 sparse depth; with specials, NaN payloads, +-inf, -0.0 and denormals planted."""
    rng = np.random.default_rng(seed)
    z = (rng.random((B, H, W)) * 79.0 + 1.0).astype(F32)
    z[rng.random((B, H, W)) >= density] = 0.0
    if specials:
        flat = z.reshape(B, -1)
        n = min(len(SPECIALS), H * W)
        for b in range(B):
            flat[b, rng.choice(H * W, size=n, replace=False)] = SPECIALS[:n]
    return z


def image(B, H, W, seed=0):
    """(B, 3, H, W) fp32 RGB with finite values in [0, 255], whole numbers and fractions, 0 and 255 included."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (B, 3, H, W)).astype(F32)
    frac = rng.random((B, 3, H, W)) < 0.3
    v[frac] = (rng.random(int(frac.sum())) * 255.0).astype(F32)
    return v


def mask_u8(B, H, W, seed=1):
    """(B, H, W) uint8 with values 0, 1, 7 and 255."""
    rng = np.random.default_rng(seed)
    return np.array([0, 1, 7, 255], dtype=np.uint8)[rng.integers(0, 4, (B, H, W))]


def intrinsics(B, H, W, seed=2):
    """(B, 3, 3) fp32: a pinhole camera per image with a fractional principal point."""
    rng = np.random.default_rng(seed)
    k = np.zeros((B, 3, 3), dtype=F32)
    k[:, 0, 0] = 700.0 + rng.random(B) * 30
    k[:, 1, 1] = 705.0 + rng.random(B) * 30
    k[:, 0, 2] = W / 2.0 + rng.random(B) * 3 - 1.5
    k[:, 1, 2] = H / 2.0 + rng.random(B) * 3 - 1.5
    k[:, 2, 2] = 1.0
    k[:, 0, 1] = 0.001  # a skew, copied through
    return k
