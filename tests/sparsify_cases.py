"""The numpy reference of nconv_depth_sparsify (include/nconv.h states the rule) and the inputs the
sparsify tests share: vectorised Philox4x32-10, the candidates, the selection as a lexsort on
(w0 & key_mask, p) and the noise with one explicit fp32 rounding per operation."""
import math

import numpy as np

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
FLT_MAX = float(np.finfo(np.float32).max)
ALL, COUNT, COUNT_DEV, FRACTION = 0, 1, 2, 3

M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = U64(0xFFFFFFFF)
S32 = U64(32)

# (counter, key, words) of Philox4x32-10
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)

# the GPU sweep: (B, H, W); (2, 64, 257) takes several workgroups per image and a ragged last tile
SHAPES = ((1, 1, 1), (1, 2, 3), (3, 9, 13), (2, 37, 71), (2, 64, 257))
BIG = (2, 352, 1216)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four uint32 words for counters c0..c3 (arrays or scalars, broadcast) and key (k0, k1)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=U64) & LOW for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # below 2^64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ U64(k0), p1 & LOW, (p0 >> S32) ^ c3 ^ U64(k1), p0 & LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(U32) for c in (c0, c1, c2, c3))


def words_hex(w):
    return " ".join(f"{int(v):08x}" for v in w)


def noise_threshold(noise_frac):
    return min(max(int(math.floor(float(noise_frac) * 4294967296.0)), 0), 0xFFFFFFFF)


def candidates(depth, mask=None, floor=0.0):
    """(B, H, W) bool. depth (B, H, W) fp32; mask (H, W) or (B, H, W) uint8 or None; floor None: all_pixels."""
    B, H, W = depth.shape
    c = np.ones((B, H, W), dtype=bool)
    if floor is not None:
        with np.errstate(invalid="ignore"):
            c = (depth > F32(floor)) & (depth <= F32(FLT_MAX))
    if mask is not None:
        c = c & (np.broadcast_to(mask, (B, H, W)) != 0)
    return c


def target(mode, C, b, n=None, keep=None):
    if mode == ALL:
        return C
    if mode == COUNT:
        return min(int(n), C)
    if mode == COUNT_DEV:
        return min(max(int(n[b]), 0), C)
    return int(math.floor(float(F32(keep)) * float(C)))


def sparsify_ref(depth, n=None, *, keep=None, seed=0, draw=0, mask=None, floor=0.0, noise_frac=0.0, noise_amp=0.1,
                 key_mask=0xFFFFFFFF, detail=False):
    """(out (B, H, W) fp32, kept (B,) int32) for depth (B, H, W) fp32; n an int or a length-B sequence
    (COUNT_DEV). detail: also the kept and the noisy masks (B, H, W) bool."""
    depth = np.ascontiguousarray(depth, dtype=F32)
    B, H, W = depth.shape
    assert n is None or keep is None
    mode = ALL if n is None and keep is None else FRACTION if keep is not None else \
        COUNT if np.ndim(n) == 0 else COUNT_DEV
    cand = candidates(depth, mask, floor)
    p = np.arange(H * W, dtype=U64)
    out = np.zeros((B, H, W), dtype=F32)
    kept = np.zeros(B, dtype=np.int32)
    keep_map = np.zeros((B, H * W), dtype=bool)
    noisy_map = np.zeros((B, H * W), dtype=bool)
    thr = noise_threshold(noise_frac)
    for b in range(B):
        w0, w1, w2, _ = philox4x32_10(p, b, int(draw) & 0xFFFFFFFF, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        cb = cand[b].reshape(-1)
        idx = np.flatnonzero(cb)
        nb = target(mode, idx.size, b, n, keep)
        order = np.lexsort((idx, w0[idx] & U32(key_mask)))  # the last key is the primary one
        sel = idx[order[:nb]]
        kept[b] = nb
        keep_map[b, sel] = True
        d = depth[b].reshape(-1)[sel]
        noisy = w1[sel] < thr  # thr = 0: none
        u = (w2[sel] >> U32(8)).astype(F32) * F32(2.0 ** -24)
        s = F32(2.0) * u - F32(1.0)
        with np.errstate(invalid="ignore", over="ignore"):
            r = (F32(noise_amp) * s).astype(F32)
            t = (d * r).astype(F32)
            v = (d + t).astype(F32)
        o = out[b].reshape(-1)
        o[sel] = np.where(noisy, v, d)
        # np.where copies d's bits where not noisy
        noisy_map[b, sel[noisy]] = True
    if detail:
        return out, kept, keep_map.reshape(B, H, W), noisy_map.reshape(B, H, W)
    return out, kept


def same_bits(got, ref, noisy=None):
    """got == ref bit for bit, except that where a noisy value is a NaN (d not finite) any NaN will do."""
    g, r = np.ascontiguousarray(got, dtype=F32).view(U32), np.ascontiguousarray(ref, dtype=F32).view(U32)
    ok = g == r
    if noisy is not None:
        ok = ok | (noisy & np.isnan(ref) & np.isnan(got))
    return bool(ok.all())


def plane(B, H, W, seed=0, density=0.6, specials=True):
    """(B, H, W) fp32 depth with empty pixels and, with specials, -0.0, negatives, NaN, +-inf and FLT_MAX."""
    rng = np.random.default_rng(seed)
    z = (rng.random((B, H, W)) * 79.0 + 1.0).astype(F32)
    z[rng.random((B, H, W)) >= density] = 0.0
    if specials and H * W >= 12:
        flat = z.reshape(B, -1)
        for b in range(B):
            at = rng.choice(H * W, size=6, replace=False)
            flat[b, at] = np.array([-0.0, -3.5, np.nan, np.inf, -np.inf, FLT_MAX], dtype=F32)
    return z


def masks(B, H, W, seed=1):
    """A shared (H, W) and a per-image (B, H, W) uint8 mask with values 0, 1 and 255."""
    rng = np.random.default_rng(seed)
    pick = np.array([0, 1, 255], dtype=np.uint8)
    return pick[rng.integers(0, 3, (H, W))], pick[rng.integers(0, 3, (B, H, W))]


def chi2_tiles(keep_map, th=44, tw=76):
    """Pearson's statistic of the kept pixels of one (H, W) image over its grid of th x tw tiles."""
    H, W = keep_map.shape
    assert H % th == 0 and W % tw == 0
    counts = keep_map.reshape(H // th, th, W // tw, tw).sum(axis=(1, 3)).astype(np.float64)
    e = keep_map.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())
