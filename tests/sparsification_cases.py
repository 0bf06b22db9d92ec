"""The numpy reference of nconv_depth_sparsification (include/nconv.h) and the cases its tests share.

order is np.argsort(key, kind="stable") over the valid pixels in raster order, the terms are np.float32,
and every sum is math.fsum over the kept terms (exactly rounded)."""
import functools
import math
import os
import re

import numpy as np

F32, U32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "realtime-depth-estimation-nconv_amd", "csrc", "sparsification.hip")

# csrc/sparsification.hip (test_sparsification_cpu.py holds them against the file)
THREADS = 256        # kT
SORT_TILE = 256      # kTile: keys per round of a workgroup
MAX_BLOCKS = 64      # kMaxBlocks: workgroups per segment
PREP_TILE = 2048     # kPrepTile: pixels per compaction tile
CHUNK = 256          # kChunk: sorted positions per partial sum

# the smallest shapes at which the sort can go wrong
SMALL = (1, 5, 7)          # less than one tile of anything
# H * W = 19781 > MAX_BLOCKS * SORT_TILE: a fully valid image gives every workgroup a run of two rounds
# (ceil(19781 / 64) = 310 -> 512), the second one partial, over 39 workgroups; 19781 % 256 = 69; ten
# compaction tiles and 78 chunks, the last of each partial
MULTI = (3, 151, 131)
# more chunks (260) than threads: spars_curve's strided loop over the partials takes a second turn
WIDE = (1, 260, 256)
assert MULTI[1] * MULTI[2] > MAX_BLOCKS * SORT_TILE and (MULTI[1] * MULTI[2]) % SORT_TILE
assert WIDE[1] * WIDE[2] > (THREADS + 1) * CHUNK

PATTERNS = ("equal", "four", "top_digit", "bottom_digit", "specials", "sorted", "reverse", "random")


def source_constants():
    """{name: value} of the constexpr ints at the top of csrc/sparsification.hip."""
    text = open(SOURCE).read()
    env = {}
    for name, expr in re.findall(r"^constexpr int (k\w+) = ([^;]+);", text, re.M):
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


def conf_key(conf, uncertainty=False):
    bits = np.ascontiguousarray(conf, dtype=F32).view(U32)
    u = bits ^ np.where(bits >> 31, U32(0xFFFFFFFF), U32(0x80000000)).astype(U32)
    if uncertainty:
        u = ~u
    return np.where(np.isnan(conf), U32(0), u).astype(U32)


def terms(pred, gt, clamp=(0.0, 0.0)):
    """(a, q) in float32: one rounding per operation, the clamp by comparisons."""
    lo = F32(clamp[0]) if clamp[0] else F32(-np.inf)
    hi = F32(clamp[1]) if clamp[1] else F32(np.inf)
    P = np.asarray(pred, dtype=F32)
    P = np.where(P < lo, lo, P)
    P = np.where(P > hi, hi, P)
    with np.errstate(all="ignore"):
        e = (P - np.asarray(gt, dtype=F32)).astype(F32)
        return np.abs(e).astype(F32), (e * e).astype(F32)


def valid_mask(gt, gt_min=0.0, gt_max=0.0):
    gt = np.asarray(gt, dtype=F32)
    v = (gt > 0) & (gt >= F32(gt_min))
    return v & (gt <= F32(gt_max)) if gt_max else v


def steps_k(n, J):
    return [j * n // J for j in range(J)]


def sparsification_ref(pred, gt, conf, steps=100, gt_min=0.0, gt_max=0.0, clamp=(0.0, 0.0), uncertainty=False,
                       sums=True):
    """(curves (B, 2, J, 3) float64, order (B, 2, H * W) int32, n (B,)) of (B, H, W) float32 arrays.
    sums=False leaves the two sums of every point 0 (cases whose terms hold a NaN)."""
    pred, gt, conf = (np.asarray(x, dtype=F32) for x in (pred, gt, conf))
    B, H, W = gt.shape
    curves = np.zeros((B, 2, steps, 3))
    order = np.full((B, 2, H * W), -1, dtype=np.int32)
    n = np.zeros(B, dtype=np.int64)
    for b in range(B):
        pix = np.flatnonzero(valid_mask(gt[b], gt_min, gt_max).reshape(-1))  # raster order
        n[b] = pix.size
        a, q = terms(pred[b], gt[b], clamp)
        a, q = a.reshape(-1)[pix], q.reshape(-1)[pix]
        keys = (conf_key(conf[b].reshape(-1)[pix], uncertainty), ~a.view(U32))
        for o in (0, 1):
            perm = np.argsort(keys[o], kind="stable")
            order[b, o, :pix.size] = pix[perm]
            sa, sq = a[perm].astype(np.float64).tolist(), q[perm].astype(np.float64).tolist()
            for j, k in enumerate(steps_k(pix.size, steps)):
                curves[b, o, j, 0] = pix.size - k
                if sums:
                    curves[b, o, j, 1] = math.fsum(sa[k:])
                    curves[b, o, j, 2] = math.fsum(sq[k:])
    return curves, order, n


def sum_bound(n):
    """The relative error of any summation order of n non-negative doubles against the exact sum."""
    g = max(int(n) - 1, 0) * 2.0 ** -53
    return g / (1.0 - g)


def assert_curves(got, want, n):
    """Counts exact; every sum within sum_bound(n_b) of the exactly rounded one (one more rounding: fsum's)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[..., 0], want[..., 0])
    for b in range(want.shape[0]):
        tol = sum_bound(n[b])
        for k in (1, 2):
            g, w = got[b, :, :, k], want[b, :, :, k]
            err = np.abs(g - w)
            print(f"image {b} sum {k}: n {int(n[b])}, max rel err {np.max(err / np.where(w > 0, w, 1)):.3e}, "
                  f"bound {tol:.3e}")
            assert (err <= tol * w).all(), (b, k, float(err.max()))


def normalised_ref(curves):
    """(2, B, 2, J) float64: the MAE and RMSE curves over their own j = 0 value (SparsificationCurves)."""
    n = curves[..., 0]
    kept = np.where(n > 0, n, 1.0)
    fig = np.stack((curves[..., 1] / kept, np.sqrt(curves[..., 2] / kept)))
    first = fig[..., :1]
    ok = (first > 0) & (n[None, ..., :1] > 0)
    return np.where(ok, fig / np.where(ok, first, 1.0), 0.0)


# ---- inputs ----------------------------------------------------------------------------------------
def ground_truth(shape, seed, valid=(1.0, 0.5, 0.3)):
    """gt in (0, 80] where valid, 0 elsewhere; image b keeps the share valid[b % 3] of its pixels."""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    gt = (rng.random(shape) * 79 + 1).astype(F32)
    for b in range(B):
        gt[b][rng.random((H, W)) >= valid[b % len(valid)]] = 0
    return gt


def confidence(shape, pattern, seed):
    rng = np.random.default_rng(seed + 1000)
    B, H, W = shape
    n = H * W
    if pattern == "equal":
        return np.full(shape, 0.5, dtype=F32)
    if pattern == "four":
        return rng.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=F32), size=shape)
    if pattern == "top_digit":  # every bit pattern below is finite
        return ((rng.integers(0, 256, size=shape).astype(U32) << 24) | U32(0x00123456)).view(F32)
    if pattern == "bottom_digit":
        return (rng.integers(0, 256, size=shape).astype(U32) | U32(0x3F000000)).view(F32)
    if pattern == "specials":
        vals = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-45, 2.0, np.inf], dtype=F32)
        return rng.choice(vals, size=shape)
    if pattern in ("sorted", "reverse"):
        ramp = (np.arange(n, dtype=np.float64) / n).astype(F32)
        return np.broadcast_to((ramp if pattern == "sorted" else ramp[::-1]).reshape(1, H, W), shape).copy()
    assert pattern == "random"
    return rng.random(shape).astype(F32)


@functools.lru_cache(maxsize=None)
def case(shape, pattern, seed=0, steps=100):
    """(pred, gt, conf, reference curves, order, n): computed once and shared; do not write to them."""
    gt = ground_truth(shape, seed)
    rng = np.random.default_rng(seed + 2000)
    pred = (gt + rng.normal(0, 2, size=shape)).astype(F32)
    pred[gt == 0] = (rng.random(shape) * 80).astype(F32)[gt == 0]
    conf = confidence(shape, pattern, seed)
    out = (pred, gt, conf) + sparsification_ref(pred, gt, conf, steps)
    for x in out:
        x.setflags(write=False)
    return out
