"""The summation order of the tiled losses (csrc/wave_ops.h) restated in numpy, so that a loss can be
held to it bit for bit from its per-element fp32 terms (test_gpu_confloss.py, test_gpu_warp.py).

First level, float32, one workgroup of 256 threads per 16 x 64 tile (terms outside the plane are 0):
  thread_sums     a thread's four terms in order, ((t0 + t1) + t2) + t3
  wave_sum        the xor butterfly over a wave's 64 lanes: v += v[lane ^ 32], then ^ 16, 8, 4, 2, 1
  tile partial    ((wave 0 + wave 1) + wave 2) + wave 3
Second level, float64, one wave per image (image_tile_sums):
  lane l adds the image's tiles l, l + 64, .. in that order, then wave_sum; the images are added in
  order; L = float32(sum / den).

Which four terms a thread owns is the kernel's: QUAD (conf_loss.hip, metrics.hip: thread t owns row
t >> 4, columns 4 (t & 15) .. + 3) or ROWS (view_warp.hip: lane = column, wave w owns rows w, w + 4,
w + 8, w + 12). A leading 0 + t0 (view_warp.hip) changes no bit: its terms are never -0.
"""
import numpy as np

TH, TW = 16, 64
f32 = np.float32


def QUAD(tile):
    """(16, 64) -> (256, 4): thread t = 16 row + column / 4."""
    return tile.reshape(TH * TW // 4, 4)


def ROWS(tile):
    """(16, 64) -> (256, 4): thread t = 64 w + column, its terms the rows w + 4 r."""
    return tile.reshape(4, 4, TW).transpose(1, 2, 0).reshape(TH * TW // 4, 4)


def wave_sum(v):
    """v (.., 64): every lane's total after the butterfly (the dtype's own additions)."""
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ m]
    return v


def thread_sums(t):
    return ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]


def tile_partial(tile, threads):
    """One tile's (16, 64) float32 terms -> its float32 partial."""
    assert tile.dtype == f32 and tile.shape == (TH, TW)
    w = wave_sum(thread_sums(threads(tile)).reshape(4, 64))[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def tile_partials(terms, threads):
    """terms (B, H, W) float32 -> (B, tiles) float32, an image's tiles row-major."""
    B, H, W = terms.shape
    nth, ntw = -(-H // TH), -(-W // TW)
    pad = np.zeros((B, nth * TH, ntw * TW), dtype=f32)
    pad[:, :H, :W] = terms
    return np.array([[tile_partial(pad[b, i * TH:(i + 1) * TH, j * TW:(j + 1) * TW], threads)
                      for i in range(nth) for j in range(ntw)] for b in range(B)], dtype=f32)


def image_sum(part):
    """One image's float32 tile partials -> its float64 sum."""
    lanes = np.zeros(64, dtype=np.float64)
    for t, p in enumerate(part):  # ascending t: lane t % 64 meets its tiles in the order t, t + 64, ..
        lanes[t % 64] += np.float64(p)
    return wave_sum(lanes)[0]


def finalize(part, den):
    """(B, tiles) float32 partials -> float32(sum / den), the images added in order."""
    acc = np.float64(0.0)
    for b in range(part.shape[0]):
        acc += image_sum(part[b])
    return f32(acc / np.float64(den))


def loss(terms, den, threads):
    terms = np.asarray(terms)
    assert terms.dtype == f32 and terms.ndim == 3
    return finalize(tile_partials(terms, threads), den)


def same_bits(a, b):
    return f32(a).tobytes() == f32(b).tobytes()
