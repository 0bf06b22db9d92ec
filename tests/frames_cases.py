"""The numpy reference of nconv_frame_ingest / nconv_depth_export_u16 and the cases of their sweeps
(tests/test_frames_cpu.py, tests/test_gpu_frames.py). The arithmetic is exact, so every comparison
against these is for equality."""
import numpy as np

# depth_decode name -> (shift, scale) of an integer plane; a float32 plane is copied (0, 1)
DECODES = {"reference": {np.dtype(np.uint16): (8, 1.0 / 256.0), np.dtype(np.uint8): (0, 1.0 / 256.0)},
           "kitti16": {np.dtype(np.uint16): (0, 1.0 / 256.0), np.dtype(np.uint8): (0, 1.0 / 256.0)}}


def decode_of(depth_decode, dtype):
    if isinstance(depth_decode, str):
        return (0, 1.0) if np.dtype(dtype) == np.float32 else DECODES[depth_decode][np.dtype(dtype)]
    return depth_decode


def rgb_ref(src, reverse=True):
    """uint8 (B, h, w, 3) -> fp32 (B, 3, h, w), the channels reversed (RGB -> BGR planes) or kept."""
    s = src[..., ::-1] if reverse else src
    return np.ascontiguousarray(s.transpose(0, 3, 1, 2).astype(np.float32))


def plane_ref(v, shift, scale):
    """(B, h, w) uint8 / uint16 / float32 -> fp32 (B, 1, h, w) = float(v >> shift) * scale."""
    if v.dtype == np.float32:
        assert shift == 0
        f = v * np.float32(scale)
    else:
        f = (v >> shift).astype(np.float32) * np.float32(scale)
    assert f.dtype == np.float32
    return np.ascontiguousarray(f[:, None])


def ingest_ref(rgb=None, depth=None, gt=None, depth_decode="reference", reverse_rgb=True):
    out = {}
    if rgb is not None:
        out["rgb"] = rgb_ref(rgb, reverse_rgb)
    for key, v in (("depth", depth), ("gt", gt)):
        if v is not None:
            out[key] = plane_ref(v, *decode_of(depth_decode, v.dtype))
    return out


def export_ref(d, scale=256.0):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(d.astype(np.float32) * np.float32(scale))
        q[np.isnan(q)] = 0
        return np.clip(q, 0, 65535).astype(np.uint16)


# ---- ingest sweep ------------------------------------------------------------------------------------
INGEST_B = (1, 2, 3)
INGEST_H = (1, 3, 17)
INGEST_W = (1, 3, 4, 5, 16, 17, 63, 64, 65, 130, 255, 256, 257, 261)
INGEST_LEFT = (0, 1, 2, 3, 5)
PLANE_DTYPES = (np.uint16, np.uint8, np.float32)
SPECIAL_U16 = (0, 255, 256, 65535)


def raw_allocation(rng, B, h, w, left, dtype, channels=None):
    """(big, view): a random (B, h + 2, w + left + 3[, 3]) array and its [:, 1:1+h, left:left+w] slice;
    the slice's first values are 0, 255, 256, 65535 (as far as the dtype and its size go)."""
    shape = (B, h + 2, w + left + 3) + ((channels,) if channels else ())
    if np.dtype(dtype) == np.float32:
        big = (rng.random(shape, dtype=np.float32) * 200 - 20).astype(np.float32)
    else:
        big = rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=np.int64).astype(dtype)
    view = big[:, 1:1 + h, left:left + w]
    if np.dtype(dtype) != np.float32:
        flat = [(b, i, j) for b in range(B) for i in range(h) for j in range(w)]
        for (b, i, j), s in zip(flat, [s for s in SPECIAL_U16 if s <= np.iinfo(dtype).max]):
            view[b, i, j] = s
    return big, view


# ---- export sweep ------------------------------------------------------------------------------------
EXPORT_B = (1, 2, 3)
EXPORT_H = (1, 5, 17)
EXPORT_W = (1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 255, 256, 257, 261)
# exact ties (k + 0.5) / 256 for even and odd k, -0.0, negatives, above 255.998 (-> 65535), +-inf, NaN
EXPORT_SPECIAL = np.array([(2 + 0.5) / 256, (3 + 0.5) / 256, (0 + 0.5) / 256, (1 + 0.5) / 256, (65534 + 0.5) / 256,
                           (65533 + 0.5) / 256, -0.0, -0.001, -3.5, -1e30, 255.9981, 255.999, 256.0, 300.0, 1e30,
                           np.inf, -np.inf, np.nan, 0.0, 1.0 / 512, 80.0], dtype=np.float32)


def export_values(rng, B, H, W):
    """(B, 1, H, W) fp32: random depths in [0, 90) with the special values dealt round-robin over
    the batch (every one present when B * H * W allows, each case starting at another one)."""
    d = (rng.random((B, 1, H, W), dtype=np.float32) * 90).astype(np.float32)
    flat = d.reshape(-1)
    n = flat.size
    start = (B * 7 + H * 3 + W) % len(EXPORT_SPECIAL)
    k = min(n, len(EXPORT_SPECIAL))
    pos = rng.permutation(n)[:k]
    flat[pos] = np.roll(EXPORT_SPECIAL, -start)[:k]
    return d
