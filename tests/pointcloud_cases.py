"""The numpy reference of back-projection (csrc/backproject.hip) and the case tables of its tests.

The arithmetic is restated operation by operation in float32, in the kernel's order, so the GPU tests
compare bit for bit:
    valid = z > z_min and z <= z_max and (conf is None or conf >= conf_min)      (NaN: not valid)
    x = ((float)j - cx) * z / fx        y = ((float)i - cy) * z / fy        z
The packed form is a boolean-mask gather of the organised one: raster order inside an image, images
in batch order."""
import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

# the sweep: a row shorter than a lane's four pixels, the segment edges (256 pixels per wave), more
# than two segments per row; one and several rows and images
SWEEP_W = (1, 3, 4, 5, 63, 255, 256, 257, 261, 513)
SWEEP_H = (1, 2, 9)
SWEEP_B = (1, 2, 3)
SWEEP_LEFT = (0, 1, 2, 3)  # first column of the view inside its allocation: every base alignment
PATTERNS = ("none", "all", "p05", "p50", "holes", "special", "edges")
INVALID = np.array([0.0, -0.0, -1.0, -80.0, np.nan, np.inf, -np.inf], dtype=F32)
COLOR_SPECIAL = np.array([-3.0, 254.5, 255.5, 300.0, np.nan, 0.5, 1.5, 2.5, -0.0, 255.0, np.inf, -np.inf], dtype=F32)


def intrinsics(rng, B=None):
    """(3, 3) or (B, 3, 3) float32 K with non-integer principal points; the entries the kernel must not
    read are poisoned with NaN."""
    n = 1 if B is None else B
    k = np.full((n, 3, 3), np.nan, dtype=F32)
    k[:, 0, 0] = rng.uniform(300, 800, n)
    k[:, 1, 1] = rng.uniform(300, 800, n)
    k[:, 0, 2] = np.floor(rng.uniform(-20, 600, n)) + rng.uniform(0.05, 0.95, n)
    k[:, 1, 2] = np.floor(rng.uniform(-20, 200, n)) + rng.uniform(0.05, 0.95, n)
    return k[0] if B is None else k


def depth_values(rng, B, H, W, pattern, z_min=0.0, z_max=FLT_MAX):
    """(B, H, W) float32 depths under a validity pattern; invalid pixels draw from INVALID."""
    z = rng.uniform(0.5, 80.0, (B, H, W)).astype(F32)
    bad = INVALID[rng.integers(0, len(INVALID), (B, H, W))]
    if pattern == "none":
        return bad
    if pattern == "all":
        return z
    if pattern in ("p05", "p50"):
        keep = rng.random((B, H, W)) < (0.05 if pattern == "p05" else 0.5)
        return np.where(keep, z, bad)
    if pattern == "holes":  # whole rows and whole 256-pixel segments without a valid pixel
        keep = np.ones((B, H, W), dtype=bool)
        keep[:, ::2] = False
        for s in range(0, W, 512):
            keep[:, :, s:s + 256] = False
        if H == 1 and W <= 256:  # keep a few valid pixels in the one segment there is
            keep[:, :, W // 2:] = True
        return np.where(keep, z, bad)
    if pattern == "special":
        return np.where(rng.random((B, H, W)) < 0.5, z, np.resize(INVALID, B * H * W).reshape(B, H, W))
    if pattern == "edges":  # exactly the bounds and their float neighbours
        lo, hi = F32(z_min), F32(z_max)
        pool = np.array([lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf)), hi,
                         np.nextafter(hi, F32(np.inf)), np.nextafter(hi, F32(-np.inf))], dtype=F32)
        return np.where(rng.random((B, H, W)) < 0.5, z, pool[rng.integers(0, len(pool), (B, H, W))])
    raise ValueError(pattern)


def valid_ref(depth, conf=None, conf_min=0.0, z_min=0.0, z_max=FLT_MAX):
    with np.errstate(invalid="ignore"):
        v = (depth > F32(z_min)) & (depth <= F32(z_max))
        if conf is not None:
            v &= conf >= F32(conf_min)
    return v


def map_ref(depth, k, conf=None, conf_min=0.0, z_min=0.0, z_max=FLT_MAX):
    """(xyz (B, 3, H, W) float32 with NaN where not valid, valid (B, H, W) bool). depth (B, H, W)
    float32, k (3, 3) or (B, 3, 3) float32."""
    depth = np.asarray(depth, dtype=F32)
    B, H, W = depth.shape
    k = np.broadcast_to(np.asarray(k, dtype=F32), (B, 3, 3))
    fx, fy, cx, cy = (k[:, a, b].reshape(B, 1, 1) for a, b in ((0, 0), (1, 1), (0, 2), (1, 2)))
    j = np.arange(W, dtype=F32).reshape(1, 1, W)
    i = np.arange(H, dtype=F32).reshape(1, H, 1)
    with np.errstate(all="ignore"):
        x = ((j - cx).astype(F32) * depth).astype(F32) / fx
        y = ((i - cy).astype(F32) * depth).astype(F32) / fy
    assert x.dtype == F32 and y.dtype == F32
    valid = valid_ref(depth, conf, conf_min, z_min, z_max)
    xyz = np.stack([x, y, np.broadcast_to(depth, x.shape)], axis=1).astype(F32)
    xyz[np.broadcast_to(~valid[:, None], xyz.shape)] = np.nan
    return xyz, valid


def color_ref(color, reverse=False):
    """(B, H, W, 3) uint8 in output order from fp32 planes (B, 3, H, W) or uint8 (B, H, W, 3)."""
    color = np.asarray(color)
    if color.dtype == np.uint8:
        c = color
    else:
        with np.errstate(invalid="ignore"):
            q = np.rint(color.astype(F32))
            q = np.where(q > 0, q, F32(0))  # comparisons: NaN -> 0
            q = np.where(q < 255, q, F32(255))
        c = q.astype(np.uint8).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(c[..., ::-1] if reverse else c)


def points_ref(depth, k, conf=None, conf_min=0.0, color=None, reverse=False, z_min=0.0, z_max=FLT_MAX):
    """The packed form: dict(xyz (N, 3) float32, rgb (N, 3) uint8 or None, index (N) int32,
    offsets (B + 1) int32), by a boolean-mask gather of map_ref."""
    xyz, valid = map_ref(depth, k, conf, conf_min, z_min, z_max)
    B, H, W = valid.shape
    pts = xyz.transpose(0, 2, 3, 1)[valid]  # C-order mask: batch, then raster
    rgb = None if color is None else color_ref(color, reverse)[valid]
    index = np.flatnonzero(valid.reshape(-1)).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(valid.reshape(B, -1).sum(1))]).astype(np.int32)
    return dict(xyz=np.ascontiguousarray(pts), rgb=rgb, index=index, offsets=offsets)


def allocation(rng, values, left, fill):
    """values (B, ...rows..., W[, 3]) placed at [:, 1:1+H, left:left+W] of a larger array with an odd
    row length, the rest `fill`; returns (big, slicer) with slicer(big) the view. Works for (B, H, W),
    (B, 3, H, W) and (B, H, W, 3)."""
    v = np.asarray(values)
    if v.ndim == 3:
        B, H, W = v.shape
        shape, cut = (B, H + 2, (W + left + 2) | 1), lambda t: t[:, 1:1 + H, left:left + W]
    elif v.shape[-1] == 3 and v.dtype == np.uint8:
        B, H, W, _ = v.shape
        shape, cut = (B, H + 2, (W + left + 2) | 1, 3), lambda t: t[:, 1:1 + H, left:left + W]
    else:
        B, _, H, W = v.shape
        shape, cut = (B, 3, H + 2, (W + left + 2) | 1), lambda t: t[:, :, 1:1 + H, left:left + W]
    big = np.full(shape, fill, dtype=v.dtype)
    cut(big)[...] = v
    return big, cut
