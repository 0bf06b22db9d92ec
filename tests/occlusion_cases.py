"""The numpy reference of the occlusion filter (csrc/occlusion.hip, nconv_depth_occlusion) and the
seeded planes of its tests.

The rule of include/nconv.h restated operation by operation in float32, so the GPU tests compare bit for
bit. For image b and pixel p = (i, j) with value v_p:
    valid(p)    v_p is finite and v_p > floor                  (floor None: -inf, every finite value)
    lim(q)      = v_q + (jump_abs + jump_rel * v_q)            three separate float32 operations: numpy
                                                               rounds each one (no fused multiply-add)
    window(p)   the q != p with |i_q - i_p| <= rh, |j_q - j_p| <= rw inside the image (clipped)
    support(p)  the number of valid q of window(p) with v_p > lim(q)     (strict)
    removed(p)  valid(p) and support(p) >= min_support
    dst[p]      v_p bit for bit where valid and not removed, +0.0 elsewhere
One loop over the window offsets on shifted arrays accumulates support."""
import numpy as np

F32 = np.float32

# The kernel's tile is 32 rows x 64 columns. (2, 71, 139) spans three tiles in both directions: two whole
# ones and a ragged remainder of 7 rows / 11 columns. (3, 37, 71) has a ragged 16-byte tail.
TILE = (32, 64)
SHAPES = ((1, 1, 1), (2, 5, 7), (3, 37, 71), (1, 40, 136), (2, 71, 139))
# the last three exceed the 5 x 7 image of SHAPES[1]
WINDOWS = ((0, 0), (1, 1), (3, 3), (2, 5), (16, 0), (0, 16), (16, 16))
MIN_SUPPORTS = (1, 2, 7)
FLOORS = (0.0, None)
DENSITIES = (0.05, 0.6)
JUMPS = (1.0, 0.0)  # the Python defaults


def valid_of(z, floor):
    fl = F32(-np.inf) if floor is None else F32(floor)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > fl)


def lim_of(z, jump_abs, jump_rel):
    """v + (jump_abs + jump_rel * v), one float32 rounding per operation."""
    z = np.asarray(z, dtype=F32)
    with np.errstate(all="ignore"):
        t = F32(jump_rel) * z
        u = F32(jump_abs) + t
        lim = z + u
    assert lim.dtype == F32
    return lim


def support_of(z, rh, rw, jump_abs, jump_rel, floor):
    """(valid (B, H, W) bool, support (B, H, W) int32)."""
    z = np.asarray(z, dtype=F32)
    B, H, W = z.shape
    valid = valid_of(z, floor)
    lim = lim_of(z, jump_abs, jump_rel)
    support = np.zeros((B, H, W), dtype=np.int32)
    for di in range(-rh, rh + 1):
        for dj in range(-rw, rw + 1):
            if di == 0 and dj == 0:
                continue
            i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)  # p with q = p + (di, dj) inside
            if i0 >= i1 or j0 >= j1:
                continue
            vp = z[:, i0:i1, j0:j1]
            lq = lim[:, i0 + di:i1 + di, j0 + dj:j1 + dj]
            vq = valid[:, i0 + di:i1 + di, j0 + dj:j1 + dj]
            with np.errstate(invalid="ignore"):
                support[:, i0:i1, j0:j1] += vq & (vp > lq)
    return valid, support


def finish(z, valid, support, min_support):
    """dict(dst, removed uint8, counts (B, 2) int32, valid) from the support plane."""
    z = np.asarray(z, dtype=F32)
    removed = valid & (support >= min_support)
    dst = np.where(valid & ~removed, z, F32(0))
    B = z.shape[0]
    counts = np.stack([valid.reshape(B, -1).sum(1), removed.reshape(B, -1).sum(1)], axis=1).astype(np.int32)
    return dict(dst=dst, removed=removed.astype(np.uint8), counts=counts, valid=valid)


def occlusion_ref(z, rh, rw, jump_abs, jump_rel, min_support, floor):
    valid, support = support_of(z, rh, rw, jump_abs, jump_rel, floor)
    return finish(z, valid, support, min_support)


def index_ref(index, r):
    """The index plane after the call: -1 where the pixel is removed or not valid."""
    return np.where((r["removed"] != 0) | ~r["valid"], np.int32(-1), index).astype(np.int32)


def window_min_ref(z, rh, rw, jump_abs, jump_rel, floor):
    """removed for min_support = 1 by the window-minimum formulation, for planes whose valid values are
    >= 0: there lim is monotone in v_q, so the smallest lim of the window is lim of the smallest valid
    value, and the centre (lim(p) >= v_p) may stay in the window."""
    z = np.asarray(z, dtype=F32)
    B, H, W = z.shape
    valid = valid_of(z, floor)
    assert (z[valid] >= 0).all()
    pad = np.full((B, H + 2 * rh, W + 2 * rw), np.inf, dtype=F32)
    pad[:, rh:rh + H, rw:rw + W] = np.where(valid, z, F32(np.inf))
    m = np.full((B, H, W), np.inf, dtype=F32)
    for di in range(2 * rh + 1):
        for dj in range(2 * rw + 1):
            m = np.minimum(m, pad[:, di:di + H, dj:dj + W])
    with np.errstate(invalid="ignore"):
        return valid & np.isfinite(m) & (z > lim_of(m, jump_abs, jump_rel))


def plane(B, H, W, seed, density=0.05, specials=True):
    """A sparse plane (B, H, W) float32: a share `density` of the pixels holds a depth in 1..80, the rest
    0; with specials a few NaN, +-inf, negative, zero-among-valid and denormal entries."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.0, 80.0, (B, H, W)).astype(F32)
    z[rng.random((B, H, W)) >= density] = 0
    if specials:
        vals = np.array([np.nan, np.inf, -np.inf, -3.5, -0.0, 0.0, 1e-40, -1e-40, 3.0e38], dtype=F32)
        n = max(1, min(B * H * W // 6, 40))
        at = rng.choice(B * H * W, size=n, replace=False)
        z.reshape(-1)[at] = vals[rng.integers(0, len(vals), n)]
    return z


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def wall_scene(H=96, W=320, f=200.0):
    """A fronto-parallel wall at 5 m in front of a background at 30 m, scanned from an origin that is
    not the camera's (8 cm above, 27 cm behind, 6 cm beside it: KITTI's offsets and a lateral one).
    The rays go from the scanner through a regular grid on the plane z = 5 m whose spacing is 1.5 px
    in the image; a ray that meets the wall's rectangle returns from there, every other one from the
    background. Camera frame (x right, y down, z forward), m = [K | 0].
    -> dict(points (N, 3) float32, m (3, 4) float32, size, see_through (N) bool: background returns
    whose line of sight from the camera crosses the wall, wall (N) bool)."""
    o = np.array([0.06, -0.08, -0.27])
    step = 1.5 * 5.0 / f
    gx = np.arange(-4.5, 4.5, step)
    gy = np.arange(-1.5, 1.5, step)
    g = np.stack(np.meshgrid(gx, gy, indexing="xy"), axis=-1).reshape(-1, 2)
    g = np.concatenate([g, np.full((len(g), 1), 5.0)], axis=1)
    x0, x1, y0, y1 = -1.0, 0.8, -0.6, 0.7
    wall = (g[:, 0] >= x0) & (g[:, 0] <= x1) & (g[:, 1] >= y0) & (g[:, 1] <= y1)
    far = o + (g - o) * ((30.0 - o[2]) / (5.0 - o[2]))
    pts = np.where(wall[:, None], g, far)
    seen_at_5 = pts[:, :2] * (5.0 / pts[:, 2:3])  # where the camera's line of sight crosses z = 5
    behind = (seen_at_5[:, 0] >= x0) & (seen_at_5[:, 0] <= x1) & (seen_at_5[:, 1] >= y0) & (seen_at_5[:, 1] <= y1)
    m = np.array([[f, 0.0, (W - 1) / 2, 0.0], [0.0, f, (H - 1) / 2, 0.0], [0.0, 0.0, 1.0, 0.0]], dtype=F32)
    return dict(points=pts.astype(F32), m=m, size=(H, W), see_through=~wall & behind, wall=wall)
