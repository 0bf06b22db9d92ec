"""The nearest-sample transform (include/nconv.h, nconv_depth_nearest) restated in numpy by brute force, and
the planes the tests run it on.

The reference does not use the separable decomposition of csrc/nearest.hip: per image it builds the int64
key d2 * (H * W) + pixel number over all (pixel, sample) pairs, in chunks of rows, and takes the smallest,
which is the rule's order (the smallest d2, ties to the smallest pixel number) in one comparison. The key
of the argmin gives d2 and the pixel number back, and all four outputs are derived from those."""
import numpy as np

F32 = np.float32
NO_DIST2 = 0x7FFFFFFF
SHAPES = ((1, 1), (1, 9), (9, 1), (7, 9), (33, 70), (65, 130), (64, 257),
          (131, 66))  # the last: three 64-row segments of the column pass, the third of three rows
DENSITIES = (0.02, 0.4)
FLOORS = (0.0, None, 2.5)
MAX_DISTANCES = (None, 0, 1.5, 5)
LDS_W = 4096  # the widest row csrc/nearest.hip keeps in LDS: wider rows take the other row kernel


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def sample_of(z, floor):
    """The validity of the rule: finite and > floor (None: every finite value)."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > (F32(-np.inf) if floor is None else F32(floor)))


def max_dist2_of(max_distance):
    """The host's max_dist2: floor(r^2) clipped to int32, -1 for None."""
    if max_distance is None:
        return -1
    return int(min(np.floor(float(max_distance) ** 2), NO_DIST2))


def solve(z, floor, chunk=1 << 22):
    """(index, dist2) of z (B, H, W) without a range limit: int32 planes, -1 / NO_DIST2 in an image
    without samples."""
    B, H, W = z.shape
    index = np.full((B, H * W), -1, dtype=np.int32)
    dist2 = np.full((B, H * W), NO_DIST2, dtype=np.int32)
    valid = sample_of(z, floor).reshape(B, -1)
    cols = np.arange(W, dtype=np.int64)
    for b in range(B):
        s = np.flatnonzero(valid[b]).astype(np.int64)
        if s.size == 0:
            continue
        sr, sc = s // W, s % W
        # the key's share that is the same in every row: (c - c')^2 * (H * W) + pixel number, (W, samples)
        key_c = (cols[:, None] - sc[None, :]) ** 2 * (H * W) + s[None, :]
        step = max(1, chunk // (W * s.size))  # rows per chunk
        for r0 in range(0, H, step):
            rows = np.arange(r0, min(H, r0 + step), dtype=np.int64)
            key = key_c[None, :, :] + ((rows[:, None] - sr[None, :]) ** 2 * (H * W))[:, None, :]
            best = key.min(axis=2)  # the argmin's key: d2 and the pixel number come apart again
            index[b, r0 * W:(r0 + len(rows)) * W] = (best % (H * W)).reshape(-1)
            dist2[b, r0 * W:(r0 + len(rows)) * W] = (best // (H * W)).reshape(-1)
    return index.reshape(B, H, W), dist2.reshape(B, H, W)


def finish(z, index, dist2, max_dist2=-1):
    """The four outputs from an unlimited (index, dist2) under the range limit max_dist2."""
    B, H, W = z.shape
    none = (index < 0) | ((dist2 > max_dist2) if max_dist2 >= 0 else False)
    ix = np.where(none, -1, index).astype(np.int32)
    d2 = np.where(none, NO_DIST2, dist2).astype(np.int32)
    flat = z.reshape(B, -1)
    dst = np.take_along_axis(flat, np.maximum(ix, 0).reshape(B, -1).astype(np.int64), axis=1).reshape(B, H, W)
    dst = np.where(none, F32(0), dst).astype(F32)
    dist = np.where(none, F32(np.inf), np.sqrt(np.where(none, 0, d2).astype(F32))).astype(F32)
    return dict(dst=dst, index=ix, dist2=d2, dist=dist)


def nearest_ref(z, floor=0.0, max_distance=None):
    index, dist2 = solve(z, floor)
    return finish(z, index, dist2, max_dist2_of(max_distance))


def single_ref(shape, at, value, max_dist2=-1):
    """In closed form: one sample `value` at pixel `at` = (r0, c0) of every image of shape (B, H, W)."""
    B, H, W = shape
    rr, cc = np.mgrid[0:H, 0:W]
    d2 = np.broadcast_to(((rr - at[0]) ** 2 + (cc - at[1]) ** 2).astype(np.int32), shape)
    z = np.zeros(shape, dtype=F32)
    z[:, at[0], at[1]] = value
    return z, finish(z, np.full(shape, at[0] * W + at[1], dtype=np.int32), d2, max_dist2)


def specials():
    return np.array([np.nan, np.inf, -np.inf, -0.0, -3.0, -1e-40, 1e-40, 2.5, 2.0], dtype=F32)


def plane(B, H, W, seed, density, background=0.0, with_specials=True):
    """(B, H, W) fp32: samples of 0.5 .. 80 m (some at or below 2.5) at `density` on `background` (0.0, or
    NaN so that floor=None leaves an empty background). Image 1 has no sample and image 2 a single one at
    (H - 1, 0). The special values are scattered over image 0 and over the empty image: NaN, +-inf, -0.0,
    negatives, denormals and values <= 2.5, none of which is a sample under the floor that excludes it."""
    rng = np.random.default_rng(seed)
    z = np.where(rng.random((B, H, W)) < density, rng.uniform(0.5, 80.0, (B, H, W)), background).astype(F32)
    sp = specials()
    if B > 1:
        z[1] = background
    if B > 2:
        z[2] = background
        z[2, H - 1, 0] = 41.5
    if with_specials:
        k = min(H * W, 3 * sp.size)
        for b in (0, 1)[:B]:
            at = rng.choice(H * W, size=k, replace=False)
            vals = np.resize(sp, k)
            if b == 1:  # the empty image stays empty under every floor of the sweep
                vals = np.where(np.isfinite(vals) & (np.isnan(background) | (vals > 0)), F32(np.nan), vals)
            z[b].reshape(-1)[at] = vals
    return z


# ---- forced ties ------------------------------------------------------------------------------------
D25 = tuple((dr, dc) for dr, dc in ((-5, 0), (-4, -3), (-4, 3), (-3, -4), (-3, 4), (0, -5), (0, 5), (3, -4), (3, 4),
                                    (4, -3), (4, 3), (5, 0)))  # the twelve offsets of d2 = 25, by pixel number


def forced_planes(H=40, W=70):
    """[(name, plane (1, H, W), centre, expected nearest pixel of the centre)]: every plane holds only the
    samples of its tie, so the centre's nearest sample is decided by the tie rule alone."""
    out = []

    def add(name, centre, offsets, value=7.0):
        z = np.zeros((1, H, W), dtype=F32)
        pts = [(centre[0] + dr, centre[1] + dc) for dr, dc in offsets]
        assert all(0 <= r < H and 0 <= c < W for r, c in pts), name
        for n, (r, c) in enumerate(pts):
            z[0, r, c] = value + n
        out.append((name, z, centre, min(r * W + c for r, c in pts)))

    rng = np.random.default_rng(25)
    for centre in ((10, 20), (31, 63), (32, 64), (20, 64), (5, 5), (H - 6, W - 6)):  # and beside the 64-lane seams
        for k in (1, 2, 5):
            add(f"row pair {k}", centre, ((0, -k), (0, k)))
            add(f"column pair {k}", centre, ((-k, 0), (k, 0)))
            add(f"diamond {k}", centre, ((-k, 0), (0, -k), (0, k), (k, 0)))
            add(f"diamond {k} without its top", centre, ((0, -k), (0, k), (k, 0)))
            add(f"diamond {k}, right and bottom", centre, ((0, k), (k, 0)))
        add("all of d2 = 25", centre, D25)
        for n in range(12):  # subsets of the twelve: equal d2 across different columns
            pick = [o for o in D25 if rng.random() < 0.4] or [D25[n]]
            add(f"d2 = 25 subset {n}", centre, pick)
        add("(3, 4) in a later column against (5, 0)", centre, ((5, 0), (3, 4)))
        add("(-3, 4) against (-3, -4) and (0, -5)", centre, ((-3, 4), (-3, -4), (0, -5)))
        add("(3, -4) above (3, -4)'s mirror in one column", centre, ((3, -4), (-3, -4), (5, 0)))
        # the search's stop: a candidate of d2 = k^2 and a larger pixel number is met first (at a smaller
        # column offset), then a sample of the centre's own row at column offset k, which ties and wins
        for k, (dr, dc) in ((5, (4, 3)), (5, (3, 4)), (5, (5, 0)), (5, (4, -3)), (1, (1, 0)), (2, (2, 0))):
            add(f"stop at k = {k}: ({dr}, {dc}) then (0, {k})", centre, ((dr, dc), (0, k)))
            add(f"stop at k = {k}: ({dr}, {dc}) then (0, -{k})", centre, ((dr, dc), (0, -k)))
    return out


def checkerboard(B, H, W):
    rr, cc = np.mgrid[0:H, 0:W]
    z = np.where((rr + cc) % 2 == 0, (1.0 + rr * W + cc), 0.0).astype(F32)
    return np.broadcast_to(z, (B, H, W)).copy()
