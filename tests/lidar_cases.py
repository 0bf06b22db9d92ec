"""The numpy reference of the LiDAR projection (csrc/lidar_project.hip) and the seeded scans of its
tests.

The arithmetic is restated operation by operation in float32, in the kernel's order, so the GPU tests
compare bit for bit. Per point p = (x, y, z) of image b and row r of b's 3 x 4 matrix:
    dot(r, p) = ((r0 * x + r1 * y) + r2 * z) + r3            (numpy has no fused multiply-add)
    a, b, c = the three dots;  u = a / c, v = b / c;  fj = rint(u), fi = rint(v)   (ties to even)
    valid = c > z_min and c <= z_max and 0 <= fj <= W - 1 and 0 <= fi <= H - 1     (NaN: not valid)
A pixel keeps the valid point with the smallest (bits(c), row): a lexsort, so the winner among
bit-equal depths is the smallest row number. np.minimum.at serves as a cross-check of the depths only."""
import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

# (B, H, W, rows per image): the tiny images force hundreds of collisions per pixel, 37 x 71 has a
# ragged 16-byte tail, 20000 rows are 79 blocks
SWEEP = ((1, 1, 1, 5), (2, 5, 7, 300), (3, 37, 71, 4000), (1, 40, 136, 20000))


def image_of_rows(offsets, n_rows):
    """Image of every row: the entries of offsets that are <= row, less one; -1 or B: no image."""
    off = np.asarray(offsets, dtype=np.int64)
    return np.searchsorted(off, np.arange(n_rows, dtype=np.int64), side="right") - 1


def project_terms(points, offsets, m, dtype=F32):
    """(img, a, b, c, u, v) of every row in `dtype` arithmetic, m (3, 4) or (B, 3, 4)."""
    pts = np.asarray(points)
    off = np.asarray(offsets, dtype=np.int64)
    B = len(off) - 1
    mm = np.broadcast_to(np.asarray(m), (B, 3, 4)).astype(dtype)
    img = image_of_rows(off, len(pts))
    mb = mm[np.clip(img, 0, B - 1)]
    x, y, z = (pts[:, k].astype(dtype) for k in range(3))

    def dot(r):
        p0, p1, p2 = mb[:, r, 0] * x, mb[:, r, 1] * y, mb[:, r, 2] * z
        return ((p0 + p1) + p2) + mb[:, r, 3]

    with np.errstate(all="ignore"):
        a, b, c = dot(0), dot(1), dot(2)
        u, v = a / c, b / c
    assert u.dtype == dtype and c.dtype == dtype
    return img, a, b, c, u, v


def valid_pixels(img, c, u, v, B, H, W, z_min=0.0, z_max=FLT_MAX):
    """(valid, pixel index (b * H + i) * W + j, -1 where not valid) from float comparisons."""
    t = c.dtype.type
    with np.errstate(invalid="ignore"):
        fj, fi = np.rint(u), np.rint(v)
        ok = (img >= 0) & (img < B) & (c > t(z_min)) & (c <= t(z_max))
        ok &= (fj >= 0) & (fj <= t(W - 1)) & (fi >= 0) & (fi <= t(H - 1))
    pix = np.full(len(c), -1, dtype=np.int64)
    pix[ok] = (img[ok] * H + fi[ok].astype(np.int64)) * W + fj[ok].astype(np.int64)
    return ok, pix


def project_ref(points, offsets, m, size, z_min=0.0, z_max=FLT_MAX):
    """dict(depth (B, 1, H, W) float32, index (B, H, W) int32, c (N) float32, pix (N) int64 with -1
    where the row is not valid)."""
    H, W = size
    B = len(offsets) - 1
    img, _, _, c, u, v = project_terms(np.asarray(points, dtype=F32), offsets, np.asarray(m, dtype=F32), F32)
    ok, pix = valid_pixels(img, c, u, v, B, H, W, z_min, z_max)
    rows = np.flatnonzero(ok)
    bits = c[rows].view(np.uint32)
    order = np.lexsort((rows, bits, pix[rows]))  # by pixel, then bits(c), then row
    ps = pix[rows][order]
    first = np.ones(len(ps), dtype=bool)
    first[1:] = ps[1:] != ps[:-1]
    depth = np.zeros(B * H * W, dtype=F32)
    index = np.full(B * H * W, -1, dtype=np.int32)
    depth[ps[first]] = c[rows][order][first]
    index[ps[first]] = rows[order][first].astype(np.int32)
    # cross-check of the depths: the unsigned minimum of the bit patterns
    zb = np.full(B * H * W, 0xFFFFFFFF, dtype=np.uint32)
    np.minimum.at(zb, pix[rows], bits)
    zb[zb == 0xFFFFFFFF] = 0
    assert np.array_equal(zb, depth.view(np.uint32))
    return dict(depth=depth.reshape(B, 1, H, W), index=index.reshape(B, H, W), c=c, pix=pix)


# ---- seeded cameras and scans ------------------------------------------------------------------------
def camera(rng, H, W):
    """A KITTI-like rectified camera and velodyne pose scaled to an H x W image: dict(P (3, 4), R
    (3, 3), T (3), m64 = P . [R | T; 0 1] in float64, m = its float32 rounding)."""
    s = W / 1216.0
    f = 721.5377 * s * rng.uniform(0.95, 1.05)
    P = np.array([[f, 0.0, (W - 1) / 2 + rng.uniform(-0.03, 0.03) * W, 44.857 * s],
                  [0.0, f, (H - 1) / 2 + rng.uniform(-0.03, 0.03) * H, 0.2164 * s],
                  [0.0, 0.0, 1.0, 0.002746]])
    # velodyne x forward, y left, z up -> camera z forward, x right, y down, tilted by about a degree
    base = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    ax, ay, az = rng.uniform(-0.02, 0.02, 3)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R = rx @ ry @ rz @ base
    T = np.array([-0.004, -0.076, -0.27]) + rng.uniform(-0.01, 0.01, 3)
    tr = np.eye(4)
    tr[:3, :3], tr[:3, 3] = R, T
    m64 = P @ tr
    return dict(P=P, R=R, T=T, m64=m64, m=m64.astype(F32))


def rows_for(rng, cam, H, W, n, inside=0.8, c_lo=2.0, c_hi=80.0):
    """n velodyne-frame points (n, 3) float64: a share `inside` aimed at uniformly placed image
    positions at camera depth c in [c_lo, c_hi], the rest around the image or behind the camera."""
    aim = rng.random(n) < inside
    u = np.where(aim, rng.uniform(-0.5, W - 0.5, n), rng.uniform(-W, 2.0 * W, n))
    v = np.where(aim, rng.uniform(-0.5, H - 0.5, n), rng.uniform(-H, 2.0 * H, n))
    c = rng.uniform(c_lo, c_hi, n)
    c = np.where(~aim & (rng.random(n) < 0.3), -c, c)
    P = cam["P"]
    zc = c - P[2, 3]
    xc = (u * c - P[0, 2] * zc - P[0, 3]) / P[0, 0]
    yc = (v * c - P[1, 2] * zc - P[1, 3]) / P[1, 1]
    return (np.stack([xc, yc, zc], axis=1) - cam["T"]) @ cam["R"]  # R^T (Xc - T), row-wise


def scan(rng, B, H, W, rows, stride=4, shared_m=False, inside=0.8):
    """A batch of B scans of `rows` rows each: (points (B * rows, stride) float32, offsets (B + 1)
    int32, m (3, 4) or (B, 3, 4) float32, cams). Column 3 is an intensity; columns past it, which the
    kernel must not read into the result, are NaN."""
    cams = [camera(rng, H, W)] * B if shared_m else [camera(rng, H, W) for _ in range(B)]
    pts = np.full((B * rows, stride), np.nan, dtype=F32)
    for b in range(B):
        pts[b * rows:(b + 1) * rows, :3] = rows_for(rng, cams[b], H, W, rows, inside).astype(F32)
    if stride > 3:
        pts[:, 3] = rng.random(B * rows).astype(F32)
    offsets = (np.arange(B + 1) * rows).astype(np.int32)
    m = cams[0]["m"] if shared_m else np.stack([c["m"] for c in cams])
    return pts, offsets, m, cams
