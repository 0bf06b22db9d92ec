"""The numpy reference of the surface normals (csrc/normals.hip, the contract in include/nconv.h)
and the surfaces of its tests.

Built on pointcloud_cases.map_ref / valid_ref (validity V and point P of a pixel) and restated one
float32 rounding at a time, in the kernel's order, so the GPU tests compare bit for bit:
    tol       = jump_abs + jump_rel * z
    usable(n) = V(n) and (gate off or |z_n - z| <= tol)           gate off: jump_rel == jump_abs == 0
    tu        = P(R) - P(L) | P(R) - P(c) | P(c) - P(L)           both | only R | only L usable
    tv        likewise from D (below) and T (above)
    c         = tv x tu;  d = (cx Px + cy Py) + cz Pz;  d > 0: c = -c
    l         = sqrt((cx cx + cy cy) + cz cz);  n = c / l  iff  l > 0 and l < inf
The packed form and the picture are derived from the (B, 3, H, W) map with NaN where there is none."""
import numpy as np

import pointcloud_cases as PC

F32 = np.float32
FLT_MAX = PC.FLT_MAX

# Worst angle (rad) between the float32 reference and the analytic plane normal over the three tilts of
# plane_cases() at (9, 261), measured on the CPU by test_normals_cpu.py::test_reference_against_analytic_plane
# (which prints it): 3.1254e-5. The tolerance is twice that.
PLANE_ANGLE_MEASURED = 3.1254e-5
PLANE_ANGLE_TOL = 2.0 * PLANE_ANGLE_MEASURED

# the GPU sweep
SWEEP_W = (1, 2, 3, 4, 5, 63, 255, 256, 257, 261, 513)
SWEEP_H = (1, 2, 3, 9)
SWEEP_B = (1, 3)
SWEEP_LEFT = (0, 1, 2, 3)
GATES = ((0.0, 0.0), (0.1, 0.0), (0.0, 0.5))  # (jump_rel, jump_abs): off, relative, absolute


def _shift(a, di, dj, fill):
    """a[..., i + di, j + dj] with `fill` outside the image (di, dj in -1, 0, 1)."""
    H, W = a.shape[-2:]
    pad = [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)]
    p = np.pad(a, pad, constant_values=fill)
    return p[..., 1 + di:1 + di + H, 1 + dj:1 + dj + W]


def normals_ref(depth, k, conf=None, conf_min=0.0, z_min=0.0, z_max=FLT_MAX, jump_rel=0.1, jump_abs=0.0):
    """(B, 3, H, W) float32 unit normals, NaN in all three planes where the pixel has none."""
    depth = np.asarray(depth, dtype=F32)
    xyz, valid = PC.map_ref(depth, k, conf, conf_min, z_min, z_max)
    assert np.array_equal(valid, PC.valid_ref(depth, conf, conf_min, z_min, z_max))
    B, H, W = depth.shape
    gate = not (F32(jump_rel) == 0 and F32(jump_abs) == 0)
    with np.errstate(all="ignore"):
        z = depth
        tol = F32(jump_abs) + (F32(jump_rel) * z).astype(F32)

        def usable(di, dj):
            vn = _shift(valid, di, dj, False)  # outside the image: not valid, whatever z_min is
            if not gate:
                return vn
            zn = _shift(z, di, dj, F32(0))
            return vn & (np.abs((zn - z).astype(F32)) <= tol)

        def tangent(lo, hi):
            ul, uh = usable(*lo), usable(*hi)
            p = np.where(uh[:, None], _shift(xyz, *hi, F32(0)), xyz)
            q = np.where(ul[:, None], _shift(xyz, *lo, F32(0)), xyz)
            return (p - q).astype(F32), ul | uh

        tu, has_u = tangent((0, -1), (0, 1))
        tv, has_v = tangent((-1, 0), (1, 0))
        ux, uy, uz = tu[:, 0], tu[:, 1], tu[:, 2]
        vx, vy, vz = tv[:, 0], tv[:, 1], tv[:, 2]
        cx = ((vy * uz).astype(F32) - (vz * uy).astype(F32)).astype(F32)
        cy = ((vz * ux).astype(F32) - (vx * uz).astype(F32)).astype(F32)
        cz = ((vx * uy).astype(F32) - (vy * ux).astype(F32)).astype(F32)
        d = (((cx * xyz[:, 0]).astype(F32) + (cy * xyz[:, 1]).astype(F32)).astype(F32)
             + (cz * xyz[:, 2]).astype(F32)).astype(F32)
        flip = d > 0
        cx, cy, cz = (np.where(flip, -c, c) for c in (cx, cy, cz))
        l = np.sqrt((((cx * cx).astype(F32) + (cy * cy).astype(F32)).astype(F32) + (cz * cz).astype(F32)).astype(F32))
        ok = valid & has_u & has_v & (l > 0) & (l < np.inf)
        n = np.stack([cx / l, cy / l, cz / l], axis=1).astype(F32)
    assert l.dtype == F32 and n.dtype == F32
    n[np.broadcast_to(~ok[:, None], n.shape)] = np.nan
    return n


def picture_ref(nmap, empty=(0, 0, 0)):
    """(B, H, W, 3) uint8: R = q(nx), G = q(-ny), B = q(-nz), `empty` where the map is NaN."""
    with np.errstate(invalid="ignore"):
        h = (nmap * F32(0.5)).astype(F32)
        u = np.stack([h[:, 0] + F32(0.5), F32(0.5) - h[:, 1], F32(0.5) - h[:, 2]], axis=-1).astype(F32)
        q = np.rint((u * F32(255.0)).astype(F32))
        q = np.where(q > 0, q, F32(0))
        q = np.where(q < 255, q, F32(255))
    img = q.astype(np.uint8)
    img[np.isnan(nmap[:, 0])] = np.asarray(empty, dtype=np.uint8)
    return img


def packed_ref(nmap, index):
    """(N, 3) float32: the map gathered at the pixel indices, (0, 0, 0) where it is NaN."""
    B, _, H, W = nmap.shape
    rows = nmap.transpose(0, 2, 3, 1).reshape(-1, 3)[np.asarray(index, dtype=np.int64)]
    return np.where(np.isnan(rows), F32(0), rows).astype(F32)


def angle(a, b):
    """Angle (rad, float64) between vectors along axis 1."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    cr = np.cross(a, b, axis=1)
    return np.arctan2(np.linalg.norm(cr, axis=1), (a * b).sum(1))


def _rays(k, B, H, W):
    k = np.broadcast_to(np.asarray(k, dtype=np.float64), (B, 3, 3))
    j = np.arange(W, dtype=np.float64).reshape(1, 1, W)
    i = np.arange(H, dtype=np.float64).reshape(1, H, 1)
    rx = (j - k[:, 0, 2].reshape(B, 1, 1)) / k[:, 0, 0].reshape(B, 1, 1)
    ry = (i - k[:, 1, 2].reshape(B, 1, 1)) / k[:, 1, 1].reshape(B, 1, 1)
    return np.broadcast_to(rx, (B, H, W)), np.broadcast_to(ry, (B, H, W))


K_SMOOTH = np.array([[420.0, 0.0, 130.25], [0.0, 410.0, 4.5], [0.0, 0.0, 1.0]], dtype=F32)


def plane(normal, d, k, B, H, W):
    """(depth (B, H, W) float32, unit normal towards the camera (3,) float64) of the plane n . P = d
    rendered through k: z = d / (n . ray)."""
    n = np.asarray(normal, dtype=np.float64)
    d = d / np.linalg.norm(n)  # the same plane with a unit normal
    n = n / np.linalg.norm(n)
    rx, ry = _rays(k, B, H, W)
    z = d / (n[0] * rx + n[1] * ry + n[2])
    return z.astype(F32), (-n if d > 0 else n)


def plane_cases(H=9, W=261):
    """Three tilts whose depth spans 2 m .. 80 m along the middle row of the K_SMOOTH image (up to 86 m in
    the corners of the two that also tilt vertically): [(depth, normal)], B = 1."""
    rx, _ = _rays(K_SMOOTH, 1, H, W)
    r0, r1 = rx.min(), rx.max()
    out = []
    for ny, sign in ((0.0, 1.0), (0.3, 1.0), (-0.2, -1.0)):
        # n = (a, ny, 1): d / (a r0 + 1) and d / (a r1 + 1) are 2 and 80 (swapped for the other sign)
        lo, hi = (2.0, 80.0) if sign > 0 else (80.0, 2.0)
        a = (hi - lo) / (lo * r0 - hi * r1)  # lo (a r0 + 1) = hi (a r1 + 1)
        d = lo * (a * r0 + 1.0)
        out.append(plane((a, ny, 1.0), d, K_SMOOTH, 1, H, W))
    return out


def sphere_cap(centre, radius, k, B, H, W):
    """(depth (B, H, W) float32, 0 where the ray misses; analytic normals (B, 3, H, W) float64 towards
    the camera) of the near side of a sphere."""
    c = np.asarray(centre, dtype=np.float64)
    rx, ry = _rays(k, B, H, W)
    r = np.stack([rx, ry, np.ones_like(rx)], axis=1)
    rr = (r * r).sum(1)
    rc = (r * c.reshape(1, 3, 1, 1)).sum(1)
    disc = rc * rc - rr * (c @ c - radius * radius)
    hit = disc > 0
    t = np.where(hit, (rc - np.sqrt(np.where(hit, disc, 0.0))) / rr, 0.0)
    n = (t[:, None] * r - c.reshape(1, 3, 1, 1)) / radius
    return t.astype(F32), n
