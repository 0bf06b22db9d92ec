"""The rule of include/nconv.h's nconv_pose_* restated in numpy, and the scenes of the pose tests
(test_pose_cpu.py, test_gpu_pose.py):

  terms_fp32      nconv_pose_normal_eq per pixel: the 28 float32 terms and the validity, every operation an
                  explicit float32 step -- what the kernel must reproduce bit for bit
  tile_partials   the 16 x 64 tiles' float32 partial sums in wave_ops.h's order (a thread's rows from +0)
  image_sums      the tiles of an image combined in double (reduce_tree.image_sum's order)
  update          nconv_pose_update in Python floats (IEEE double, no contraction): damping, the square-root-free
                  Cholesky, the status, the Cayley retraction, the fp32 pose and m
  align           the whole estimate: levels x (iters x (normal_eq + update) + the final cost)
  residual64 / jacobian64   the same residual and Jacobian in float64 (the Jacobian's own check)
  scene           the analytic scene of the convergence tests
  pool_loop       the 2 x 2 nearest-valid pool as a loop
"""
import json
import os

import numpy as np

f32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)
TH, TW, K = 16, 64, 28
BOUND_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_bound.json")


def _batched(x, B, shape, dtype=f32):
    x = np.asarray(x, dtype=dtype)
    return np.broadcast_to(x, (B, *shape)) if x.ndim == 2 else x


# ------------------------------------------------------------------------------------------------
# nconv_pose_normal_eq
# ------------------------------------------------------------------------------------------------
def terms_fp32(depth, k, tgt, src, k_src, m, pose, mask=None, huber=0.0, z_min=1e-3, z_max=0.0):
    """(terms (B, 28, H, W) float32, valid (B, H, W) bool, aux): depth (B, H, W), k and k_src (3, 3) or (B, 3, 3),
    tgt (B, C, H, W), src (B, C, Hs, Ws), m and pose (B, 3, 4) float32. aux: u, v, s, dIu, dIv."""
    z = np.asarray(depth, dtype=f32)
    src, tgt = np.asarray(src, dtype=f32), np.asarray(tgt, dtype=f32)
    B, H, W = z.shape
    C, Hs, Ws = src.shape[1:]
    k, ks = _batched(k, B, (3, 3)), _batched(k_src, B, (3, 3))
    m, p = _batched(m, B, (3, 4)), _batched(pose, B, (3, 4))
    col = lambda a: np.asarray(a, dtype=f32)[:, None, None]  # noqa: E731
    fx, fy, cx, cy = col(k[:, 0, 0]), col(k[:, 1, 1]), col(k[:, 0, 2]), col(k[:, 1, 2])
    fxs, fys = col(ks[:, 0, 0]), col(ks[:, 1, 1])
    M = [[col(m[:, r, q]) for q in range(4)] for r in range(3)]
    P = [[col(p[:, r, q]) for q in range(4)] for r in range(3)]
    jj = np.arange(W, dtype=f32)[None, None, :]
    ii = np.arange(H, dtype=f32)[None, :, None]
    one, hub = f32(1.0), f32(huber)
    with np.errstate(all="ignore"):
        tx, ty = jj - cx, ii - cy
        x, y = (tx * z) / fx, (ty * z) / fy
        zmax = f32(FLT_MAX) if z_max == 0.0 else f32(z_max)
        pvalid = (z > f32(z_min)) & (z <= zmax)

        def dot(r):
            return ((r[0] * x + r[1] * y) + r[2] * z) + r[3]

        a, bb, c = dot(M[0]), dot(M[1]), dot(M[2])
        u, v = a / c, bb / c
        valid = pvalid & (c > 0) & (u >= 0) & (u <= f32(Ws - 1)) & (v >= 0) & (v <= f32(Hs - 1))
        if mask is not None:
            valid = valid & (np.asarray(mask) != 0)
        us, vs = np.where(valid, u, f32(0)), np.where(valid, v, f32(0))
        fu, fv = np.floor(us), np.floor(vs)
        j0, i0 = fu.astype(np.int64), fv.astype(np.int64)
        j1, i1 = np.minimum(j0 + 1, Ws - 1), np.minimum(i0 + 1, Hs - 1)
        wu, wv = us - fu, vs - fv
        w0u, w0v = one - wu, one - wv
        # an invalid pixel's depth reads 0 in the kernel; its terms are discarded either way
        Xp, Yp, Zp = dot(P[0]), dot(P[1]), dot(P[2])
        xn, yn, iz = Xp / Zp, Yp / Zp, one / Zp
        xx, yy, xy = xn * xn, yn * yn, xn * yn
        Ju = {0: fxs * iz, 2: -(fxs * (xn * iz)), 3: -(fxs * xy), 4: fxs * (one + xx), 5: -(fxs * yn)}
        Jv = {1: fys * iz, 2: -(fys * (yn * iz)), 3: -(fys * (one + yy)), 4: fys * xy, 5: fys * xn}
        bi = np.arange(B)[:, None, None]
        per, S, DU, DV = [], [], [], []
        for ch in range(C):
            q = src[:, ch]
            a00, a01, a10, a11 = q[bi, i0, j0], q[bi, i0, j1], q[bi, i1, j0], q[bi, i1, j1]
            top = w0u * a00 + wu * a01
            bot = w0u * a10 + wu * a11
            s = w0v * top + wv * bot
            dIu = w0v * (a01 - a00) + wv * (a11 - a10)
            dIv = bot - top
            res = s - tgt[:, ch]
            J = [dIu * Ju[0], dIv * Jv[1]] + [dIu * Ju[n] + dIv * Jv[n] for n in range(2, 6)]
            ar = np.abs(res)
            w = np.ones_like(res) if huber == 0.0 else np.where(ar <= hub, one, hub / ar).astype(f32)
            wj = [w * J[n] for n in range(6)]
            t = [wj[n] * J[l] for n in range(6) for l in range(n, 6)]
            t += [wj[n] * res for n in range(6)]
            t.append((w * res) * res)
            per.append(t)
            S.append(s), DU.append(dIu), DV.append(dIv)
        terms = np.zeros((B, K, H, W), dtype=f32)
        for n in range(K):
            t = per[0][n] if C == 1 else (per[0][n] + per[1][n]) + per[2][n]
            assert t.dtype == f32
            terms[:, n] = np.where(valid, t, f32(0))
    return terms, valid, {"u": u, "v": v, "s": S, "dIu": DU, "dIv": DV}


def _butterfly(v):
    lane = np.arange(64)
    for msk in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ msk]
    return v


def tile_partials(terms, valid):
    """(part (B, tiles, 28) float32, cnt (B, tiles) int): thread (wave w, lane) adds the rows w, w + 4, w + 8,
    w + 12 of its column to +0 in that order, wave_sum, then ((w0 + w1) + w2) + w3; tiles row-major."""
    B, _, H, W = terms.shape
    nth, ntw = -(-H // TH), -(-W // TW)
    pad = np.zeros((B, K + 1, nth * TH, ntw * TW), dtype=f32)
    pad[:, :K, :H, :W] = terms
    pad[:, K, :H, :W] = valid
    t = pad.reshape(B, K + 1, nth, 4, 4, ntw, 64)          # row = 16 tile + 4 r + w
    acc = np.zeros((B, K + 1, nth, 4, ntw, 64), dtype=f32)
    for r in range(4):
        acc = acc + t[:, :, :, r]
    w = _butterfly(acc)[..., 0]                            # (B, K + 1, nth, 4 waves, ntw)
    part = ((w[:, :, :, 0] + w[:, :, :, 1]) + w[:, :, :, 2]) + w[:, :, :, 3]
    assert part.dtype == f32
    part = part.reshape(B, K + 1, nth * ntw).transpose(0, 2, 1)
    return np.ascontiguousarray(part[:, :, :K]), part[:, :, K].astype(np.int64)   # counts <= 1024: exact in fp32


def image_sums(part):
    """(B, tiles, 28) float32 -> (B, 28) float64: lane l adds the tiles l, l + 64, .. in order, then wave_sum."""
    B, tiles, _ = part.shape
    lanes = np.zeros((B, K, 64), dtype=np.float64)
    for t in range(tiles):
        lanes[:, :, t % 64] += part[:, t, :].astype(np.float64)
    return _butterfly(lanes)[..., 0]


# ------------------------------------------------------------------------------------------------
# nconv_pose_update
# ------------------------------------------------------------------------------------------------
def cayley(omega):
    """dR (3 x 3 nested lists of Python floats) of the rule's Cayley retraction."""
    a0, a1, a2 = (float(w) / 2.0 for w in omega)
    q00, q11, q22 = a0 * a0, a1 * a1, a2 * a2
    q01, q02, q12 = a0 * a1, a0 * a2, a1 * a2
    f = 2.0 / (1.0 + ((q00 + q11) + q22))
    return [[1.0 + f * (-(q11 + q22)), f * (-a2 + q01), f * (a1 + q02)],
            [f * (a2 + q01), 1.0 + f * (-(q00 + q22)), f * (-a0 + q12)],
            [f * (-a1 + q02), f * (a0 + q12), 1.0 + f * (-(q00 + q11))]]


def retract(state, delta):
    """[R | t] <- dR [R | t], t += nu, on a 3 x 4 nested list of Python floats."""
    dR = cayley(delta[3:6])
    N = [[(dR[i][0] * state[0][j] + dR[i][1] * state[1][j]) + dR[i][2] * state[2][j] for j in range(4)]
         for i in range(3)]
    for i in range(3):
        N[i][3] = N[i][3] + float(delta[i])
    return N


def solve(S, n, damping, min_points):
    """(delta (6 Python floats), status) from the 28 sums of one image."""
    S = [float(v) for v in S]
    A = [[0.0] * 6 for _ in range(6)]
    o = 0
    for r in range(6):
        for l in range(r, 6):
            A[r][l] = A[l][r] = S[o]
            o += 1
    damping = float(f32(damping))
    g = [0.0] * 6
    for r in range(6):
        A[r][r] = A[r][r] + damping * A[r][r]
        g[r] = -S[21 + r]
    if n < min_points:
        return [0.0] * 6, 1
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    with np.errstate(all="ignore"):
        for j in range(6):
            vv = [0.0] * 6
            d = A[j][j]
            for r in range(j):
                vv[r] = L[j][r] * D[r]
                d = d - L[j][r] * vv[r]
            if not d > 0.0 or not d <= DBL_MAX:
                return [0.0] * 6, 2
            D[j] = d
            for i in range(j + 1, 6):
                e = A[i][j]
                for r in range(j):
                    e = e - L[i][r] * vv[r]
                L[i][j] = e / d
        y = [0.0] * 6
        for i in range(6):
            e = g[i]
            for r in range(i):
                e = e - L[i][r] * y[r]
            y[i] = e
        delta = [0.0] * 6
        for i in range(5, -1, -1):
            e = y[i] / D[i]
            for r in range(i + 1, 6):
                e = e - L[r][i] * delta[r]
            delta[i] = e
    if any(not abs(v) <= DBL_MAX for v in delta):
        return [0.0] * 6, 3
    return delta, 0


def project(k_src, state):
    """(3, 4) float32 m = K_src [R | t] in double in the rule's order, rounded once."""
    ks = np.asarray(k_src, dtype=np.float64)
    return np.array([[(float(ks[i, 0]) * state[0][j] + float(ks[i, 1]) * state[1][j]) + float(ks[i, 2]) * state[2][j]
                      for j in range(4)] for i in range(3)], dtype=np.float64).astype(f32)


def update(sums, n, state, k_src, C, damping, min_points):
    """One image: (state', pose fp32 (3, 4), m fp32 (3, 4), status, cost fp32)."""
    cost = f32(float(sums[27]) / (float(C) * float(max(int(n), 1))))
    delta, status = solve(sums, int(n), damping, min_points)
    if status == 0:
        state = retract(state, delta)
    return state, np.array(state, dtype=np.float64).astype(f32), project(k_src, state), status, cost


def normal_eq(lv, m, pose, huber, z_min, z_max):
    terms, valid, _ = terms_fp32(lv["depth"], lv["k"], lv["tgt"], lv["src"], lv["k_src"], m, pose, lv.get("mask"),
                                 huber, z_min, z_max)
    part, cnt = tile_partials(terms, valid)
    return image_sums(part), cnt.sum(axis=1)


def align(levels, init=None, iters=8, huber=0.0, damping=1e-4, min_points=32, z_min=1e-3, z_max=0.0, trace=None):
    """The estimate over `levels` (a list of dicts depth (B, H, W), k, tgt, src, k_src, mask; index 0 the full
    resolution, run last). Returns a dict: pose, m (B, 3, 4) float32 of level 0, state (B nested lists), cost, n
    (L, B, iters + 1), status (L, B), sums (B, 28) of the last normal_eq. trace(level, it, states): called after
    every update."""
    B = np.asarray(levels[0]["depth"]).shape[0]
    C = np.asarray(levels[0]["tgt"]).shape[1]
    eye = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    if init is None:
        states = [[row[:] for row in eye] for _ in range(B)]
    else:
        init = _batched(np.asarray(init, dtype=np.float64), B, (3, 4), np.float64)
        states = [[[float(v) for v in row] for row in init[b]] for b in range(B)]
    Ln = len(levels)
    cost = np.zeros((Ln, B, iters + 1), dtype=f32)
    ns = np.zeros((Ln, B, iters + 1), dtype=np.int64)
    status = np.zeros((Ln, B), dtype=np.int64)
    pose = np.stack([np.array(s, dtype=np.float64).astype(f32) for s in states])
    m, sums = None, None
    for level in range(Ln - 1, -1, -1):
        lv = levels[level]
        ks = _batched(lv["k_src"], B, (3, 3))
        m = np.stack([project(ks[b], states[b]) for b in range(B)])
        for it in range(iters + 1):
            sums, n = normal_eq(lv, m, pose, huber, z_min, z_max)
            if it == iters:
                for b in range(B):
                    cost[level, b, it] = f32(float(sums[b, 27]) / (float(C) * float(max(int(n[b]), 1))))
                ns[level, :, it] = n
                break
            new = [update(sums[b], n[b], states[b], ks[b], C, damping, min_points) for b in range(B)]
            states = [r[0] for r in new]
            pose = np.stack([r[1] for r in new])
            m = np.stack([r[2] for r in new])
            status[level] = [r[3] for r in new]
            cost[level, :, it] = [r[4] for r in new]
            ns[level, :, it] = n
            if trace is not None:
                trace(level, it, states)
    return {"pose": pose, "m": m, "state": states, "cost": cost, "n": ns, "status": status, "sums": sums}


# ------------------------------------------------------------------------------------------------
# the float64 residual and Jacobian (one image, one channel), for the Jacobian's own check
# ------------------------------------------------------------------------------------------------
def residual64(image, z, k, k_src, tgt, state, pix):
    """r = I(project(R P + t)) - tgt at the pixels pix (N, 2) of (i, j), I a callable (u, v) -> intensity."""
    k, ks = np.asarray(k, dtype=np.float64), np.asarray(k_src, dtype=np.float64)
    S = np.asarray(state, dtype=np.float64)
    i, j = pix[:, 0].astype(np.float64), pix[:, 1].astype(np.float64)
    zz = np.asarray(z, dtype=np.float64)
    P = np.stack(((j - k[0, 2]) * zz / k[0, 0], (i - k[1, 2]) * zz / k[1, 1], zz))
    Q = S[:, :3] @ P + S[:, 3:4]
    u = ks[0, 0] * Q[0] / Q[2] + ks[0, 2]
    v = ks[1, 1] * Q[1] / Q[2] + ks[1, 2]
    return image(u, v) - tgt, (u, v, Q)


def jacobian64(grad, k_src, uvQ):
    """(N, 6): dr / d(nu, omega) of the left perturbation by the rule's formulas; grad: (u, v) -> (dI/du, dI/dv)."""
    ks = np.asarray(k_src, dtype=np.float64)
    u, v, Q = uvQ
    xn, yn, iz = Q[0] / Q[2], Q[1] / Q[2], 1.0 / Q[2]
    o = np.zeros_like(xn)
    Ju = ks[0, 0] * np.stack((iz, o, -xn * iz, -xn * yn, 1 + xn * xn, -yn))
    Jv = ks[1, 1] * np.stack((o, iz, -yn * iz, -(1 + yn * yn), xn * yn, xn))
    gu, gv = grad(u, v)
    return (gu * Ju + gv * Jv).T


# ------------------------------------------------------------------------------------------------
# the analytic scene
# ------------------------------------------------------------------------------------------------
def image(u, v):
    return (127.5 + 40 * np.sin(0.21 * u + 0.3) * np.cos(0.17 * v) + 30 * np.sin(0.11 * u - 0.13 * v + 1)
            + 20 * np.cos(0.05 * u + 0.29 * v))


def image_grad(u, v):
    gu = (40 * 0.21 * np.cos(0.21 * u + 0.3) * np.cos(0.17 * v) + 30 * 0.11 * np.cos(0.11 * u - 0.13 * v + 1)
          - 20 * 0.05 * np.sin(0.05 * u + 0.29 * v))
    gv = (-40 * 0.17 * np.sin(0.21 * u + 0.3) * np.sin(0.17 * v) - 30 * 0.13 * np.cos(0.11 * u - 0.13 * v + 1)
          - 20 * 0.29 * np.sin(0.05 * u + 0.29 * v))
    return gu, gv


def true_pose(t, omega):
    """(3, 4) float64 [R | t], R the Cayley rotation of omega."""
    return np.concatenate((np.array(cayley(omega)), np.asarray(t, dtype=np.float64)[:, None]), axis=1)


SMALL = ((0.05, -0.02, 0.15), (0.004, -0.006, 0.003))
LARGE = ((0.2, -0.1, 0.6), (0.01, -0.02, 0.01))


def scene(H=48, W=64, motion=SMALL, keep=0.10, seed=0, B=1, C=1, scale=1.0):
    """The issue's scene as a one-level dict of float32 arrays plus 'true' (3, 4) float64 and 'z_dense'
    (B, H, W): the source is I at integer pixels, the target I at the true projection of every pixel (by its
    dense depth z = 6 + 0.05 j + 0.08 i + 1.5 sin(0.3 j)), `keep` of the pixels kept as samples. scale: the
    pattern's coordinates are divided by it (a 96 x 128 version of the 48 x 64 scene: scale = 2). Channel ch of
    C > 1 is the image shifted by 5 ch grey levels."""
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = 6 + 0.05 * (jj / scale) + 0.08 * (ii / scale) + 1.5 * np.sin(0.3 * (jj / scale))
    k = np.array([[0.9 * W, 0, (W - 1) / 2], [0, 0.9 * W, (H - 1) / 2], [0, 0, 1]], dtype=np.float64)
    T = true_pose(*motion)
    pix = np.stack((ii.ravel(), jj.ravel()), axis=1)
    img = lambda u, v: image(u / scale, v / scale)  # noqa: E731
    _, (u, v, _) = residual64(img, z.ravel(), k, k, 0.0, T, pix)
    tgt1 = img(u, v).reshape(H, W)
    src1 = img(jj, ii)
    rng = np.random.RandomState(seed)
    depth = np.stack([np.where(rng.rand(H, W) < keep, z, 0.0) for _ in range(B)]).astype(f32)
    chans = lambda a: np.stack([a + 5.0 * ch for ch in range(C)])  # noqa: E731
    tgt = np.broadcast_to(chans(tgt1), (B, C, H, W)).astype(f32)
    src = np.broadcast_to(chans(src1), (B, C, H, W)).astype(f32)
    return {"depth": depth, "k": k.astype(f32), "k_src": k.astype(f32), "tgt": np.ascontiguousarray(tgt),
            "src": np.ascontiguousarray(src), "mask": None, "true": T, "z_dense": np.broadcast_to(z, (B, H, W)).astype(f32)}


def pose_error(state, true):
    """(|t - t_true|, the Frobenius norm of R R_true^T - I)."""
    S, T = np.asarray(state, dtype=np.float64), np.asarray(true, dtype=np.float64)
    return float(np.linalg.norm(S[:, 3] - T[:, 3])), float(np.linalg.norm(S[:, :3] @ T[:, :3].T - np.eye(3)))


def max_flow(sc, state=None):
    """The largest displacement in pixels between a sample's own pixel and its projection by the true pose
    (state: relative to the projection by that pose instead)."""
    z = sc["z_dense"][0].astype(np.float64)
    H, W = z.shape
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pix = np.stack((ii.ravel(), jj.ravel()), axis=1)
    _, (u, v, _) = residual64(image, z.ravel(), sc["k"], sc["k_src"], 0.0, sc["true"], pix)
    return float(np.sqrt((u - jj.ravel()) ** 2 + (v - ii.ravel()) ** 2).max())


def pool_loop(depth, mask=None, z_min=1e-3, z_max=0.0):
    """(B, H, W) -> (B, H / 2, W / 2) float32: per 2 x 2 cell the smallest valid sample, 0 where none."""
    z = np.asarray(depth, dtype=f32)
    B, H, W = z.shape
    zmax = f32(FLT_MAX) if z_max == 0.0 else f32(z_max)
    out = np.zeros((B, H // 2, W // 2), dtype=f32)
    for b in range(B):
        for i in range(H // 2):
            for j in range(W // 2):
                best = None
                for di in (0, 1):
                    for dj in (0, 1):
                        val = z[b, 2 * i + di, 2 * j + dj]
                        ok = val > f32(z_min) and val <= zmax
                        if mask is not None:
                            ok = ok and mask[b, 2 * i + di, 2 * j + dj] != 0
                        if ok and (best is None or val < best):
                            best = val
                out[b, i, j] = f32(0) if best is None else best
    return out


def load_bound():
    with open(BOUND_JSON) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------
# the cases and the bound taken from the restatement itself
# ------------------------------------------------------------------------------------------------
MARGIN = 2.0                                 # the bound is MARGIN x the restatement's own final error
OUTLIER_AMPLITUDE, OUTLIER_HUBER = 60.0, 0.5  # chosen on the restatement: 0.0070 m with the weight, 0.38 m without
# the pyramid case: the pattern at twice the frequency on 96 x 128 and a sideways motion of 28 pixels, from which
# one level ends 1.7 m off and three levels 1.2 mm off (the restatement, 8 iterations per level)
PYRAMID_SCENE = dict(H=96, W=128, motion=((1.3, 0.0, 0.0), (0.0, 0.0, 0.0)), scale=0.5)


def with_outliers(sc, share=0.10, amplitude=OUTLIER_AMPLITUDE, seed=7):
    """The scene with `share` of the target's pixels moved by +- amplitude grey levels."""
    sc = dict(sc)
    H, W = sc["tgt"].shape[-2:]
    rng = np.random.RandomState(seed)
    out = rng.rand(H, W) < share
    sign = np.where(rng.rand(H, W) < 0.5, -1.0, 1.0)
    sc["tgt"] = (sc["tgt"] + (amplitude * sign * out).astype(f32)).astype(f32)
    return sc


def photo_loss_cpu(sc, m):
    """warp.photometric_loss's value on the scene's dense depth, from warp_cases' fp32 rule, summed in double."""
    import warp_cases
    r = warp_cases.rule_fp32(sc["z_dense"], sc["k"], sc["src"], m, None, sc["tgt"])
    return float(r["terms"].astype(np.float64).sum() / float(r["den"]))


def measure_bound():
    table = {"margin": MARGIN}
    for name, motion in (("small", SMALL), ("large", LARGE)):
        sc = scene(motion=motion)
        r = align([sc], iters=8)
        t_err, r_err = pose_error(r["state"][0], sc["true"])
        eye = np.eye(3, 4)
        m_true = project(sc["k_src"], sc["true"].tolist())
        m_eye = project(sc["k_src"], eye.tolist())
        table[name] = {"t_err_ref": float(f"{t_err:.4g}"), "t_err_bound": float(f"{MARGIN * t_err:.4g}"),
                       "r_err_ref": float(f"{r_err:.4g}"), "r_err_bound": float(f"{MARGIN * r_err:.4g}"),
                       "t_err_init": float(f"{pose_error(eye, sc['true'])[0]:.4g}"),
                       "photo_true": float(f"{photo_loss_cpu(sc, m_true):.4g}"),
                       "photo_est": float(f"{photo_loss_cpu(sc, r['m'][0]):.4g}"),
                       "photo_identity": float(f"{photo_loss_cpu(sc, m_eye):.4g}")}
        table[name]["photo_factor"] = float(f"{MARGIN * table[name]['photo_est'] / table[name]['photo_true']:.4g}")
    return table


if __name__ == "__main__":
    import sys
    t = measure_bound()
    print(json.dumps(t, indent=1))
    if "--write" in sys.argv:
        with open(BOUND_JSON, "w") as fh:
            json.dump(t, fh, indent=1)
            fh.write("\n")
