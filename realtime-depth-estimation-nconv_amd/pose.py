"""The relative camera pose between the current frame and a neighbouring one, from the current frame's sparse
depth and the two images, on the device: the `m` that warp.view_warp, warp.photometric_loss,
warp.photometric_ssim_loss and the smoothness-regularised training step take as an input.

The recipes those losses come from (Ma, Cavalheiro, Karaman, ICRA 2019) get the pose of a training pair by
feature matching and PnP on the host. What a batch already holds fits direct image alignment instead (Kerl,
Sturm, Cremers, ICRA 2013; LSD-SLAM's tracker): the sparse depth of the target frame gives 3-D points, and the
pose is the one that minimises the intensity difference between the target frame at those pixels and the source
frame at their projections, by damped Gauss-Newton on SE(3), coarse to fine.

  pose_step        one Gauss-Newton iteration (nconv_pose_normal_eq + nconv_pose_update: two launches)
  estimate_pose    `levels` pyramid levels of `iters` iterations each, the pose of a level starting the next
  PoseEstimator    the same for fixed sizes with workspace, histories and outputs kept (hipGraph capture)
  EstimatePose     the DevicePrefetcher stage: batch["pose"], batch["m"] from batch["rgb_near"]
  pool_sparse      the half-resolution level of a sparse plane: the nearest valid sample of each 2 x 2 cell
  pose_projection  K_src . [R | t] in double in the kernels' order, rounded once (what nconv_pose_update writes)

The rule (include/nconv.h, nconv_pose_*): a pixel is a sample iff z > z_min && z <= z_max, its mask is not 0 and
its projection by the current pose lies inside the source; u, v, the taps, s, dIu and dIv are view_warp's bit for
bit; r = s - tgt, J = dIu Ju + dIv Jv for the left perturbation dP' = nu + omega x P', the Huber weight
w = |r| <= huber ? 1 : huber / |r| (0: least squares); per image sum w J^T J, sum w J r, sum w r^2 and the count,
fp32 over fixed 16 x 64 tiles, the tiles in double in a fixed order, no atomics. The update, in double: A = H +
damping diag(H), a square-root-free Cholesky solve of A delta = -b, the Cayley retraction R <- dR R,
t <- dR t + nu with dR = I + (2 / (1 + a.a)) ([a]x + [a]x^2), a = omega / 2 -- only + - x /, so the result is the
same bits on every run and a numpy restatement reproduces it. The pose state is double, in the workspace.

The pyramid is built per call with torch ops: the frames by F.avg_pool2d(., 2), the intrinsics by
warp.halve_intrinsics, the sparse plane by pool_sparse, which MOVES A SAMPLE BY UP TO HALF A COARSE PIXEL (it
keeps its depth but sits at its cell's centre); that is why the last level is always the full resolution, and
only its m is returned. A level whose H or W is odd is refused.

Not offered: feature matching or PnP; RANSAC; a step-acceptance test (true Levenberg-Marquardt: the damping is
fixed, and a step that raises the cost is kept); joint refinement of the depth; more than one source per call;
affine brightness correction. huber's default (10, in units of 8-bit-valued frames) is a convention: nobody has
measured it on KITTI. Device tensors only: there is no PyTorch path.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _views, warp

PREFIX = "pose"
HUBER_DEFAULT = 10.0       # grey levels of 8-bit-valued frames; a convention, not measured on KITTI
MIN_POINTS_DEFAULT = 32
SUMS = 28                  # 21 of the upper triangle of sum w J^T J, 6 of sum w J r, sum w r^2
STATUS = {0: "ok", 1: "fewer than min_points samples", 2: "a pivot of the solve is not finite or <= 0",
          3: "the step is not finite"}


def pose_projection(k_src, state):
    """(B, 3, 4) fp32 m = K_src . [R | t] from k_src (3, 3) or (B, 3, 3) and the (B, 3, 4) float64 pose state:
    m[i][j] = (Ks[i][0] P[0][j] + Ks[i][1] P[1][j]) + Ks[i][2] P[2][j] in double by element-wise operations (no
    matrix product, whose order is the library's), rounded once: nconv_pose_update's m bit for bit."""
    ks = k_src.double()
    if ks.dim() == 2:
        ks = ks[None]
    p = state.double()
    m = (ks[:, :, 0:1] * p[:, 0:1, :] + ks[:, :, 1:2] * p[:, 1:2, :]) + ks[:, :, 2:3] * p[:, 2:3, :]
    return m.float()


def pool_sparse(depth, mask=None, z_min=1e-3, z_max=None):
    """The half-resolution level of a sparse plane (B, 1, H, W), H and W even: per 2 x 2 cell the nearest valid
    sample (the minimum over the cell's pixels with z > z_min && z <= z_max and a nonzero mask; NaN is not
    valid), 0 where the cell has none. The sample keeps its depth but moves to the cell's centre: by up to half
    a coarse pixel."""
    z = depth
    zmax = torch.finfo(torch.float32).max if z_max is None else float(z_max)
    ok = (z > float(z_min)) & (z <= zmax)
    if mask is not None:
        mk = mask if mask.dim() == 4 else mask[:, None]
        ok = ok & (mk != 0)
    inf = torch.full_like(z, float("inf"))
    near = -F.max_pool2d(-torch.where(ok, z, inf), 2)
    return torch.where(torch.isfinite(near), near, torch.zeros_like(near))


def pyramid(depth, k, tgt, src, k_src, levels, mask=None, z_min=1e-3, z_max=None):
    """The levels as a list of dicts (depth, k, tgt, src, k_src, mask), index 0 the full resolution (the
    operands as given), index l the 2^l-fold reduction: frames by F.avg_pool2d(., 2), intrinsics by
    warp.halve_intrinsics, the sparse plane by pool_sparse (the mask is folded into it at the first reduction).
    Pure torch ops: works on CPU tensors as well."""
    levels = int(levels)
    if levels < 1:
        raise ValueError(f"{PREFIX}: levels = {levels} must be at least 1")
    out = [dict(depth=depth, k=k, tgt=tgt, src=src, k_src=k_src, mask=mask)]
    for l in range(1, levels):
        p = out[-1]
        for name in ("tgt", "src"):
            h, w = p[name].shape[-2:]
            if h % 2 or w % 2:
                raise ValueError(f"{PREFIX}: levels = {levels} halves {name} {l} times, but its size at level "
                                 f"{l - 1} is {h} x {w}, which is odd: choose fewer levels or crop to a multiple of "
                                 f"{2 ** (levels - 1)}")
        out.append(dict(depth=pool_sparse(p["depth"], p["mask"], z_min, z_max),
                        k=warp.halve_intrinsics(p["k"]), tgt=F.avg_pool2d(p["tgt"], 2), src=F.avg_pool2d(p["src"], 2),
                        k_src=warp.halve_intrinsics(p["k_src"]), mask=None))
    return out


def workspace_bytes(B, H, W):
    """Bytes of the workspace (nconv_pose_workspace_bytes): the float64 pose state (B, 3, 4) first, then the
    (B, 28) float64 sums of the last update, then the tiles' partial sums."""
    from . import _lib
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31)")
    return _lib.lib().nconv_pose_workspace_bytes(B, H, W)


def _options(huber, damping, min_points):
    for name, v in (("huber", huber), ("damping", damping), ("min_points", min_points)):
        if torch.is_tensor(v):
            raise TypeError(f"{PREFIX}: {name} must be a Python number (a constant of the call, and of a captured "
                            "graph), not a tensor")
    huber, damping, min_points = float(huber), float(damping), int(min_points)
    if not huber >= 0.0:
        raise ValueError(f"{PREFIX}: huber = {huber} must be >= 0 (0: plain least squares)")
    if not damping >= 0.0:
        raise ValueError(f"{PREFIX}: damping = {damping} must be >= 0")
    if min_points < 6:
        raise ValueError(f"{PREFIX}: min_points = {min_points} must be at least 6 (the pose has six unknowns)")
    return huber, damping, min_points


def _initial(init, B, device):
    """The (B, 3, 4) float64 start: the identity, or init (3, 4), (4, 4), (B, 3, 4) or (B, 4, 4)."""
    if init is None:
        return torch.eye(3, 4, dtype=torch.float64, device=device).expand(B, 3, 4)
    _views.require_tensor(init, "init", (torch.float32, torch.float64), PREFIX)
    if init.dim() not in (2, 3) or tuple(init.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"{PREFIX}: the pose must be (3, 4), (4, 4) or a batch of them, got {tuple(init.shape)}")
    p = init[..., :3, :].double()
    p = p[None] if p.dim() == 2 else p
    if p.shape[0] not in (1, B):
        raise ValueError(f"{PREFIX}: the pose holds {p.shape[0]} transforms, the batch {B} images")
    if p.device != device:
        raise RuntimeError(f"{PREFIX}: the pose on {p.device}, depth on {device}")
    return p.expand(B, 3, 4)


class _Buffers:
    """What a run keeps on the device: the workspace (its head the float64 pose state and sums), the fp32 pose,
    one m per level, and per level the status and the cost / n histories of iters + 1 entries."""

    def __init__(self, B, H, W, levels, iters, device):
        self.B, self.levels, self.history = B, levels, iters + 1
        self.nbytes = workspace_bytes(B, H, W)
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.state = self.ws[:B * 96].view(torch.float64).view(B, 3, 4)
        self.sums = self.ws[B * 96:B * (96 + SUMS * 8)].view(torch.float64).view(B, SUMS)
        self.pose = torch.zeros(B, 3, 4, dtype=torch.float32, device=device)
        self.m = torch.zeros(levels, B, 3, 4, dtype=torch.float32, device=device)
        self.status = torch.zeros(levels, B, dtype=torch.int32, device=device)
        self.cost = torch.zeros(levels, B, self.history, dtype=torch.float32, device=device)
        self.n = torch.zeros(levels, B, self.history, dtype=torch.int32, device=device)

    def matches(self, B, H, W, levels, iters, device):
        return (self.B == B and self.levels == levels and self.history == iters + 1 and self.ws.device == device
                and self.nbytes == workspace_bytes(B, H, W))


def _k_matrix(x, what, B):
    _views.require_tensor(x, what, (torch.float32,), PREFIX)
    if tuple(x.shape) not in ((3, 3), (1, 3, 3), (B, 3, 3)) or not x.is_contiguous():
        raise ValueError(f"{PREFIX}: {what} must be a contiguous (3, 3), (1, 3, 3) or ({B}, 3, 3), got "
                         f"{tuple(x.shape)} of strides {x.stride()}")
    return 9 if x.dim() == 3 and x.shape[0] == B and B > 1 else 0


def _descriptor(lv, buf, level, huber, damping, min_points, z_min, z_max):
    """The NconvPoseAlign of one level: warp's checked descriptor of the shared fields, then the new ones."""
    from . import _lib
    w, (B, C, H, W), t, mask = warp._descriptor(lv["depth"], lv["k"], lv["src"], buf.m[level], lv["mask"], z_min,
                                                z_max, lv["tgt"])
    d = _lib.NconvPoseAlign()
    for f, _ in _lib.NconvViewWarp._fields_:
        setattr(d, f, getattr(w, f))
    k_src = lv["k_src"]
    d.k_src_image_stride = _k_matrix(k_src, "k_src", B)
    if k_src.device != lv["depth"].device:
        raise RuntimeError(f"{PREFIX}: k_src on {k_src.device}, depth on {lv['depth'].device}")
    d.tgt, d.tgt_image_stride, d.tgt_channel_stride, d.tgt_row_stride = lv["tgt"].data_ptr(), t[0], t[1], t[2]
    d.k_src = k_src.data_ptr()
    d.pose, d.status = buf.pose.data_ptr(), buf.status[level].data_ptr()
    d.cost, d.n_hist, d.history = buf.cost[level].data_ptr(), buf.n[level].data_ptr(), buf.history
    d.huber, d.damping, d.min_points = huber, damping, min_points
    return d, (lv, mask)     # the tensors the descriptor points into stay alive with it


def _run_level(lv, buf, level, iters, opts, z_min, z_max):
    """iters iterations at one level from buf.state, then the cost at the pose reached: 2 iters + 2 launches."""
    from . import _lib
    lib = _lib.lib()
    buf.m[level].copy_(pose_projection(lv["k_src"], buf.state))
    d, keep = _descriptor(lv, buf, level, *opts, z_min, z_max)
    st, ws = _lib.stream_handle(buf.ws.device), _lib.ptr(buf.ws)
    for it in range(iters + 1):
        _lib.check(lib.nconv_pose_normal_eq(ctypes.byref(d), ws, buf.nbytes, st), "nconv_pose_normal_eq")
        _lib.check(lib.nconv_pose_update(ctypes.byref(d), ws, buf.nbytes, it, int(it < iters), st),
                   "nconv_pose_update")
    del keep


def _plane(depth):
    _views.require_tensor(depth, "depth", (torch.float32,), PREFIX)
    if depth.dim() == 3:
        depth = depth[:, None]
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"{PREFIX}: depth must be (B, 1, H, W) or (B, H, W), got {tuple(depth.shape)}")
    _views.on_device(depth, "depth", PREFIX, "poses are estimated by libnconv")
    return depth


def _estimate(depth, k, tgt, src, k_src, init, levels, iters, opts, mask, z_min, z_max, buf):
    depth = _plane(depth)
    B, H, W = depth.shape[0], depth.shape[2], depth.shape[3]
    k_src = k if k_src is None else k_src
    iters = int(iters)
    if iters < 1:
        raise ValueError(f"{PREFIX}: iters = {iters} must be at least 1")
    for name, x in (("tgt", tgt), ("src", src)):
        _views.require_tensor(x, name, (torch.float32,), PREFIX)
        if x.dim() != 4:
            raise ValueError(f"{PREFIX}: {name} must be (B, C, h, w), got {tuple(x.shape)}")
    lvs = pyramid(depth, k, tgt, src, k_src, levels, mask, z_min, z_max)
    if buf is None:
        buf = _Buffers(B, H, W, len(lvs), iters, depth.device)
    elif not buf.matches(B, H, W, len(lvs), iters, depth.device):
        raise ValueError(f"{PREFIX}: the kept buffers were made for another batch, size, levels or iters")
    buf.state.copy_(_initial(init, B, depth.device))
    buf.pose.copy_(buf.state)
    for level in range(len(lvs) - 1, -1, -1):
        _run_level(lvs[level], buf, level, iters, opts, z_min, z_max)
    return buf


def pose_step(depth, k, tgt, src, k_src, pose, mask=None, huber=HUBER_DEFAULT, damping=1e-4,
              min_points=MIN_POINTS_DEFAULT, z_min=1e-3, z_max=None):
    """One Gauss-Newton iteration from `pose`: (pose (B, 3, 4) fp32, m (B, 3, 4) fp32, info). info: 'cost' (B)
    fp32, the cost sum w r^2 / (C max(n, 1)) AT THE GIVEN POSE; 'n' (B) int32 samples; 'status' (B) int32 (STATUS);
    'sums' (B, 28) float64: the upper triangle of sum w J^T J row-major, sum w J r, sum w r^2; 'state' the
    (B, 3, 4) float64 pose. depth: (B, 1, H, W) fp32 sparse plane, any view of unit-stride rows; k, k_src: (3, 3)
    or (B, 3, 3) fp32 (k_src None: k); tgt (B, C, H, W), src (B, C, Hs, Ws) fp32, C = 1 or 3; pose: (3, 4),
    (4, 4) or a batch, float32 or float64, target camera frame -> source camera frame; mask: optional bool / uint8
    (B, 1, H, W). Two launches; nothing is read back."""
    opts = _options(huber, damping, min_points)
    depth = _plane(depth)
    B, H, W = depth.shape[0], depth.shape[2], depth.shape[3]
    k_src = k if k_src is None else k_src
    buf = _Buffers(B, H, W, 1, 1, depth.device)
    buf.state.copy_(_initial(pose, B, depth.device))
    buf.pose.copy_(buf.state)
    from . import _lib
    lib = _lib.lib()
    lv = dict(depth=depth, k=k, tgt=tgt, src=src, k_src=k_src, mask=mask)
    buf.m[0].copy_(pose_projection(k_src, buf.state))
    d, keep = _descriptor(lv, buf, 0, *opts, z_min, z_max)
    st, ws = _lib.stream_handle(depth.device), _lib.ptr(buf.ws)
    _lib.check(lib.nconv_pose_normal_eq(ctypes.byref(d), ws, buf.nbytes, st), "nconv_pose_normal_eq")
    _lib.check(lib.nconv_pose_update(ctypes.byref(d), ws, buf.nbytes, 0, 1, st), "nconv_pose_update")
    del keep
    info = {"cost": buf.cost[0, :, 0], "n": buf.n[0, :, 0], "status": buf.status[0], "sums": buf.sums,
            "state": buf.state}
    return buf.pose, buf.m[0], info


def _info(buf):
    return {"cost": buf.cost, "n": buf.n, "status": buf.status, "state": buf.state}


def estimate_pose(depth, k, tgt, src, k_src=None, init=None, levels=3, iters=8, huber=HUBER_DEFAULT, damping=1e-4,
                  min_points=MIN_POINTS_DEFAULT, mask=None, z_min=1e-3, z_max=None, return_info=False):
    """(pose, m): the (B, 3, 4) fp32 rigid transform [R | t] from the target camera's frame to the source
    camera's, and m = K_src . [R | t] at the full resolution, what view_warp and the photometric losses take; with
    return_info (pose, m, info), info's 'cost' and 'n' (levels, B, iters + 1) the histories per level (index 0 the
    full resolution; entry it the cost before iteration it, the last one the cost at the level's final pose),
    'status' (levels, B) int32 of each level's last iteration (STATUS; nonzero: that image's pose was left as it
    was) and 'state' the float64 pose: device tensors, nothing is read back. Operands as pose_step's; init None:
    the identity. The levels run coarse to fine, each from the pose of the one before; levels = 1 is the full
    resolution alone. 2 (iters + 1) launches per level plus the pyramid's torch ops."""
    opts = _options(huber, damping, min_points)
    buf = _estimate(depth, k, tgt, src, k_src, init, levels, iters, opts, mask, z_min, z_max, None)
    return (buf.pose, buf.m[0], _info(buf)) if return_info else (buf.pose, buf.m[0])


class PoseEstimator:
    """estimate_pose for fixed sizes with the workspace, the histories and the outputs kept between calls, so
    that a call can be captured with torch.cuda.graph and replayed on operands refilled in place:
    est(depth, k, tgt, src, k_src=None, init=None, mask=None) -> (pose, m), the kept tensors, overwritten by the
    next call; est.info holds the histories and the status. The pyramid's levels are torch ops: under capture
    their memory is the graph's own pool."""

    def __init__(self, size, B=1, C=3, levels=3, iters=8, huber=HUBER_DEFAULT, damping=1e-4,
                 min_points=MIN_POINTS_DEFAULT, z_min=1e-3, z_max=None, device=None):
        H, W = (int(v) for v in size)
        if min(H, W, int(B)) <= 0 or int(C) not in (1, 3) or int(levels) < 1 or int(iters) < 1:
            raise ValueError(f"{PREFIX}: sizes, levels and iters must be positive and C 1 or 3, got {size}, B={B}, "
                             f"C={C}, levels={levels}, iters={iters}")
        if H % 2 ** (int(levels) - 1) or W % 2 ** (int(levels) - 1):
            raise ValueError(f"{PREFIX}: levels = {levels} needs H and W divisible by {2 ** (int(levels) - 1)}, got "
                             f"{H} x {W}: a level whose H or W is odd cannot be halved")
        self.size, self.B, self.C, self.levels, self.iters = (H, W), int(B), int(C), int(levels), int(iters)
        self.opts = _options(huber, damping, min_points)
        self.z_min, self.z_max = z_min, z_max
        dev = torch.device("cuda" if device is None else device)
        self._buf = _Buffers(self.B, H, W, self.levels, self.iters, dev)
        self.info = _info(self._buf)

    def __call__(self, depth, k, tgt, src, k_src=None, init=None, mask=None):
        if torch.is_tensor(depth) and torch.is_tensor(tgt) and tgt.dim() == 4:
            got = (depth.shape[0], tgt.shape[1], tuple(depth.shape[-2:]))
            if got != (self.B, self.C, self.size):
                raise ValueError(f"{PREFIX}: PoseEstimator was built for B={self.B}, C={self.C}, {self.size}; got "
                                 f"B={got[0]}, C={got[1]}, {got[2]}")
        buf = _estimate(depth, k, tgt, src, k_src, init, self.levels, self.iters, self.opts, mask, self.z_min,
                        self.z_max, self._buf)
        return buf.pose, buf.m[0]


class EstimatePose:
    """A batch-dict stage for data.DevicePrefetcher(..., ingest=EstimatePose(chain=Ingest())): chain is called on
    the batch first, so that batch["rgb"] and batch["depth"] are fp32; where the batch carries a neighbouring
    frame batch[near_key] ((B, 3, h, w) fp32, or uint8 (B, h, w, 3), which is ingested as "rgb" was), it gains
    batch["pose"] and batch[out_key], estimate_pose's pose and m with batch["k"] as both cameras, on the stream
    the stage is called on. A batch without near_key is passed through untouched. options: estimate_pose's
    levels, iters, huber, damping, min_points, z_min, z_max. Which file is the neighbouring frame is the
    dataset's business: the loaders of data.py do not hand one out."""

    def __init__(self, chain=None, near_key="rgb_near", out_key="m", **options):
        allowed = ("levels", "iters", "huber", "damping", "min_points", "z_min", "z_max")
        for name in options:
            if name not in allowed:
                raise TypeError(f"{PREFIX}: EstimatePose has no option {name!r} (it has {', '.join(allowed)})")
        self.chain, self.near_key, self.out_key, self.options = chain, near_key, out_key, options

    def __call__(self, batch):
        if self.chain is not None:
            batch = self.chain(batch)
        near = batch.get(self.near_key)
        if near is None:
            return batch
        batch = dict(batch)
        if near.dtype == torch.uint8:
            from .frames import ingest
            near = ingest(rgb=near, reverse_rgb=getattr(self.chain, "reverse_rgb", True))["rgb"]
            batch[self.near_key] = near
        batch["pose"], batch[self.out_key] = estimate_pose(batch["depth"], batch["k"], batch["rgb"], near,
                                                           **self.options)
        return batch
