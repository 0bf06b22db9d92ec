"""Cross-view depth consistency on the device: two views compared by their DEPTH, where warp.py compares colours.

A sequence run through DNET yields a depth map, a confidence and (pose.estimate_pose) a relative pose per frame.

  inverse_pose               [R | t] -> [R^T | -R^T t] (a torch op)
  depth_consistency          the geometric check of MVSNet's filter_depth / COLMAP's fusion over 1..4 neighbouring
                             views, and the fused depth (nconv_depth_consistency: one launch whatever S)
  DepthFuser                 the same with kept outputs and precomputed matrices (hipGraph capture)
  geometry_consistency_loss  SC-SfMLearner's geometry-consistency term (Bian et al., NeurIPS 2019), differentiable
                             in the prediction alone (nconv_geo_consistency_loss_fwd / _bwd: two launches forward,
                             one backward)
  GeometryConsistencyLoss    its nn.Module
  GeometryConsistency        ViewWarper's sibling: kept workspace, loss and gradient (hipGraph capture)

The rule (include/nconv.h, fp32, one rounding per operation): a target pixel at depth z is projected into source s
as view_warp does (same validity, same four taps, here taken on the source's depth plane); the taps must all be
depths themselves (> z_min, <= z_max: no blend across a hole or a NaN); their blend zs at the projected (u, v)
gives a point in the source camera, which m_back = K . [R | t]^-1 carries back to (u2, v2) at depth z2 in the
target view. Source s is consistent with the pixel iff the point came back within px_tol pixels of (j, i) and
|z2 - z| <= rel_tol z. fused is the mean of z and the consistent sources' z2 where at least min_views agree, else
0; count is their number. The loss is the mean over the pixels with a valid projection and valid taps of
|c - zs| / (c + zs), c the pixel's depth in the source camera (the third row of K_src must be 0 0 1, as the
loaders' is; not checked on the device); its per-pixel map `diff` in [0, 1) is the paper's occlusion / moving-
object weight.

Recipes: `fused, n = depth_consistency(...)`, then `backproject(fused, k, conf=conf, conf_min=0.5)` is a cloud that
is clean BEFORE the frames are merged (fused is 0, which backproject drops, where the views disagree);
`mask = (diff < 0.1).to(torch.uint8)` is the `mask=` of the photometric losses; in training,
`calculate_loss(pred, gt, True) + w * geo(pred, k, prev_depth, None, None, m=m)` is a GraphedTrainStep loss_fn
with m refilled in place.

Not offered: confidence-weighted averaging; per-image kept counts; a gradient to the source depth (a scatter:
a source that requires one is refused) or to the pose; a float weight map into the photometric losses (they take
a uint8 mask); more than four sources. The symmetric loss of the paper is two calls with the roles and the pose
swapped. The defaults px_tol=1, rel_tol=0.01, min_views=1 are MVSNet's convention; nobody has measured them on
KITTI with this network. Device tensors only: there is no PyTorch path.
"""
import ctypes

import torch

from . import _views
from . import warp as _warp

PREFIX = "consistency"
MAX_SOURCES = 4


def inverse_pose(pose):
    """[R | t] -> [R^T | -R^T t]: the rigid transform the other way round, (B, 3, 4) in pose's dtype. pose: (3, 4),
    (4, 4), (B, 3, 4) or (B, 4, 4) (the bottom row of a 4 x 4 is not read). A torch op, not a kernel: twelve
    numbers per image, computed in float64 and rounded once."""
    _views.require_tensor(pose, "pose", (torch.float32, torch.float64), PREFIX)
    if pose.dim() not in (2, 3) or tuple(pose.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"{PREFIX}: pose must be (3, 4), (4, 4) or a batch of them, got {tuple(pose.shape)}")
    p = pose[..., :3, :].double()
    if p.dim() == 2:
        p = p[None]
    rt = p[..., :3].transpose(-1, -2)
    return torch.cat((rt, -(rt @ p[..., 3:])), dim=-1).to(pose.dtype).contiguous()


def _plane4(x, what):
    """An (H, W), (1, H, W) or (B, 1, H, W) fp32 view as (B, 1, H, W), strides kept."""
    _views.require_tensor(x, what, (torch.float32,), PREFIX)
    if x.dim() == 2:
        return x[None, None]
    if x.dim() == 3 and x.shape[0] == 1:
        return x[None]
    if x.dim() == 4 and x.shape[1] == 1:
        return x
    raise ValueError(f"{PREFIX}: {what} must be (H, W), (1, H, W) or (B, 1, H, W), got {tuple(x.shape)}")


def _sequence(xs, what, S=None):
    if torch.is_tensor(xs):
        raise TypeError(f"{PREFIX}: {what} must be a sequence of 1..{MAX_SOURCES} tensors, not a tensor")
    xs = list(xs)
    if not 1 <= len(xs) <= MAX_SOURCES or (S is not None and len(xs) != S):
        want = f"1..{MAX_SOURCES}" if S is None else str(S)
        raise ValueError(f"{PREFIX}: {what} must hold {want} tensors (one per source), got {len(xs)}")
    return xs


def _tolerances(px_tol, rel_tol, min_views, S):
    if any(torch.is_tensor(v) for v in (px_tol, rel_tol, min_views)):
        raise TypeError(f"{PREFIX}: px_tol, rel_tol and min_views must be Python numbers (constants of the call, and "
                        "of a captured graph), not tensors")
    px_tol, rel_tol = float(px_tol), float(rel_tol)
    if not px_tol >= 0.0 or not rel_tol >= 0.0:
        raise ValueError(f"{PREFIX}: px_tol = {px_tol} and rel_tol = {rel_tol} must be >= 0")
    if int(min_views) != min_views or not 0 <= int(min_views) <= S:
        raise ValueError(f"{PREFIX}: min_views = {min_views} must be an integer in 0..{S} (the number of sources)")
    return px_tol, rel_tol, int(min_views)


def _check(depth, k, src_depths, k_srcs, ms, m_backs, px_tol, rel_tol, min_views, mask, z_min, z_max, want_views,
           want_error, out):
    from . import _lib
    src_depths = _sequence(src_depths, "src_depths")
    S = len(src_depths)
    k_srcs, ms, m_backs = _sequence(k_srcs, "k_srcs", S), _sequence(ms, "ms", S), _sequence(m_backs, "m_backs", S)
    px_tol, rel_tol, min_views = _tolerances(px_tol, rel_tol, min_views, S)
    depth = _plane4(depth, "depth").detach()
    descs, extras, keep = [], [], []
    for s in range(S):
        src = _plane4(src_depths[s], f"src_depths[{s}]")
        d, (B, _, H, W), _, mview = _warp._descriptor(depth, k, src, ms[s], mask, z_min, z_max)
        e = _lib.NconvConsistencySource()
        e.k_src_image_stride = _warp._matrix(k_srcs[s], f"k_srcs[{s}]", B, (3, 3))
        e.m_back_image_stride = _warp._matrix(m_backs[s], f"m_backs[{s}]", B, (3, 4))
        for name, x in ((f"k_srcs[{s}]", k_srcs[s]), (f"m_backs[{s}]", m_backs[s])):
            _views.on_device(x, name, PREFIX, "depth maps are compared by libnconv")
            if x.device != depth.device:
                raise RuntimeError(f"{PREFIX}: {name} on {x.device}, depth on {depth.device}")
        e.k_src, e.m_back = k_srcs[s].data_ptr(), m_backs[s].data_ptr()
        descs.append(d), extras.append(e), keep.append((src, mview))
    if B * S * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: (B, S, H, W) = {(B, S, H, W)} is too large (B * S * H * W < 2^31)")
    dev = depth.device
    u8, f32 = torch.uint8, torch.float32
    fused = _views.output(out, "fused", (B, 1, H, W), f32, dev, PREFIX, source="depth")
    count = _views.output(out, "count", (B, H, W), u8, dev, PREFIX, source="depth")
    views = _views.output(out, "views", (B, H, W), u8, dev, PREFIX, source="depth") if want_views else None
    reproj = _views.output(out, "reproj", (B, S, H, W), f32, dev, PREFIX, source="depth") if want_error else None
    reldiff = _views.output(out, "reldiff", (B, S, H, W), f32, dev, PREFIX, source="depth") if want_error else None
    rc = _lib.lib().nconv_depth_consistency(
        (_lib.NconvViewWarp * S)(*descs), (_lib.NconvConsistencySource * S)(*extras), S, px_tol, rel_tol, min_views,
        _lib.ptr(fused), _lib.ptr(count), _lib.ptr(views), _lib.ptr(reproj), _lib.ptr(reldiff),
        _lib.stream_handle(dev))
    _lib.check(rc, "nconv_depth_consistency")
    return (fused, count) + ((views,) if want_views else ()) + ((reproj, reldiff) if want_error else ())


def depth_consistency(depth, k, src_depths, k_srcs, poses, px_tol=1.0, rel_tol=0.01, min_views=1, mask=None,
                      z_min=1e-3, z_max=None, return_views=False, return_error=False):
    """The cross-view check and fusion of a depth map against S = 1..4 neighbouring depth maps: (fused (B, 1, H, W)
    fp32, count (B, H, W) uint8[, views][, reproj, reldiff]). fused: the mean of z and the consistent sources'
    carried-back depths where the pixel is valid and count >= min_views, else 0; count: the number of consistent
    sources; views (return_views): uint8, bit s set iff source s is consistent; reproj, reldiff (return_error):
    (B, S, H, W) fp32, the squared pixel distance of the round trip and |z2 - z| / z, +inf where the round trip is
    not defined. depth: (H, W), (1, H, W) or (B, 1, H, W) fp32, any view of unit-stride rows (DNET's cropped output);
    k: (3, 3) or (B, 3, 3), the target camera; src_depths, k_srcs, poses: sequences of S tensors, each source's
    depth (its own size), intrinsics and the pose that takes the target camera frame to the source's (as
    warp_projection's). m = warp_projection(k_src, pose) and m_back = warp_projection(k, inverse_pose(pose)) are
    formed here (torch ops; DepthFuser takes them precomputed). mask: optional bool / uint8 (B, 1, H, W) of the
    target. px_tol, rel_tol, min_views: Python numbers. Nothing here is differentiable. One launch."""
    src_depths = _sequence(src_depths, "src_depths")
    k_srcs, poses = _sequence(k_srcs, "k_srcs", len(src_depths)), _sequence(poses, "poses", len(src_depths))
    with torch.no_grad():
        ms = [_warp.warp_projection(ks, p) for ks, p in zip(k_srcs, poses)]
        m_backs = [_warp.warp_projection(k, inverse_pose(p)) for p in poses]
        return _check(depth, k, src_depths, k_srcs, ms, m_backs, px_tol, rel_tol, min_views, mask, z_min, z_max,
                      bool(return_views), bool(return_error), None)


class DepthFuser:
    """depth_consistency for fixed sizes with its outputs kept between calls and the matrices precomputed: no
    allocation after construction, so the call can be captured with torch.cuda.graph and replayed on operands
    refilled in place. fuser(depth, k, src_depths, k_srcs, ms, m_backs) -> the tuple depth_consistency returns;
    ms[s] = warp_projection(k_srcs[s], pose_s) and m_backs[s] = warp_projection(k, inverse_pose(pose_s)), (B, 3, 4)
    or (3, 4) fp32 buffers. The returned tensors are the kept ones, overwritten by the next call."""

    def __init__(self, size, src_size=None, S=2, B=1, device=None, px_tol=1.0, rel_tol=0.01, min_views=1, z_min=1e-3,
                 z_max=None):
        H, W = (int(v) for v in size)
        Hs, Ws = (H, W) if src_size is None else (int(v) for v in src_size)
        if min(H, W, Hs, Ws, int(B)) <= 0 or not 1 <= int(S) <= MAX_SOURCES:
            raise ValueError(f"{PREFIX}: sizes must be positive and S in 1..{MAX_SOURCES}, got {size}, {src_size}, "
                             f"S={S}, B={B}")
        self.size, self.src_size, self.S, self.B = (H, W), (Hs, Ws), int(S), int(B)
        self.px_tol, self.rel_tol, self.min_views = _tolerances(px_tol, rel_tol, min_views, self.S)
        self.z_min, self.z_max = z_min, z_max
        dev = torch.device("cuda" if device is None else device)
        f32 = dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self._out = {"fused": torch.empty(self.B, 1, H, W, **f32), "count": torch.empty(self.B, H, W, **u8),
                     "views": torch.empty(self.B, H, W, **u8), "reproj": torch.empty(self.B, self.S, H, W, **f32),
                     "reldiff": torch.empty(self.B, self.S, H, W, **f32)}

    def __call__(self, depth, k, src_depths, k_srcs, ms, m_backs, mask=None, return_views=False,
                 return_error=False):
        src_depths = _sequence(src_depths, "src_depths")
        if torch.is_tensor(depth) and all(torch.is_tensor(s) for s in src_depths):
            got = (_plane4(depth, "depth").shape[0], tuple(depth.shape[-2:]), len(src_depths),
                   {tuple(s.shape[-2:]) for s in src_depths})
            if got != (self.B, self.size, self.S, {self.src_size}):
                raise ValueError(f"{PREFIX}: DepthFuser was built for B={self.B}, {self.size} from S={self.S} sources "
                                 f"of {self.src_size}; got B={got[0]}, {got[1]} from S={got[2]} of {sorted(got[3])}")
        with torch.no_grad():
            return _check(depth, k, src_depths, k_srcs, ms, m_backs, self.px_tol, self.rel_tol, self.min_views, mask,
                          self.z_min, self.z_max, bool(return_views), bool(return_error), self._out)


def workspace_bytes(B, H, W):
    """Bytes of geometry_consistency_loss's workspace (nconv_geo_consistency_workspace_bytes); its first int32 is
    n_g, the number of counted pixels."""
    from . import _lib
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31)")
    return _lib.lib().nconv_geo_consistency_workspace_bytes(B, H, W)


class GeometryConsistencyLossFn(torch.autograd.Function):
    """geometry_consistency_loss's kernels (nconv_geo_consistency_loss_fwd / _bwd); the gradient reaches the
    prediction alone."""

    @staticmethod
    def forward(ctx, pred, k, src_depth, m, mask, z_min, z_max, want_diff, out):
        from . import _lib
        d, (B, _, H, W), _, mask = _warp._descriptor(pred, k, src_depth, m, mask, z_min, z_max)
        dev = pred.device
        nbytes = workspace_bytes(B, H, W)
        ws = _views.output(out, "workspace", (nbytes,), torch.uint8, dev, PREFIX, source="pred")
        loss = _views.output(out, "loss", (), torch.float32, dev, PREFIX, source="pred")
        diff = _views.output(out, "diff", (B, 1, H, W), torch.float32, dev, PREFIX, source="pred") if want_diff \
            else None
        rc = _lib.lib().nconv_geo_consistency_loss_fwd(ctypes.byref(d), _lib.ptr(loss), _lib.ptr(diff), _lib.ptr(ws),
                                                       nbytes, _lib.stream_handle(dev))
        _lib.check(rc, "nconv_geo_consistency_loss_fwd")
        ctx.z = (z_min, z_max)
        ctx.g_depth = None if out is None else out.get("g_depth")
        ctx.save_for_backward(pred, k, src_depth, m, mask, ws)
        n_g = ws[:4].view(torch.int32)[0]
        ctx.mark_non_differentiable(*(x for x in (n_g, diff) if x is not None))
        return loss, n_g, diff

    @staticmethod
    def backward(ctx, gloss, *_):
        from . import _lib
        pred, k, src_depth, m, mask, ws = ctx.saved_tensors
        d, (B, _, H, W), _, _ = _warp._descriptor(pred, k, src_depth, m, mask, *ctx.z)
        gloss = gloss.contiguous()
        g = ctx.g_depth if ctx.g_depth is not None else torch.empty((B, 1, H, W), dtype=torch.float32,
                                                                    device=pred.device)
        rc = _lib.lib().nconv_geo_consistency_loss_bwd(ctypes.byref(d), _lib.ptr(gloss), _lib.ptr(ws), ws.numel(),
                                                       _lib.ptr(g), _lib.stream_handle(pred.device))
        _lib.check(rc, "nconv_geo_consistency_loss_bwd")
        return g.view(pred.shape), None, None, None, None, None, None, None, None


def _geo_loss(pred, k, src_depth, m, mask, z_min, z_max, return_diff, return_count, out):
    loss, n_g, diff = GeometryConsistencyLossFn.apply(_plane4(pred, "pred"), k, _plane4(src_depth, "src_depth"), m,
                                                      mask, z_min, z_max, bool(return_diff), out)
    res = (loss,) + ((diff,) if return_diff else ()) + ((n_g,) if return_count else ())
    return res if len(res) > 1 else loss


def geometry_consistency_loss(pred, k, src_depth, k_src, pose, mask=None, z_min=1e-3, z_max=None, return_diff=False,
                              return_count=False, m=None):
    """SC-SfMLearner's geometry-consistency loss: the mean of diff = |c - zs| / (c + zs) over the n_g pixels of pred
    whose projection into the source view is valid (view_warp's rule) and whose four depth taps there are all
    valid; c is the pixel's depth in the source camera, zs the source's depth blended at its projection. A scalar
    on the device, followed, as asked for, by diff (return_diff: (B, 1, H, W) fp32, 0 where not counted) and n_g
    (return_count: an int32 view of the workspace, no host synchronisation). pred: (H, W), (1, H, W) or
    (B, 1, H, W) fp32, any view of unit-stride rows; k: the target camera; src_depth: the neighbouring view's depth,
    its own size, sparse planes included (a hole is no tap); k_src, pose: its camera and the transform from the
    target camera frame to it, m = warp_projection(k_src, pose) being formed here unless m is given (then k_src
    and pose are not read: a captured step refills m in place). The third row of k_src must be 0 0 1.
    Differentiable in pred alone: a src_depth, k or m that requires a gradient is refused (the gradient to the
    source depth would be a scatter). The paper's symmetric loss is two calls with the roles and the pose swapped.
    Two launches forward, one backward."""
    if m is None:
        with torch.no_grad():
            m = _warp.warp_projection(k_src, pose)
    return _geo_loss(pred, k, src_depth, m, mask, z_min, z_max, return_diff, return_count, None)


class GeometryConsistencyLoss(torch.nn.Module):
    """geometry_consistency_loss with its depth window held: loss(pred, k, src_depth, k_src, pose, mask=None, m=None).
    In a training step: calculate_loss(pred, gt, True) + w * geo(pred, k, prev_depth, None, None, m=m), with m
    refilled in place per batch (a GraphedTrainStep input)."""

    def __init__(self, z_min=1e-3, z_max=None):
        super().__init__()
        if not float(z_min) >= 0.0 or (z_max is not None and not float(z_max) >= float(z_min)):
            raise ValueError(f"{PREFIX}: need 0 <= z_min <= z_max, got z_min={z_min}, z_max={z_max}")
        self.z_min, self.z_max = float(z_min), None if z_max is None else float(z_max)

    def forward(self, pred, k, src_depth, k_src=None, pose=None, mask=None, m=None):
        return geometry_consistency_loss(pred, k, src_depth, k_src, pose, mask, self.z_min, self.z_max, m=m)


class GeometryConsistency:
    """geometry_consistency_loss for fixed sizes with its workspace, loss, diff and gradient kept between calls: no
    allocation after construction, so the loss and its backward can be captured with torch.cuda.graph and replayed
    on operands refilled in place (ViewWarper's sibling). geo(pred, k, src_depth, m) -> loss, or the tuple
    geometry_consistency_loss returns with return_diff / return_count; m = warp_projection(k_src, pose), a kept
    (B, 3, 4) or (3, 4) fp32 buffer. The returned tensors are the kept ones, overwritten by the next call."""

    def __init__(self, size, src_size=None, B=1, device=None, z_min=1e-3, z_max=None):
        H, W = (int(v) for v in size)
        Hs, Ws = (H, W) if src_size is None else (int(v) for v in src_size)
        if min(H, W, Hs, Ws, int(B)) <= 0:
            raise ValueError(f"{PREFIX}: sizes must be positive, got {size}, {src_size}, B={B}")
        self.size, self.src_size, self.B = (H, W), (Hs, Ws), int(B)
        self.z_min, self.z_max = z_min, z_max
        dev = torch.device("cuda" if device is None else device)
        f32 = dict(dtype=torch.float32, device=dev)
        self._out = {"workspace": torch.empty(workspace_bytes(self.B, H, W), dtype=torch.uint8, device=dev),
                     "loss": torch.empty((), **f32), "diff": torch.empty(self.B, 1, H, W, **f32),
                     "g_depth": torch.empty(self.B, 1, H, W, **f32)}

    def __call__(self, pred, k, src_depth, m, mask=None, return_diff=False, return_count=False):
        if torch.is_tensor(pred) and torch.is_tensor(src_depth):
            got = (_plane4(pred, "pred").shape[0], tuple(pred.shape[-2:]), tuple(src_depth.shape[-2:]))
            if got != (self.B, self.size, self.src_size):
                raise ValueError(f"{PREFIX}: GeometryConsistency was built for B={self.B}, {self.size} from "
                                 f"{self.src_size}; got B={got[0]}, {got[1]} from {got[2]}")
        return _geo_loss(pred, k, src_depth, m, mask, self.z_min, self.z_max, return_diff, return_count, self._out)
