"""Self-supervised view synthesis on the device: a neighbouring camera frame warped into the current view
by the predicted depth and a known relative pose, and the photometric (L1) loss on top of it.

The supervised losses (train.calculate_loss, train.confidence_loss) need a ground-truth plane, and KITTI's
ends at the LiDAR's upper scan line. The usual remedy (Ma, Cavalheiro, Karaman, ICRA 2019; the monodepth
family) is a photometric term: warp the neighbouring frame with the prediction, penalise the difference
to the current frame, and let the gradient flow into the depth.

  warp_projection     K_src . [R | t] as the (B, 3, 4) matrix the kernels take (lidar.projection_from_k's sibling)
  view_warp           src (B, C, Hs, Ws) -> warped (B, C, H, W), differentiable in the depth only
                      (nconv_view_warp_fwd / _bwd: one launch each)
  photometric_loss    mean over valid pixels and channels of |warped - tgt| with the warp fused in
                      (nconv_photo_loss_fwd / _bwd: two launches forward, one backward; warped never
                      reaches memory)
  photometric_ssim_loss  alpha / 2 (1 - SSIM) + (1 - alpha) L1, the loss the monodepth family trains with, over
                      3 x 3 windows of all-valid pixels, the warp fused in (nconv_photo_ssim_loss_fwd / _bwd:
                      two launches forward, one backward; neither warped nor any SSIM plane reaches memory)
  min_reprojection_loss  monodepth2's per-pixel minimum of that loss's error over 1..4 sources, with auto-masking,
                      an optional winner plane and per-pixel error map (nconv_photo_min_loss_fwd / _bwd: two
                      launches forward, one backward, whatever the number of sources)
  MinReprojectionLoss, MinReprojector  its nn.Module and its variant with kept buffers (hipGraph capture)
  PhotometricLoss     either single-source loss as an nn.Module (alpha = 0: the L1 path)
  ViewWarper          the same with outputs and workspace kept between calls (hipGraph capture)
  halve_intrinsics    k of a half-resolution pyramid level made by 2 x 2 average pooling
  halve_projection    m of that level

The rule (include/nconv.h, fp32, one rounding per operation): P = pointcloud.backproject's point of the
pixel at depth z; (a, b, c) = m . (P, 1) with lidar.project_points' dot; u = a / c, v = b / c; the pixel is
valid iff z > z_min, z <= z_max, c > 0, 0 <= u <= Ws - 1, 0 <= v <= Hs - 1 and its mask is not 0; a valid
pixel is the bilinear blend of the four source pixels around (v, u) (pixel centres at integer
coordinates, F.grid_sample's align_corners=True), an invalid one is 0 and has no gradient. The results
are the same bits on every run: each target pixel owns its four taps, so the depth's gradient is a gather.

The SSIM term (include/nconv.h, nconv_photo_ssim_loss_*): a pixel has a window iff it is not on the image's
one-pixel frame and all nine pixels of its 3 x 3 neighbourhood are valid -- not monodepth's
ReflectionPad2d(1), on purpose: a term counts where all its pixels count, as in smooth.py; the means, variances
and the covariance are monodepth's E[xy] - E[x] E[y] over the window, c1 = (0.01 R)^2, c2 = (0.03 R)^2 for the
data range R, and the term is clamp((1 - SSIM) / 2, 0, 1) averaged over windows and channels.

The minimum over several sources (include/nconv.h, nconv_photo_min_loss_*): per pixel the smallest of the
sources' errors alpha termw + (1 - alpha) term over the sources in which the pixel has a window, the lowest
index winning a tie; with auto-masking a pixel whose best unwarped source matches at least as well adds nothing
to the sum but stays in the mean over the pixels with a winner.

Not offered: a gradient with respect to the source image (a scatter) or to m (poses are inputs); for the SSIM
term reflection padding and windows other than 3 x 3; a built-in image pyramid (a level is F.avg_pool2d(., 2) of the frames and the depth with halve_intrinsics(k) and
halve_projection(m): dividing k by 2 is wrong by half a pixel). The pose itself is pose.estimate_pose's. Device
tensors only: there is no PyTorch path.
"""
import ctypes

import torch

from . import _views
from .lidar import projection_from_k

PREFIX = "warp"


def warp_projection(k_src, pose):
    """K_src . [R | t]: the (B, 3, 4) fp32 matrix `m` of view_warp / photometric_loss on k_src's device.
    k_src: (3, 3) or (B, 3, 3) intrinsics of the source camera. pose: (3, 4), (4, 4), (B, 3, 4) or
    (B, 4, 4), the rigid transform that takes a point of the target camera's frame to the source camera's
    (the bottom row of a 4 x 4 is not read). The product is taken in float64 and rounded once."""
    _views.require_tensor(k_src, "k_src", (torch.float32, torch.float64), PREFIX)
    _views.require_tensor(pose, "pose", (torch.float32, torch.float64), PREFIX)
    if pose.dim() not in (2, 3) or tuple(pose.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"{PREFIX}: pose must be (3, 4), (4, 4) or a batch of them, got {tuple(pose.shape)}")
    p = projection_from_k(k_src).double()                      # [K | 0], (3, 4) or (B, 3, 4)
    if pose.device != p.device:
        raise RuntimeError(f"{PREFIX}: pose on {pose.device}, k_src on {p.device}")
    rt = pose[..., :3, :].double()
    if p.dim() == 3 and rt.dim() == 3 and p.shape[0] != rt.shape[0]:
        raise ValueError(f"{PREFIX}: k_src holds {p.shape[0]} cameras, pose {rt.shape[0]} transforms")
    last = rt.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(rt.shape[:-2] + (1, 4))
    m = p @ torch.cat((rt, last), dim=-2)                      # [K | 0] . [R t; 0 1] = [K R | K t]
    return (m if m.dim() == 3 else m[None]).float().contiguous()


def _halved(x, what, shape):
    _views.require_tensor(x, what, (torch.float32, torch.float64), PREFIX)
    if x.dim() not in (2, 3) or tuple(x.shape[-2:]) != shape:
        raise ValueError(f"{PREFIX}: {what} must be {shape} or a batch of them, got {tuple(x.shape)}")
    return x.double().clone()


def halve_intrinsics(k):
    """The intrinsics of a half-resolution level made by 2 x 2 average pooling, whose pixel j' sits at the
    full-resolution coordinate 2 j' + 0.5 (pixel centres at integer coordinates, as view_warp fixes them):
    fx' = fx / 2, cx' = (cx - 0.5) / 2, likewise in y; plain k / 2 is wrong by half a pixel. k: (3, 3) or
    (B, 3, 3), float32 or float64; computed in float64 and rounded once to k's dtype."""
    h = _halved(k, "k", (3, 3))
    h[..., :2, :] = (h[..., :2, :] - 0.5 * h[..., 2:3, :]) / 2
    return h.to(k.dtype)


def halve_projection(m):
    """The projection K_src . [R | t] into the half-resolution level of the source frame (halve_intrinsics of
    K_src applied to m): rows 0 and 1 become (row - 0.5 row 2) / 2. m: (3, 4) or (B, 3, 4); computed in
    float64 and rounded once to m's dtype."""
    h = _halved(m, "m", (3, 4))
    h[..., :2, :] = (h[..., :2, :] - 0.5 * h[..., 2:3, :]) / 2
    return h.to(m.dtype)


def _image_view(x, what, B, C):
    """(image stride, channel stride, row stride) of a (B, C, h, w) fp32 view of unit-stride rows."""
    _views.require_tensor(x, what, (torch.float32,), PREFIX)
    if x.dim() != 4 or x.shape[0] != B or (C is not None and x.shape[1] != C):
        want = f"({B}, {'C' if C is None else C}, h, w)"
        raise ValueError(f"{PREFIX}: {what} must be {want}, got {tuple(x.shape)}")
    if x.shape[1] not in (1, 3):
        raise ValueError(f"{PREFIX}: {what} has {x.shape[1]} channels; C must be 1 or 3")
    if x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError(f"{PREFIX}: {what} of shape {tuple(x.shape)} is empty")
    if x.stride(3) != 1 and x.shape[3] > 1:
        raise ValueError(f"{PREFIX}: {what} of strides {x.stride()} has no unit-stride rows")
    return x.stride(0), x.stride(1), x.stride(2) if x.shape[2] > 1 else max(x.stride(2), x.shape[3])


def _matrix(x, what, B, shape):
    _views.require_tensor(x, what, (torch.float32,), PREFIX)
    if tuple(x.shape) not in (shape, (1, *shape), (B, *shape)):
        raise ValueError(f"{PREFIX}: {what} must be {shape}, {(1, *shape)} or {(B, *shape)}, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{PREFIX}: {what} of strides {x.stride()} is not contiguous")
    if x.requires_grad:
        raise ValueError(f"{PREFIX}: {what} requires a gradient, and only the depth gets one (poses and intrinsics "
                         f"are inputs): pass {what}.detach()")
    return shape[0] * shape[1] if x.dim() == 3 and x.shape[0] == B else 0


def _descriptor(depth, k, src, m, mask, z_min, z_max, tgt=None):
    """The checked operands as (NconvViewWarp, (B, C, H, W), tgt strides). Shapes, dtypes and gradients
    are checked before the devices, so that a wrong call says what is wrong with it wherever it runs."""
    from . import _lib
    _views.require_tensor(depth, "depth", (torch.float32,), PREFIX)
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"{PREFIX}: depth must be (B, 1, H, W), got {tuple(depth.shape)}")
    B, H, W, dbs, drs = _views.plane_view(depth, "depth", PREFIX)
    sbs, scs, srs = _image_view(src, "src", B, None)
    C, Hs, Ws = src.shape[1], src.shape[2], src.shape[3]
    if src.requires_grad:
        raise ValueError(f"{PREFIX}: src requires a gradient, and only the depth gets one: the gradient with respect "
                         "to the source image would scatter each target pixel's value over four source pixels "
                         "(atomics, run-to-run differences), which this deterministic gather does not offer; pass "
                         "src.detach()")
    kbs = _matrix(k, "k", B, (3, 3))
    mbs = _matrix(m, "m", B, (3, 4))
    d = _lib.NconvViewWarp()
    if mask is not None:
        _views.require_tensor(mask, "mask", (torch.bool, torch.uint8), PREFIX)
        if mask.dim() == 3:
            mask = mask[:, None]
        if tuple(mask.shape) != (B, 1, H, W):
            raise ValueError(f"{PREFIX}: mask must be ({B}, 1, {H}, {W}) or ({B}, {H}, {W}), got {tuple(mask.shape)}")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        _, _, _, d.mask_image_stride, d.mask_row_stride = _views.plane_view(mask, "mask", PREFIX)
    tstr = None
    if tgt is not None:
        tstr = _image_view(tgt, "tgt", B, C)
        if tuple(tgt.shape[2:]) != (H, W):
            raise ValueError(f"{PREFIX}: tgt of shape {tuple(tgt.shape)} does not match depth's {H} x {W}")
        if tgt.requires_grad:
            raise ValueError(f"{PREFIX}: tgt requires a gradient, and only the depth gets one: pass tgt.detach()")
    z_min = float(z_min)
    z_max = 0.0 if z_max is None else float(z_max)
    if not z_min >= 0.0:
        raise ValueError(f"{PREFIX}: z_min = {z_min} is negative (a valid depth is positive)")
    if z_max != 0.0 and not z_max >= z_min:
        raise ValueError(f"{PREFIX}: z_max = {z_max} < z_min = {z_min}")
    if B * C * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: a batch of (B, C, H, W) = {(B, C, H, W)} is too large (B * C * H * W < 2^31)")
    dev = depth.device
    for name, x in (("depth", depth), ("src", src), ("k", k), ("m", m), ("mask", mask), ("tgt", tgt)):
        if x is None:
            continue
        _views.on_device(x, name, PREFIX, "frames are warped by libnconv")
        if x.device != dev:
            raise RuntimeError(f"{PREFIX}: {name} on {x.device}, depth on {dev}")
    d.B, d.C, d.H, d.W, d.Hs, d.Ws = B, C, H, W, Hs, Ws
    d.depth, d.depth_image_stride, d.depth_row_stride = depth.data_ptr(), dbs, drs
    d.mask = None if mask is None else mask.data_ptr()
    d.src, d.src_image_stride, d.src_channel_stride, d.src_row_stride = src.data_ptr(), sbs, scs, srs
    d.k, d.k_image_stride, d.m, d.m_image_stride = k.data_ptr(), kbs, m.data_ptr(), mbs
    d.z_min, d.z_max = z_min, z_max
    return d, (B, C, H, W), tstr, mask


def workspace_bytes(B, H, W):
    """Bytes of photometric_loss's workspace (nconv_photo_loss_workspace_bytes); its first int32 is n_v."""
    from . import _lib
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31)")
    return _lib.lib().nconv_photo_loss_workspace_bytes(B, H, W)


class ViewWarpFn(torch.autograd.Function):
    """view_warp's kernels (nconv_view_warp_fwd / _bwd); the gradient reaches the depth alone."""

    @staticmethod
    def forward(ctx, depth, k, src, m, mask, z_min, z_max, out):
        from . import _lib
        d, (B, C, H, W), _, mask = _descriptor(depth, k, src, m, mask, z_min, z_max)
        dev = depth.device
        warped = _views.output(out, "warped", (B, C, H, W), torch.float32, dev, PREFIX, source="depth")
        valid = _views.output(out, "valid", (B, H, W), torch.uint8, dev, PREFIX, source="depth")
        rc = _lib.lib().nconv_view_warp_fwd(ctypes.byref(d), _lib.ptr(warped), _lib.ptr(valid), _lib.stream_handle(dev))
        _lib.check(rc, "nconv_view_warp_fwd")
        ctx.z = (z_min, z_max)
        ctx.g_depth = None if out is None else out.get("g_depth")
        ctx.save_for_backward(depth, k, src, m, mask)
        ctx.mark_non_differentiable(valid)
        return warped, valid

    @staticmethod
    def backward(ctx, g_warped, _g_valid):
        from . import _lib
        depth, k, src, m, mask = ctx.saved_tensors
        d, (B, C, H, W), _, _ = _descriptor(depth, k, src, m, mask, *ctx.z)
        g_warped = g_warped.contiguous()
        g = ctx.g_depth if ctx.g_depth is not None else torch.empty((B, 1, H, W), dtype=torch.float32,
                                                                    device=depth.device)
        rc = _lib.lib().nconv_view_warp_bwd(ctypes.byref(d), _lib.ptr(g_warped), _lib.ptr(g),
                                            _lib.stream_handle(depth.device))
        _lib.check(rc, "nconv_view_warp_bwd")
        return g, None, None, None, None, None, None, None


def view_warp(depth, k, src, m, mask=None, z_min=0.0, z_max=None, return_valid=False, out=None):
    """src warped into the target view: (B, C, H, W) fp32, or (warped, valid) with return_valid, valid
    (B, H, W) bool. depth: (B, 1, H, W) fp32, any view of unit-stride rows (DNET's cropped output); k:
    (3, 3) or (B, 3, 3), the target camera; src: (B, C, Hs, Ws) fp32 view of unit-stride rows, C = 1 or
    3, its size its own; m: (3, 4) or (B, 3, 4) (warp_projection); mask: optional bool / uint8
    (B, 1, H, W), 0 = not valid; z_max None: no upper bound. Differentiable in depth only: a src, k or m
    that requires a gradient is refused. out: an optional dict of kept contiguous buffers 'warped',
    'valid' (uint8), 'g_depth' (B, 1, H, W). One launch forward, one backward."""
    warped, valid = ViewWarpFn.apply(depth, k, src, m, mask, z_min, z_max, out)
    return (warped, valid.view(torch.bool)) if return_valid else warped


class PhotoLossFn(torch.autograd.Function):
    """photometric_loss's kernels (nconv_photo_loss_fwd / _bwd); the gradient reaches the depth alone."""

    @staticmethod
    def forward(ctx, depth, k, tgt, src, m, mask, z_min, z_max, out):
        from . import _lib
        d, (B, C, H, W), t, mask = _descriptor(depth, k, src, m, mask, z_min, z_max, tgt)
        dev = depth.device
        nbytes = workspace_bytes(B, H, W)
        ws = _views.output(out, "workspace", (nbytes,), torch.uint8, dev, PREFIX, source="depth")
        loss = _views.output(out, "loss", (), torch.float32, dev, PREFIX, source="depth")
        rc = _lib.lib().nconv_photo_loss_fwd(ctypes.byref(d), _lib.ptr(tgt), t[0], t[1], t[2], _lib.ptr(loss),
                                             _lib.ptr(ws), nbytes, _lib.stream_handle(dev))
        _lib.check(rc, "nconv_photo_loss_fwd")
        ctx.z = (z_min, z_max)
        ctx.g_depth = None if out is None else out.get("g_depth")
        ctx.save_for_backward(depth, k, tgt, src, m, mask, ws)
        n_v = ws[:4].view(torch.int32)[0]
        ctx.mark_non_differentiable(n_v)
        return loss, n_v

    @staticmethod
    def backward(ctx, gloss, _g_n):
        from . import _lib
        depth, k, tgt, src, m, mask, ws = ctx.saved_tensors
        d, (B, C, H, W), t, _ = _descriptor(depth, k, src, m, mask, *ctx.z, tgt)
        gloss = gloss.contiguous()
        g = ctx.g_depth if ctx.g_depth is not None else torch.empty((B, 1, H, W), dtype=torch.float32,
                                                                    device=depth.device)
        rc = _lib.lib().nconv_photo_loss_bwd(ctypes.byref(d), _lib.ptr(tgt), t[0], t[1], t[2], _lib.ptr(gloss),
                                             _lib.ptr(ws), ws.numel(), _lib.ptr(g), _lib.stream_handle(depth.device))
        _lib.check(rc, "nconv_photo_loss_bwd")
        return g, None, None, None, None, None, None, None, None


def photometric_loss(depth, k, tgt, src, m, mask=None, z_min=0.0, z_max=None, return_valid_count=False, out=None):
    """sum over valid pixels and channels of |warp(src) - tgt| / (C max(n_v, 1)): a scalar on the device,
    or (loss, n_v) with return_valid_count, n_v the int32 number of valid pixels (a view of the
    workspace: no host synchronisation). tgt: (B, C, H, W) fp32 view of unit-stride rows, the current
    frame; the other operands as view_warp's. Differentiable in depth only. out: an optional dict of
    kept contiguous buffers 'workspace' (uint8, workspace_bytes(B, H, W)), 'loss' (fp32 scalar),
    'g_depth' (B, 1, H, W). Two launches forward, one backward; warped never reaches memory."""
    loss, n_v = PhotoLossFn.apply(depth, k, tgt, src, m, mask, z_min, z_max, out)
    return (loss, n_v) if return_valid_count else loss


def _ssim_constants(alpha, data_range):
    """(alpha, c1, c2) as Python floats: c1 = (0.01 R)^2 and c2 = (0.03 R)^2 formed in double (ctypes rounds
    them to fp32 once). alpha and data_range are Python numbers, not tensors: constants of a captured graph."""
    if torch.is_tensor(alpha) or torch.is_tensor(data_range):
        raise TypeError(f"{PREFIX}: alpha and data_range must be Python floats (they are constants of the call, "
                        "and of a captured graph), not tensors")
    alpha, R = float(alpha), float(data_range)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{PREFIX}: alpha = {alpha} is outside [0, 1]")
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    f32 = torch.finfo(torch.float32)
    if not (R > 0.0 and f32.tiny <= c1 and c2 <= f32.max):
        raise ValueError(f"{PREFIX}: data_range = {R} must be positive and finite, with (0.01 R)^2 and (0.03 R)^2 "
                         "normal fp32 numbers")
    return alpha, c1, c2


def ssim_workspace_bytes(B, H, W):
    """Bytes of photometric_ssim_loss's workspace (nconv_photo_ssim_workspace_bytes); its first two int32 are
    n_v and n_w."""
    from . import _lib
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31)")
    return _lib.lib().nconv_photo_ssim_workspace_bytes(B, H, W)


class PhotoSsimLossFn(torch.autograd.Function):
    """photometric_ssim_loss's kernels (nconv_photo_ssim_loss_fwd / _bwd); the gradient reaches the depth alone."""

    @staticmethod
    def forward(ctx, depth, k, tgt, src, m, mask, consts, z_min, z_max, out):
        from . import _lib
        d, (B, C, H, W), t, mask = _descriptor(depth, k, src, m, mask, z_min, z_max, tgt)
        dev = depth.device
        nbytes = ssim_workspace_bytes(B, H, W)
        ws = _views.output(out, "workspace", (nbytes,), torch.uint8, dev, PREFIX, source="depth")
        loss = _views.output(out, "loss", (), torch.float32, dev, PREFIX, source="depth")
        rc = _lib.lib().nconv_photo_ssim_loss_fwd(ctypes.byref(d), _lib.ptr(tgt), t[0], t[1], t[2], *consts,
                                                  _lib.ptr(loss), _lib.ptr(ws), nbytes, _lib.stream_handle(dev))
        _lib.check(rc, "nconv_photo_ssim_loss_fwd")
        ctx.z, ctx.consts = (z_min, z_max), consts
        ctx.g_depth = None if out is None else out.get("g_depth")
        ctx.save_for_backward(depth, k, tgt, src, m, mask, ws)
        n = ws[:8].view(torch.int32)
        n_v, n_w = n[0], n[1]
        ctx.mark_non_differentiable(n_v, n_w)
        return loss, n_v, n_w

    @staticmethod
    def backward(ctx, gloss, _g_nv, _g_nw):
        from . import _lib
        depth, k, tgt, src, m, mask, ws = ctx.saved_tensors
        d, (B, C, H, W), t, _ = _descriptor(depth, k, src, m, mask, *ctx.z, tgt)
        gloss = gloss.contiguous()
        g = ctx.g_depth if ctx.g_depth is not None else torch.empty((B, 1, H, W), dtype=torch.float32,
                                                                    device=depth.device)
        rc = _lib.lib().nconv_photo_ssim_loss_bwd(ctypes.byref(d), _lib.ptr(tgt), t[0], t[1], t[2], *ctx.consts,
                                                  _lib.ptr(gloss), _lib.ptr(ws), ws.numel(), _lib.ptr(g),
                                                  _lib.stream_handle(depth.device))
        _lib.check(rc, "nconv_photo_ssim_loss_bwd")
        return g, None, None, None, None, None, None, None, None, None


def photometric_ssim_loss(depth, k, tgt, src, m, mask=None, alpha=0.85, data_range=255.0, z_min=0.0, z_max=None,
                          return_counts=False, out=None):
    """alpha Lw + (1 - alpha) Lv: Lv is photometric_loss's L1 mean over the n_v valid pixels, Lw the mean over
    the n_w windows and the channels of clamp((1 - SSIM) / 2, 0, 1), SSIM over the 3 x 3 window of a pixel whose
    nine pixels are all valid (no reflection padding: the image's one-pixel frame has no window). A scalar on the
    device, or (loss, n_v, n_w) with return_counts, the counts int32 views of the workspace (no host
    synchronisation). alpha (monodepth: 0.85) and data_range (255 for 8-bit-valued frames, 1 for [0, 1]; c1 =
    (0.01 R)^2, c2 = (0.03 R)^2) are Python floats, captured as constants by a graph. The operands as
    photometric_loss's; differentiable in depth only: a src, tgt, k or m that requires a gradient is refused.
    out: an optional dict of kept contiguous buffers 'workspace' (uint8, ssim_workspace_bytes(B, H, W)), 'loss',
    'g_depth' (B, 1, H, W). Two launches forward, one backward; the backward recomputes the warp of each tile and
    its halo, so neither warped nor any SSIM plane reaches memory. At alpha = 0 the loss and the gradient equal
    photometric_loss's."""
    consts = _ssim_constants(alpha, data_range)
    loss, n_v, n_w = PhotoSsimLossFn.apply(depth, k, tgt, src, m, mask, consts, z_min, z_max, out)
    return (loss, n_v, n_w) if return_counts else loss


class PhotometricLoss(torch.nn.Module):
    """photometric_loss with its depth window held: loss(depth, k, tgt, src, m, mask=None). In a
    training step: calculate_loss(pred, gt, True) + w * photo(pred, k, rgb, rgb_near, m), with m refilled
    in place per batch (a GraphedTrainStep input). alpha = 0 (the default) is the L1 loss, exactly as before;
    alpha > 0 is photometric_ssim_loss with that alpha and data_range (Python floats, constants of a capture)."""

    def __init__(self, z_min=0.0, z_max=None, alpha=0.0, data_range=255.0):
        super().__init__()
        if not float(z_min) >= 0.0 or (z_max is not None and not float(z_max) >= float(z_min)):
            raise ValueError(f"{PREFIX}: need 0 <= z_min <= z_max, got z_min={z_min}, z_max={z_max}")
        self.z_min, self.z_max = float(z_min), None if z_max is None else float(z_max)
        self.alpha, _, _ = _ssim_constants(alpha, data_range)
        self.data_range = float(data_range)

    def forward(self, depth, k, tgt, src, m, mask=None):
        if self.alpha == 0.0:
            return photometric_loss(depth, k, tgt, src, m, mask, self.z_min, self.z_max)
        return photometric_ssim_loss(depth, k, tgt, src, m, mask, self.alpha, self.data_range, self.z_min, self.z_max)


class ViewWarper:
    """view_warp and photometric_loss for fixed sizes with their outputs, gradient and workspace kept
    between calls: no allocation after construction, so the calls can be captured with torch.cuda.graph
    and replayed on operands refilled in place. warper(depth, k, src, m) -> warped (or (warped, valid));
    warper.loss(depth, k, tgt, src, m) -> loss (or (loss, n_v)). The returned tensors are the kept ones,
    overwritten by the next call; the warp and the loss keep separate gradient buffers. alpha > 0: .loss is
    photometric_ssim_loss with that alpha and data_range (Python floats) and its own kept workspace, loss
    and gradient buffer; alpha = 0 (the default) is the L1 loss as before."""

    def __init__(self, size, src_size=None, B=1, C=3, device=None, z_min=0.0, z_max=None, alpha=0.0,
                 data_range=255.0):
        H, W = (int(v) for v in size)
        Hs, Ws = (H, W) if src_size is None else (int(v) for v in src_size)
        if min(H, W, Hs, Ws, int(B)) <= 0 or int(C) not in (1, 3):
            raise ValueError(f"{PREFIX}: sizes must be positive and C 1 or 3, got {size}, {src_size}, B={B}, C={C}")
        self.size, self.src_size, self.B, self.C = (H, W), (Hs, Ws), int(B), int(C)
        self.z_min, self.z_max = z_min, z_max
        self.alpha, _, _ = _ssim_constants(alpha, data_range)
        self.data_range = float(data_range)
        dev = torch.device("cuda" if device is None else device)
        f32 = dict(dtype=torch.float32, device=dev)
        self._warp = {"warped": torch.empty(self.B, self.C, H, W, **f32),
                      "valid": torch.empty(self.B, H, W, dtype=torch.uint8, device=dev),
                      "g_depth": torch.empty(self.B, 1, H, W, **f32)}
        self._loss = {"workspace": torch.empty(workspace_bytes(self.B, H, W), dtype=torch.uint8, device=dev),
                      "loss": torch.empty((), **f32), "g_depth": torch.empty(self.B, 1, H, W, **f32)}
        self._ssim = None
        if self.alpha != 0.0:
            self._ssim = {"workspace": torch.empty(ssim_workspace_bytes(self.B, H, W), dtype=torch.uint8, device=dev),
                          "loss": torch.empty((), **f32), "g_depth": torch.empty(self.B, 1, H, W, **f32)}

    def _check(self, depth, src):
        if torch.is_tensor(depth) and torch.is_tensor(src) and depth.dim() == 4 and src.dim() == 4:
            got = (depth.shape[0], src.shape[1], tuple(depth.shape[2:]), tuple(src.shape[2:]))
            if got != (self.B, self.C, self.size, self.src_size):
                raise ValueError(f"{PREFIX}: ViewWarper was built for B={self.B}, C={self.C}, {self.size} from "
                                 f"{self.src_size}; got B={got[0]}, C={got[1]}, {got[2]} from {got[3]}")

    def __call__(self, depth, k, src, m, mask=None, return_valid=False):
        self._check(depth, src)
        return view_warp(depth, k, src, m, mask, self.z_min, self.z_max, return_valid, out=self._warp)

    def loss(self, depth, k, tgt, src, m, mask=None, return_valid_count=False):
        self._check(depth, src)
        if self._ssim is not None:
            r = photometric_ssim_loss(depth, k, tgt, src, m, mask, self.alpha, self.data_range, self.z_min,
                                      self.z_max, return_valid_count, out=self._ssim)
            return r[:2] if return_valid_count else r
        return photometric_loss(depth, k, tgt, src, m, mask, self.z_min, self.z_max, return_valid_count,
                                out=self._loss)


# ------------------------------------------------------------------------------------------------
# the minimum reprojection over several sources, with auto-masking (nconv_photo_min_loss_*)
# ------------------------------------------------------------------------------------------------
MAX_SOURCES = 4
WINNER_MASKED, WINNER_NONE = 254, 255


def _min_descriptors(depth, k, tgt, srcs, ms, mask, z_min, z_max, automask):
    """The S checked descriptors as a ctypes array, (B, C, H, W), tgt's strides and the mask as passed on."""
    from . import _lib
    if torch.is_tensor(srcs) or torch.is_tensor(ms):
        raise TypeError(f"{PREFIX}: srcs and ms must be sequences of 1..{MAX_SOURCES} tensors, not tensors")
    srcs, ms = list(srcs), list(ms)
    if not 1 <= len(srcs) <= MAX_SOURCES or len(ms) != len(srcs):
        raise ValueError(f"{PREFIX}: need 1..{MAX_SOURCES} sources and as many matrices, got {len(srcs)} srcs and "
                         f"{len(ms)} ms")
    if automask and torch.is_tensor(depth) and depth.dim() == 4:  # shapes before devices, as _descriptor does
        H, W = depth.shape[2:]
        for s, src in enumerate(srcs):
            if torch.is_tensor(src) and src.dim() == 4 and tuple(src.shape[2:]) != (H, W):
                raise ValueError(f"{PREFIX}: automask compares the unwarped sources with tgt, so every source must "
                                 f"be {H} x {W}; srcs[{s}] is {src.shape[2]} x {src.shape[3]} (pass automask=False)")
    descs, shape, tstr, mview = [], None, None, None
    for src, m in zip(srcs, ms):
        d, shape, tstr, mview = _descriptor(depth, k, src, m, mask, z_min, z_max, tgt)
        descs.append(d)
    return (_lib.NconvViewWarp * len(descs))(*descs), shape, tstr, mview


def min_workspace_bytes(B, H, W):
    """Bytes of min_reprojection_loss's workspace (nconv_photo_min_workspace_bytes); its first two int32 are n_c
    and n_m, and it holds the winner byte plane the backward reads."""
    from . import _lib
    B, H, W = int(B), int(H), int(W)
    if B <= 0 or H <= 0 or W <= 0 or B * H * W >= 2 ** 31:
        raise ValueError(f"{PREFIX}: a batch of (B, H, W) = {(B, H, W)} is empty or too large (B * H * W < 2^31)")
    return _lib.lib().nconv_photo_min_workspace_bytes(B, H, W)


class MinReprojectionLossFn(torch.autograd.Function):
    """min_reprojection_loss's kernels (nconv_photo_min_loss_fwd / _bwd); the gradient reaches the depth alone."""

    @staticmethod
    def forward(ctx, depth, k, tgt, mask, consts, automask, z_min, z_max, want, out, S, *srcs_ms):
        from . import _lib
        srcs, ms = srcs_ms[:S], srcs_ms[S:]
        views, (B, C, H, W), t, mask = _min_descriptors(depth, k, tgt, srcs, ms, mask, z_min, z_max, automask)
        dev = depth.device
        nbytes = min_workspace_bytes(B, H, W)
        ws = _views.output(out, "workspace", (nbytes,), torch.uint8, dev, PREFIX, source="depth")
        loss = _views.output(out, "loss", (), torch.float32, dev, PREFIX, source="depth")
        winner = _views.output(out, "winner", (B, H, W), torch.uint8, dev, PREFIX, source="depth") if want[0] else None
        error = _views.output(out, "error", (B, H, W), torch.float32, dev, PREFIX, source="depth") if want[1] else None
        rc = _lib.lib().nconv_photo_min_loss_fwd(views, S, _lib.ptr(tgt), t[0], t[1], t[2], *consts, int(automask),
                                                 _lib.ptr(loss), _lib.ptr(winner), _lib.ptr(error), _lib.ptr(ws),
                                                 nbytes, _lib.stream_handle(dev))
        _lib.check(rc, "nconv_photo_min_loss_fwd")
        ctx.z, ctx.consts, ctx.automask, ctx.S = (z_min, z_max), consts, automask, S
        ctx.g_depth = None if out is None else out.get("g_depth")
        ctx.save_for_backward(depth, k, tgt, mask, ws, *srcs_ms)
        n = ws[:8].view(torch.int32)
        n_c, n_m = n[0], n[1]
        ctx.mark_non_differentiable(*(x for x in (n_c, n_m, winner, error) if x is not None))
        return loss, n_c, n_m, winner, error

    @staticmethod
    def backward(ctx, gloss, *_):
        from . import _lib
        depth, k, tgt, mask, ws, *srcs_ms = ctx.saved_tensors
        S = ctx.S
        views, (B, C, H, W), t, _ = _min_descriptors(depth, k, tgt, srcs_ms[:S], srcs_ms[S:], mask, *ctx.z,
                                                     ctx.automask)
        gloss = gloss.contiguous()
        g = ctx.g_depth if ctx.g_depth is not None else torch.empty((B, 1, H, W), dtype=torch.float32,
                                                                    device=depth.device)
        rc = _lib.lib().nconv_photo_min_loss_bwd(views, S, _lib.ptr(tgt), t[0], t[1], t[2], *ctx.consts,
                                                 int(ctx.automask), _lib.ptr(gloss), _lib.ptr(ws), ws.numel(),
                                                 _lib.ptr(g), _lib.stream_handle(depth.device))
        _lib.check(rc, "nconv_photo_min_loss_bwd")
        return (g,) + (None,) * (10 + 2 * S)


def min_reprojection_loss(depth, k, tgt, srcs, ms, mask=None, alpha=0.85, data_range=255.0, automask=True,
                          z_min=0.0, z_max=None, return_counts=False, return_winner=False, return_error=False,
                          out=None):
    """monodepth2's loss over several source frames: per pixel the SMALLEST of E_s = alpha termw_s + (1 - alpha)
    term_s over the sources in which the pixel is comparable (has a window; at alpha = 0: is valid), termw_s and
    term_s the per-pixel channel sums of photometric_ssim_loss's and photometric_loss's terms; the lowest index
    wins a tie. automask: a pixel whose best UNWARPED source matches tgt at least as well (Imin <= best) is
    masked: it adds nothing to the sum but stays in the mean, L = sum over kept pixels of best / (C max(n_c, 1)),
    n_c the pixels with a winner (every source must then have tgt's size). A scalar on the device, followed, as
    asked for, by (n_c, n_m) (return_counts: int32 views of the workspace, n_m the masked pixels), winner
    (return_winner: uint8 (B, H, W), the source's index, 254 masked, 255 none) and error (return_error: fp32
    (B, H, W), best / C of a kept pixel, else 0: the per-pixel error map, ready for colorize). srcs, ms: sequences
    of 1..4 tensors, each as photometric_ssim_loss's src and m (a source may have its own size); the other
    operands as photometric_ssim_loss's; differentiable in depth only. out: an optional dict of kept contiguous
    buffers 'workspace' (uint8, min_workspace_bytes(B, H, W)), 'loss', 'g_depth' (B, 1, H, W), 'winner', 'error'.
    Two launches forward, one backward, whatever the number of sources. With one source and no auto-masking the
    loss and the gradient equal photometric_loss's at alpha = 0 and photometric_ssim_loss's at alpha = 1; in
    between this is a different loss (one mean over the pixels with a window, not two means)."""
    consts = _ssim_constants(alpha, data_range)
    srcs, ms = list(srcs), list(ms)
    if len(ms) != len(srcs):
        raise ValueError(f"{PREFIX}: need as many matrices as sources, got {len(srcs)} srcs and {len(ms)} ms")
    loss, n_c, n_m, winner, error = MinReprojectionLossFn.apply(
        depth, k, tgt, mask, consts, bool(automask), z_min, z_max, (bool(return_winner), bool(return_error)), out,
        len(srcs), *srcs, *ms)
    res = (loss,) + ((n_c, n_m) if return_counts else ()) + ((winner,) if return_winner else ()) \
        + ((error,) if return_error else ())
    return res if len(res) > 1 else loss


class MinReprojectionLoss(torch.nn.Module):
    """min_reprojection_loss with its constants held: loss(depth, k, tgt, srcs, ms, mask=None). In a training
    step: calculate_loss(pred, gt, True) + w * loss(pred, k, rgb, (rgb_prev, rgb_next), (m_prev, m_next)), the ms
    refilled in place per batch (GraphedTrainStep inputs). alpha, data_range and automask are Python values,
    constants of a capture."""

    def __init__(self, alpha=0.85, automask=True, data_range=255.0, z_min=0.0, z_max=None):
        super().__init__()
        if not float(z_min) >= 0.0 or (z_max is not None and not float(z_max) >= float(z_min)):
            raise ValueError(f"{PREFIX}: need 0 <= z_min <= z_max, got z_min={z_min}, z_max={z_max}")
        self.z_min, self.z_max = float(z_min), None if z_max is None else float(z_max)
        self.alpha, _, _ = _ssim_constants(alpha, data_range)
        self.data_range, self.automask = float(data_range), bool(automask)

    def forward(self, depth, k, tgt, srcs, ms, mask=None):
        return min_reprojection_loss(depth, k, tgt, srcs, ms, mask, self.alpha, self.data_range, self.automask,
                                     self.z_min, self.z_max)


class MinReprojector:
    """min_reprojection_loss for fixed sizes with its workspace, loss, gradient, winner and error buffers kept
    between calls: no allocation after construction, so the calls can be captured with torch.cuda.graph and
    replayed on operands refilled in place (ViewWarper's sibling). reproj(depth, k, tgt, srcs, ms) -> loss, or the
    tuple min_reprojection_loss returns with return_counts / return_winner / return_error. The returned tensors
    are the kept ones, overwritten by the next call."""

    def __init__(self, size, S=2, B=1, C=3, device=None, alpha=0.85, data_range=255.0, automask=True, z_min=0.0,
                 z_max=None):
        H, W = (int(v) for v in size)
        if min(H, W, int(B)) <= 0 or int(C) not in (1, 3) or not 1 <= int(S) <= MAX_SOURCES:
            raise ValueError(f"{PREFIX}: sizes must be positive, C 1 or 3 and S in 1..{MAX_SOURCES}, got {size}, "
                             f"S={S}, B={B}, C={C}")
        self.size, self.S, self.B, self.C = (H, W), int(S), int(B), int(C)
        self.z_min, self.z_max = z_min, z_max
        self.alpha, _, _ = _ssim_constants(alpha, data_range)
        self.data_range, self.automask = float(data_range), bool(automask)
        dev = torch.device("cuda" if device is None else device)
        f32 = dict(dtype=torch.float32, device=dev)
        self._out = {"workspace": torch.empty(min_workspace_bytes(self.B, H, W), dtype=torch.uint8, device=dev),
                     "loss": torch.empty((), **f32), "g_depth": torch.empty(self.B, 1, H, W, **f32),
                     "winner": torch.empty(self.B, H, W, dtype=torch.uint8, device=dev),
                     "error": torch.empty(self.B, H, W, **f32)}

    def __call__(self, depth, k, tgt, srcs, ms, mask=None, return_counts=False, return_winner=False,
                 return_error=False):
        srcs = list(srcs)
        if torch.is_tensor(depth) and depth.dim() == 4 and torch.is_tensor(tgt) and tgt.dim() == 4:
            got = (depth.shape[0], tgt.shape[1], tuple(depth.shape[2:]), len(srcs))
            if got != (self.B, self.C, self.size, self.S):
                raise ValueError(f"{PREFIX}: MinReprojector was built for B={self.B}, C={self.C}, {self.size}, "
                                 f"S={self.S}; got B={got[0]}, C={got[1]}, {got[2]}, S={got[3]}")
        return min_reprojection_loss(depth, k, tgt, srcs, ms, mask, self.alpha, self.data_range, self.automask,
                                     self.z_min, self.z_max, return_counts, return_winner, return_error,
                                     out=self._out)
