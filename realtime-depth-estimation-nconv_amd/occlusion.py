"""Occluded LiDAR returns taken out of a sparse depth plane on the device (nconv_depth_occlusion,
csrc/occlusion.hip).

The scanner does not sit where the camera sits (KITTI: about 8 cm above and 27 cm behind cam0), so beside
every foreground silhouette a projected scan holds background returns the camera cannot see, between the
foreground returns. lidar.project_points resolves collisions on one pixel only, and KITTI's velodyne_raw
PNGs hold such returns too. To a normalised convolution they are confidence-1 samples tens of metres off,
right at the depth edges.

    remove_occluded   one call: the filtered plane, optionally the removed mask, the counts, and a
                      project_points index plane updated in place
    OcclusionFilter   the same with its outputs kept between calls (hipGraph capture)
    RemoveOccluded    a batch-dict stage for data.DevicePrefetcher(..., ingest=RemoveOccluded(Ingest()))

The rule is include/nconv.h's: a valid pixel p (finite, > floor) is removed when at least min_support
valid pixels q of its (2 rh + 1) x (2 rw + 1) window, clipped at the image border, have
v_p > v_q + (jump_abs + jump_rel * v_q). tests/occlusion_cases.py restates it in numpy and the GPU tests
hold the kernel to it bit for bit.

The defaults (7 x 7 window, 1 m, one supporter) are a common convention; nobody has measured them on
KITTI. What the rule cannot avoid: a visible background return just outside a silhouette is dropped as
well; on the road surface a tall window with a small jump removes far ground returns in favour of the
nearer scan line below them; min_support > 1 keeps one stray near return (dust, rain) from clearing a
window of good ones.
"""
import ctypes
import math

import torch

from . import _views

_PREFIX = "occlusion"
_DOING = "the filter runs in libnconv"
MAX_RADIUS = 16


def _window(window):
    if hasattr(window, "__index__"):
        rh = rw = int(window)
    else:
        try:
            rh, rw = (int(v) for v in window)
        except (TypeError, ValueError):
            raise TypeError(f"{_PREFIX}: window must be an int or (rh, rw), got {window!r}") from None
    if not (0 <= rh <= MAX_RADIUS and 0 <= rw <= MAX_RADIUS):
        raise ValueError(f"{_PREFIX}: window = {(rh, rw)} outside 0..{MAX_RADIUS}")
    return rh, rw


def remove_occluded(S, window=(3, 3), jump_abs=1.0, jump_rel=0.0, min_support=1, floor=0.0, index=None,
                    return_removed=False, return_counts=False, out=None):
    """The plane S without its occluded returns: (B, 1, H, W) fp32, S's value bit for bit where the pixel
    is valid and kept, +0.0 elsewhere. With return_removed and / or return_counts a tuple (depth[, removed]
    [, counts]): removed (B, H, W) uint8, 1 where a return was dropped; counts (B, 2) int32 = (valid,
    removed) per image.

    S: (H, W), (1, H, W) or (B, 1, H, W) fp32 on the device, any view of unit-stride rows. window: the
    half-sizes (rh, rw) of the (2 rh + 1) x (2 rw + 1) window, each 0..16, or an int for a square one.
    A pixel is valid iff it is finite and > floor (floor=None: every finite value); a valid pixel is
    removed when at least min_support valid pixels q of its window have
    S[p] > S[q] + (jump_abs + jump_rel * S[q]). The window is clipped at the image border.
    index: the (B, H, W) int32 plane of lidar.project_points(..., return_index=True); it is set to -1 in
    place where the pixel is removed or not valid, so its non-negative entries are the scan rows that
    survive. An int32 tensor in window's place is taken as the index, so that
    remove_occluded(*project_points(points, offsets, m, size, return_index=True)) reads as it should.
    out: an optional dict of preallocated buffers 'depth' ((B, 1, H, W) fp32 of unit-stride rows, not
    overlapping S), 'removed' and 'counts'. One kernel launch (two with counts), no host synchronisation
    and, with out complete, no allocation: capturable with torch.cuda.graph.
    The defaults are a convention nobody has measured on KITTI; see the module's text for what the rule
    drops besides occluded returns."""
    from . import _lib
    if torch.is_tensor(window):
        if index is not None:
            raise TypeError(f"{_PREFIX}: a tensor in window's place is the index, and index is given too")
        index, window = window, (3, 3)
    _views.require_tensor(S, "S", (torch.float32,), _PREFIX)
    B, H, W, sbs, srs = _views.plane_view(S, "S", _PREFIX)
    rh, rw = _window(window)
    jump_abs, jump_rel = float(jump_abs), float(jump_rel)
    if not (jump_abs >= 0.0 and jump_rel >= 0.0):
        raise ValueError(f"{_PREFIX}: jump_abs = {jump_abs}, jump_rel = {jump_rel}: both must be >= 0")
    min_support = int(min_support)
    if min_support < 1:
        raise ValueError(f"{_PREFIX}: min_support = {min_support} is below 1")
    floor = -math.inf if floor is None else float(floor)
    if floor != floor:
        raise ValueError(f"{_PREFIX}: floor is NaN")
    if index is not None:
        _views.require_tensor(index, "index", (torch.int32,), _PREFIX)
        if tuple(index.shape) != (B, H, W) or not index.is_contiguous():
            raise ValueError(f"{_PREFIX}: index must be a contiguous ({B}, {H}, {W}) plane, got {tuple(index.shape)} "
                             f"of strides {index.stride()}")
    _views.on_device(S, "S", _PREFIX, _DOING)
    dev = S.device
    if index is not None:
        _views.on_device(index, "index", _PREFIX, _DOING)
        if index.device != dev:
            raise RuntimeError(f"{_PREFIX}: index on {index.device}, S on {dev}")
    dst, dbs, drs = _views.dest_plane(out, "depth", B, H, W, dev, _PREFIX, source="S")
    removed = counts = None
    if return_removed:
        removed = _views.output(out, "removed", (B, H, W), torch.uint8, dev, _PREFIX, source="S")
    if return_counts:
        counts = _views.output(out, "counts", (B, 2), torch.int32, dev, _PREFIX, source="S")
    d = _lib.NconvDepthOcclusion()
    d.B, d.H, d.W, d.rh, d.rw, d.min_support = B, H, W, rh, rw, min(min_support, 0x7FFFFFFF)
    d.src, d.src_image_stride, d.src_row_stride = S.data_ptr(), sbs, srs
    d.jump_abs, d.jump_rel, d.floor = jump_abs, jump_rel, floor
    rc = _lib.lib().nconv_depth_occlusion(ctypes.byref(d), _lib.ptr(dst), dbs, drs, _lib.ptr(removed), _lib.ptr(index),
                                          _lib.ptr(counts), _lib.stream_handle(dev))
    _lib.check(rc, "nconv_depth_occlusion")
    r = (dst,) + ((removed,) if return_removed else ()) + ((counts,) if return_counts else ())
    return r if len(r) > 1 else dst


class OcclusionFilter:
    """remove_occluded for a fixed (H, W) and batch size B with the outputs kept between calls: no
    allocation after the first call on a device, so a call can be captured with torch.cuda.graph and
    replayed on a source refilled in place. options: remove_occluded's keyword arguments (window,
    jump_abs, jump_rel, min_support, floor, return_removed, return_counts). Returns the kept tensors,
    overwritten by the next call."""

    def __init__(self, size, B=1, **options):
        self.size, self.B = (int(size[0]), int(size[1])), int(B)
        for k in ("index", "out"):
            if k in options:
                raise TypeError(f"{_PREFIX}: OcclusionFilter takes no option {k!r}")
        self.options = options
        self._dev, self._out = None, None

    def __call__(self, S, index=None):
        if torch.is_tensor(S) and S.is_cuda and S.device != self._dev:
            H, W = self.size
            out = {"depth": torch.empty(self.B, 1, H, W, device=S.device)}
            if self.options.get("return_removed"):
                out["removed"] = torch.empty(self.B, H, W, dtype=torch.uint8, device=S.device)
            if self.options.get("return_counts"):
                out["counts"] = torch.empty(self.B, 2, dtype=torch.int32, device=S.device)
            self._dev, self._out = S.device, out
        return remove_occluded(S, index=index, out=self._out, **self.options)


class RemoveOccluded:
    """A batch-dict stage for data.DevicePrefetcher(..., ingest=RemoveOccluded(chain=Ingest())): chain
    (frames.Ingest(), ...) is called on the batch first, so that batch['depth'] is fp32; then
    batch['depth'] is replaced by remove_occluded(batch['depth'], **options). Every other entry is
    passed through untouched."""

    def __init__(self, chain=None, **options):
        for k in ("index", "out", "return_removed", "return_counts"):
            if k in options:
                raise TypeError(f"{_PREFIX}: RemoveOccluded takes no option {k!r}")
        self.chain, self.options = chain, options

    def __call__(self, batch):
        if self.chain is not None:
            batch = self.chain(batch)
        batch = dict(batch)
        batch["depth"] = remove_occluded(batch["depth"], **self.options)
        return batch
