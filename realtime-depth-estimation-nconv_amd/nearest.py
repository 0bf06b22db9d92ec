"""The nearest input sample of every pixel of a sparse depth plane, and how far away it is, on the device
(nconv_depth_nearest, csrc/nearest.hip): the exact Euclidean distance transform with its feature map.

    nearest_sample   one call: the nearest-neighbour fill, optionally the nearest sample's pixel number,
                     the squared distance and the distance
    NearestFiller    the same with its buffers, the workspace included, kept between calls (hipGraph capture)
    NearestFill      an nn.Module without parameters: compat.utils.get_metrics(NearestFill(), loader, "cuda")
    NearestSample    a batch-dict stage for data.DevicePrefetcher(..., ingest=NearestSample(Ingest()))

The rule is include/nconv.h's: a pixel is a sample when it is finite and > floor; the nearest sample of a
pixel is the one with the smallest squared pixel distance (r - r')^2 + (c - c')^2, ties going to the
smallest pixel number r' * W + c'; with max_distance a pixel farther than that from every sample has none.
Integer geometry: tests/nearest_cases.py restates it in numpy by brute force and the GPU tests hold the
kernels to it bit for bit.

Nearest-neighbour interpolation is the other non-learned baseline of the depth-completion tables (Uhrig et
al., "Sparsity Invariant CNNs", 3DV 2017; Ma and Karaman, "Sparse-to-Dense", ICRA 2018). Unlike IP-Basic
it fills every pixel of an image that has a sample at all, and it keeps its input samples bit for bit.
The distance plane stratifies an error by the distance to the nearest return,

    _, d2 = nearest_sample(S, return_dist2=True)
    near.update(pred, gt * (d2 <= 4 * 4)[:, None]); far.update(pred, gt * (d2 > 32 * 32)[:, None])

(two DepthMetrics; where there is no sample at all dist2 is 0x7FFFFFFF, so it counts as far), and trims what
a network had no evidence for from a cloud: backproject(depth * (d2 <= r * r)[:, None], K) drops every
pixel farther than r pixels from any return, as conf_min drops the ones the network itself doubts.
"""
import ctypes
import math

import torch

from . import _views

_PREFIX = "nearest"
_DOING = "the transform runs in libnconv"
_OPTIONS = ("floor", "max_distance", "return_index", "return_dist2", "return_dist")
_EXTRAS = (("return_index", "index", torch.int32), ("return_dist2", "dist2", torch.int32),
           ("return_dist", "dist", torch.float32))
NO_DIST2 = 0x7FFFFFFF  # dist2 where a pixel has no nearest sample


def _max_dist2(max_distance):
    """max_dist2 of the C boundary: floor(r * r) clipped to int32, -1 (no limit) for None."""
    if max_distance is None:
        return -1
    r = float(max_distance)
    if not r >= 0.0:
        raise ValueError(f"{_PREFIX}: max_distance = {max_distance} must be >= 0 (or None: no limit)")
    r2 = r * r
    return NO_DIST2 if r2 >= NO_DIST2 else int(math.floor(r2))


def nearest_sample(S, floor=0.0, max_distance=None, return_index=False, return_dist2=False, return_dist=False,
                   out=None):
    """The sparse plane S filled from its nearest samples: (B, 1, H, W) fp32, at every pixel the value of
    the nearest sample bit for bit (a sample keeps its own value), +0.0 where there is none. With
    return_index, return_dist2 and / or return_dist a tuple (depth[, index][, dist2][, dist]): index
    (B, H, W) int32, the pixel number r' * W + c' of the nearest sample, -1 where there is none; dist2
    (B, H, W) int32, the squared pixel distance to it, 0x7FFFFFFF where there is none (so that
    dist2 <= r * r is false there); dist (B, H, W) fp32, its correctly rounded square root, +inf.

    S: (H, W), (1, H, W) or (B, 1, H, W) fp32 on the device, any view of unit-stride rows. A pixel is a
    sample iff it is finite and > floor (floor=None: every finite value). The nearest sample has the
    smallest (r - r')^2 + (c - c')^2; ties go to the smallest pixel number. max_distance: a float >= 0,
    a pixel whose nearest sample is farther than that many pixels has none (the kernel compares the
    squared distance with floor(max_distance^2)); None: no limit. An image without samples has none
    anywhere.
    out: an optional dict of preallocated buffers 'depth' ((B, 1, H, W) fp32 of unit-stride rows),
    'index', 'dist2', 'dist' and the workspace 'work' ((B, H, W) int32, overwritten), none of them
    overlapping S or another. Two kernel launches, no host synchronisation and, with out complete, no
    allocation: capturable with torch.cuda.graph."""
    from . import _lib
    _views.require_tensor(S, "S", (torch.float32,), _PREFIX)
    B, H, W, sbs, srs = _views.plane_view(S, "S", _PREFIX)
    floor = -math.inf if floor is None else float(floor)
    if floor != floor:
        raise ValueError(f"{_PREFIX}: floor is NaN")
    max_dist2 = _max_dist2(max_distance)
    dev = S.device
    dst, dbs, drs = _views.dest_plane(out, "depth", B, H, W, dev, _PREFIX, source="S")
    asked = dict(return_index=return_index, return_dist2=return_dist2, return_dist=return_dist)
    extras = {key: _views.output(out, key, (B, H, W), dtype, dev, _PREFIX, source="S") if asked[flag] else None
              for flag, key, dtype in _EXTRAS}
    work = _views.output(out, "work", (B, H, W), torch.int32, dev, _PREFIX, source="S")
    _views.on_device(S, "S", _PREFIX, _DOING)  # after the buffers: a malformed out is refused on any device
    d = _lib.NconvDepthNearest()
    d.B, d.H, d.W = B, H, W
    d.src, d.src_image_stride, d.src_row_stride = S.data_ptr(), sbs, srs
    d.floor, d.max_dist2 = floor, max_dist2
    rc = _lib.lib().nconv_depth_nearest(ctypes.byref(d), _lib.ptr(dst), dbs, drs, _lib.ptr(extras["index"]),
                                        _lib.ptr(extras["dist2"]), _lib.ptr(extras["dist"]), _lib.ptr(work),
                                        _lib.stream_handle(dev))
    _lib.check(rc, "nconv_depth_nearest")
    r = (dst,) + tuple(extras[key] for _, key, _ in _EXTRAS if extras[key] is not None)
    return r if len(r) > 1 else dst


def _check_options(options, who, allowed=_OPTIONS):
    for k in options:
        if k not in allowed:
            raise TypeError(f"{_PREFIX}: {who} takes no option {k!r}")


class NearestFiller:
    """nearest_sample for a fixed (H, W) and batch size B with its outputs and its workspace kept between
    calls: no allocation after the first call on a device, so a call can be captured with
    torch.cuda.graph and replayed on a source refilled in place. options: nearest_sample's keyword
    arguments (floor, max_distance, return_index, return_dist2, return_dist). Returns the kept tensors,
    overwritten by the next call."""

    def __init__(self, size, B=1, **options):
        self.size, self.B = (int(size[0]), int(size[1])), int(B)
        _check_options(options, "NearestFiller")
        self.options = options
        self._dev, self._out = None, None

    def __call__(self, S):
        if torch.is_tensor(S) and S.is_cuda and S.device != self._dev:
            H, W = self.size
            out = {"depth": torch.empty(self.B, 1, H, W, device=S.device),
                   "work": torch.empty(self.B, H, W, dtype=torch.int32, device=S.device)}
            for flag, key, dtype in _EXTRAS:
                if self.options.get(flag):
                    out[key] = torch.empty(self.B, H, W, dtype=dtype, device=S.device)
            self._dev, self._out = S.device, out
        return nearest_sample(S, out=self._out, **self.options)


class NearestFill(torch.nn.Module):
    """Nearest-neighbour interpolation as a model without parameters: forward(depth) is
    nearest_sample(depth, **options), so compat.utils.get_metrics(NearestFill(), loader, "cuda") scores
    the baseline through the loop that scores the networks. options: floor, max_distance."""

    def __init__(self, **options):
        super().__init__()
        _check_options(options, "NearestFill", ("floor", "max_distance"))
        self.options = options

    def forward(self, depth):
        return nearest_sample(depth, **self.options)

    def extra_repr(self):
        return ", ".join(f"{k}={v!r}" for k, v in self.options.items())


class NearestSample:
    """A batch-dict stage for data.DevicePrefetcher(..., ingest=NearestSample(chain=Ingest())): chain
    (frames.Ingest(), ...) is called on the batch first, so that batch[key] is fp32; then
    batch[out_key] is the nearest-neighbour fill of batch[key] and, where dist_key is named,
    batch[dist_key] the fp32 distance to the nearest sample as (B, 1, H, W). options: floor,
    max_distance. Every other entry is passed through untouched."""

    def __init__(self, chain=None, key="depth", out_key="filled", dist_key=None, **options):
        _check_options(options, "NearestSample", ("floor", "max_distance"))
        self.chain, self.key, self.out_key, self.dist_key, self.options = chain, key, out_key, dist_key, options

    def __call__(self, batch):
        if self.chain is not None:
            batch = self.chain(batch)
        batch = dict(batch)
        if self.dist_key is None:
            batch[self.out_key] = nearest_sample(batch[self.key], **self.options)
        else:
            batch[self.out_key], dist = nearest_sample(batch[self.key], return_dist=True, **self.options)
            batch[self.dist_key] = dist[:, None]
        return batch
