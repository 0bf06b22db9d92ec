"""Classical depth completion of a sparse depth plane on the device: the IP-Basic baseline
(nconv_depth_ipbasic, csrc/ipbasic.hip).

IP-Basic (Ku, Harakeh, Waslander, "In Defense of Classical Image Processing: Fast Depth Completion on the
CPU", CRV 2018) is the non-learned method every depth-completion table puts beside its networks, and what
people use to pre-densify a sparse plane or to get a quick dense picture of a scan.

    ipbasic_fill    one call: the completed plane
    IPBasicFiller   the same with its buffers kept between calls (hipGraph capture)
    IPBasic         an nn.Module without parameters: compat.utils.get_metrics(IPBasic(), loader, "cuda")
    IPBasicFill     a batch-dict stage for data.DevicePrefetcher(..., ingest=IPBasicFill(Ingest()))

The rule is include/nconv.h's, fill_in_fast of IP-Basic made total and deterministic: depths are inverted
(max_depth - d; 0 where there is no sample), dilated with the custom kernel, closed with a full 5 x 5,
holes filled from a full 7 x 7 dilation, optionally extrapolated to the top of the image and filled from a
31 x 31 dilation, then a 5 x 5 median, a 5 x 5 Gaussian blur of the valid pixels, and inverted back.
tests/ipbasic_cases.py restates it in numpy and the GPU tests hold the kernel to it bit for bit.

IP-Basic does not preserve its input samples (the median and the blur move them) unless keep_samples is
set. The upstream script's bilateral blur needs exp, which cannot be fixed bit for bit, and is not offered.
Parity with the cv2 script itself is not pinned: cv2 is not a dependency here.
"""
import ctypes
import math

import torch

from . import _views

_PREFIX = "ipbasic"
_DOING = "the completion runs in libnconv"
_OPTIONS = ("max_depth", "kernel", "extrapolate", "median", "blur", "keep_samples")


def _kernel(kernel):
    from . import _lib
    try:
        shape, size = kernel
    except (TypeError, ValueError):
        raise TypeError(f"{_PREFIX}: kernel must be (shape, size), got {kernel!r}") from None
    if not isinstance(shape, str) or not hasattr(size, "__index__"):
        raise TypeError(f"{_PREFIX}: kernel must be (shape, size), got {kernel!r}")
    if shape not in _lib.IPBASIC_KERNELS:
        raise ValueError(f"{_PREFIX}: kernel shape {shape!r} is not one of {sorted(_lib.IPBASIC_KERNELS)}")
    if int(size) not in (3, 5, 7):
        raise ValueError(f"{_PREFIX}: kernel size {int(size)} is not 3, 5 or 7")
    return _lib.IPBASIC_KERNELS[shape], int(size)


def _blur(blur):
    from . import _lib
    if blur is not None and not isinstance(blur, str):
        raise TypeError(f"{_PREFIX}: blur must be 'gaussian', 'none' or None, got {blur!r}")
    if blur == "bilateral":
        raise ValueError(f"{_PREFIX}: blur 'bilateral' is not offered (it needs exp, which cannot be fixed bit for "
                         "bit); use 'gaussian' or None")
    if blur not in _lib.IPBASIC_BLURS:
        raise ValueError(f"{_PREFIX}: blur {blur!r} is not 'gaussian', 'none' or None")
    return _lib.IPBASIC_BLURS[blur]


def ipbasic_fill(S, max_depth=100.0, kernel=("diamond", 5), extrapolate=False, median=True, blur="gaussian",
                 keep_samples=False, out=None):
    """The sparse plane S completed by IP-Basic: (B, 1, H, W) fp32, +0.0 where nothing could be filled.

    S: (H, W), (1, H, W) or (B, 1, H, W) fp32 on the device, any view of unit-stride rows. A pixel is a
    sample when it is finite, > 0.1 and below max_depth - 0.1; everything else (NaN, inf, negatives,
    zeros) is empty. kernel: (shape, size) of the first dilation, shape 'full', 'cross' or 'diamond', size
    3, 5 or 7. extrapolate: carry each column's top value to the top of the image and fill what is left
    from a 31 x 31 dilation. median: the 5 x 5 median. blur: 'gaussian' (5 x 5, of the valid pixels) or
    None / 'none'. keep_samples: the input samples come out bit for bit; without it IP-Basic does not
    preserve them.
    out: an optional dict of preallocated buffers 'depth' ((B, 1, H, W) fp32 of unit-stride rows, not
    overlapping S) and, with extrapolate, 'work' ((B, H, W) fp32) and 'top' ((B, W) int32). One kernel
    launch (three with extrapolate), no host synchronisation and, with out complete, no allocation:
    capturable with torch.cuda.graph."""
    from . import _lib
    _views.require_tensor(S, "S", (torch.float32,), _PREFIX)
    B, H, W, sbs, srs = _views.plane_view(S, "S", _PREFIX)
    max_depth = float(max_depth)
    if not (math.isfinite(max_depth) and max_depth > 0.2):
        raise ValueError(f"{_PREFIX}: max_depth = {max_depth} must be finite and above 0.2")
    shape, size = _kernel(kernel)
    blur = _blur(blur)
    _views.on_device(S, "S", _PREFIX, _DOING)
    dev = S.device
    dst, dbs, drs = _views.dest_plane(out, "depth", B, H, W, dev, _PREFIX, source="S")
    work = top = None
    if extrapolate:
        work = _views.output(out, "work", (B, H, W), torch.float32, dev, _PREFIX, source="S")
        top = _views.output(out, "top", (B, W), torch.int32, dev, _PREFIX, source="S")
    d = _lib.NconvDepthIpbasic()
    d.B, d.H, d.W = B, H, W
    d.src, d.src_image_stride, d.src_row_stride = S.data_ptr(), sbs, srs
    d.max_depth, d.kernel_shape, d.kernel_size = max_depth, shape, size
    d.extrapolate, d.median, d.blur, d.keep_samples = bool(extrapolate), bool(median), blur, bool(keep_samples)
    rc = _lib.lib().nconv_depth_ipbasic(ctypes.byref(d), _lib.ptr(dst), dbs, drs, _lib.ptr(work), _lib.ptr(top),
                                        _lib.stream_handle(dev))
    _lib.check(rc, "nconv_depth_ipbasic")
    return dst


def _check_options(options, who):
    for k in options:
        if k not in _OPTIONS:
            raise TypeError(f"{_PREFIX}: {who} takes no option {k!r}")


class IPBasicFiller:
    """ipbasic_fill for a fixed (H, W) and batch size B with its buffers kept between calls: no allocation
    after the first call on a device, so a call can be captured with torch.cuda.graph and replayed on a
    source refilled in place. options: ipbasic_fill's keyword arguments (max_depth, kernel, extrapolate,
    median, blur, keep_samples). Returns the kept tensor, overwritten by the next call."""

    def __init__(self, size, B=1, **options):
        self.size, self.B = (int(size[0]), int(size[1])), int(B)
        _check_options(options, "IPBasicFiller")
        self.options = options
        self._dev, self._out = None, None

    def __call__(self, S):
        if torch.is_tensor(S) and S.is_cuda and S.device != self._dev:
            H, W = self.size
            out = {"depth": torch.empty(self.B, 1, H, W, device=S.device)}
            if self.options.get("extrapolate"):
                out["work"] = torch.empty(self.B, H, W, device=S.device)
                out["top"] = torch.empty(self.B, W, dtype=torch.int32, device=S.device)
            self._dev, self._out = S.device, out
        return ipbasic_fill(S, out=self._out, **self.options)


class IPBasic(torch.nn.Module):
    """IP-Basic as a model without parameters: forward(depth) is ipbasic_fill(depth, **options), so
    compat.utils.get_metrics(IPBasic(extrapolate=True), loader, "cuda") scores the classical baseline
    through the loop that scores the networks."""

    def __init__(self, **options):
        super().__init__()
        _check_options(options, "IPBasic")
        self.options = options

    def forward(self, depth):
        return ipbasic_fill(depth, **self.options)

    def extra_repr(self):
        return ", ".join(f"{k}={v!r}" for k, v in self.options.items())


class IPBasicFill:
    """A batch-dict stage for data.DevicePrefetcher(..., ingest=IPBasicFill(chain=Ingest())): chain
    (frames.Ingest(), ...) is called on the batch first, so that batch[key] is fp32; then
    batch[out_key] = ipbasic_fill(batch[key], **options), out_key=None replacing batch[key]. Every other
    entry is passed through untouched."""

    def __init__(self, chain=None, key="depth", out_key=None, **options):
        _check_options(options, "IPBasicFill")
        self.chain, self.key, self.out_key, self.options = chain, key, key if out_key is None else out_key, options

    def __call__(self, batch):
        if self.chain is not None:
            batch = self.chain(batch)
        batch = dict(batch)
        batch[self.out_key] = ipbasic_fill(batch[self.key], **self.options)
        return batch
