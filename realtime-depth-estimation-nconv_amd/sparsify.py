"""Random sparse-depth sampling on the device (nconv_depth_sparsify, csrc/sparsify.hip): an exact number
of random samples per image, a function of (input, seed, draw) alone.

    sparsify        one call: "N random samples", a kept fraction, a mask, optional noise
    Sparsifier      the same with its buffers and a device-side (seed, draw) state kept between calls,
                    so a call can be captured with torch.cuda.graph and every replay draws a new sample
    SparsifyBatch   the reference's NYU rule (DataLoader_NYU.preprocess_depth) as a batch stage of
                    data.DevicePrefetcher, for DataLoader_NYU(sparse="device")

The rule is include/nconv.h's: the kept pixels of image b are the n_b candidates with the smallest
(Philox word & key_mask, pixel number); tests/sparsify_cases.py restates it in numpy and the GPU tests
hold the kernels to it bit for bit. It does not reproduce torch.randperm's stream.
"""
import ctypes
import math

import torch

from . import _views

_PREFIX = "sparsify"
_DOING = "the sampling runs in libnconv"


def _on_device(x, what):
    _views.on_device(x, what, _PREFIX, _DOING)


def _output(out, key, shape, dtype, device):
    return _views.output(out, key, shape, dtype, device, _PREFIX, source="depth")


def workspace_bytes(B, H, W):
    """Bytes of the 'workspace' buffer of sparsify for a (B, 1, H, W) batch."""
    from . import _lib
    return _lib.lib().nconv_depth_sparsify_workspace_bytes(B, H, W)


def noise_threshold(noise_frac):
    """floor(noise_frac * 2^32) in double, clamped to [0, 2^32 - 1]: a kept pixel is noisy iff its
    second Philox word is below it."""
    f = float(noise_frac)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"{_PREFIX}: noise_frac = {noise_frac} outside [0, 1]")
    return min(max(int(math.floor(f * 4294967296.0)), 0), 0xFFFFFFFF)


def state_words(seed, draw):
    """(seed_lo, seed_hi, draw) as the three int32 the device state holds (the bits of the uint32 words)."""
    seed, draw = int(seed), int(draw)
    words = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, draw & 0xFFFFFFFF)
    return [w - (1 << 32) if w >= (1 << 31) else w for w in words]


def make_state(seed, draw, device):
    """A (3,) int32 device state, uploaded from pinned memory without a synchronisation."""
    return torch.tensor(state_words(seed, draw), dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def sparsify(depth, n=None, *, keep=None, seed=0, draw=0, state=None, mask=None, floor=0.0, noise_frac=0.0,
             noise_amp=0.1, key_mask=0xFFFFFFFF, return_kept=False, out=None):
    """A random subset of a depth plane with an exact number of samples per image: (B, 1, H, W) fp32, the
    kept pixels' values and +0.0 elsewhere; with return_kept (depth, kept), kept (B,) int32 the number
    kept per image.

    depth: (H, W), (1, H, W) or (B, 1, H, W) fp32 on the device, any view of unit-stride rows (a cropped
    view samples like its contiguous copy: the random words belong to the logical pixel number).
    Candidates are the pixels with depth > floor (and finite), or every pixel with floor=None (the
    reference's NYU rule, which spends part of its budget on empty pixels), that the mask (uint8 (H, W)
    or (B, 1, H, W) on the device, non-zero = pass) lets through. Of an image's C candidates
      n (int)                 min(n, C) are kept
      n ((B,) int32 tensor)   min(max(n[b], 0), C), read on the device
      keep (0..1)             floor(keep * C)
      neither                 all C (mask and noise only)
    n and keep are mutually exclusive. The draw is Philox4x32-10 keyed by the 64-bit seed at counter
    (pixel, image, draw): `state`, a (3,) int32 device tensor (seed_lo, seed_hi, draw), replaces seed and
    draw and is only read; without it the three words are uploaded from pinned memory, with no
    synchronisation. key_mask below 0xffffffff forces ties onto the pixel number (0: the first pixels in
    raster order); it exists for tests.
    noise_frac > 0: a kept pixel is perturbed with probability noise_frac, d + d * (noise_amp * s) with s
    uniform in [-1, 1). This is Bernoulli per pixel, whereas the reference perturbs an exact 10 % count of
    the pixels.
    out: an optional dict of preallocated buffers 'depth' ((B, 1, H, W) fp32 of unit-stride rows; it may
    be `depth` itself: in place), 'kept' ((B,) int32) and 'workspace' (uint8, workspace_bytes(B, H, W)).
    Eight kernel launches whatever the data and n, no host synchronisation, and no
    allocation when out is complete and state is given: capturable with torch.cuda.graph."""
    from . import _lib
    _views.require_tensor(depth, "depth", (torch.float32,), _PREFIX)
    B, H, W, sbs, srs = _views.plane_view(depth, "depth", _PREFIX)
    if n is not None and keep is not None:
        raise ValueError(f"{_PREFIX}: n and keep are mutually exclusive")
    n_dev = None
    n_host, keep_f = 0, 0.0
    if n is None and keep is None:
        mode = _lib.SPARSIFY_ALL
    elif keep is not None:
        mode, keep_f = _lib.SPARSIFY_FRACTION, float(keep)
        if not 0.0 <= keep_f <= 1.0:
            raise ValueError(f"{_PREFIX}: keep = {keep} outside [0, 1]")
    elif torch.is_tensor(n):
        mode, n_dev = _lib.SPARSIFY_COUNT_DEV, n
        _views.require_tensor(n, "n", (torch.int32,), _PREFIX)
        if tuple(n.shape) != (B,) or not n.is_contiguous():
            raise ValueError(f"{_PREFIX}: a tensor n must be a contiguous ({B},) vector, got {tuple(n.shape)}")
    else:
        mode, n_host = _lib.SPARSIFY_COUNT, int(n)
        if n_host < 0:
            raise ValueError(f"{_PREFIX}: n = {n} is negative")
        n_host = min(n_host, 0x7FFFFFFF)
    mbs = mrs = 0
    if mask is not None:
        _views.require_tensor(mask, "mask", (torch.uint8,), _PREFIX)
        mB, mH, mW, mbs, mrs = _views.plane_view(mask, "mask", _PREFIX)
        if (mH, mW) != (H, W) or mB not in (1, B):
            raise ValueError(f"{_PREFIX}: mask of shape {tuple(mask.shape)} does not match depth {tuple(depth.shape)}")
        if mB == 1:
            mbs = 0
    thr = noise_threshold(noise_frac)
    key_mask = int(key_mask)
    if not 0 <= key_mask <= 0xFFFFFFFF:
        raise ValueError(f"{_PREFIX}: key_mask = {key_mask:#x} is not a 32-bit mask")
    if state is not None:
        _views.require_tensor(state, "state", (torch.int32,), _PREFIX)
        if tuple(state.shape) != (3,) or not state.is_contiguous():
            raise ValueError(f"{_PREFIX}: state must be a contiguous (3,) vector, got {tuple(state.shape)}")
    _on_device(depth, "depth")
    dev = depth.device
    for t, what in ((mask, "mask"), (n_dev, "n"), (state, "state")):
        if t is not None:
            _on_device(t, what)
            if t.device != dev:
                raise RuntimeError(f"{_PREFIX}: {what} on {t.device}, depth on {dev}")
    dst, dbs, drs = _views.dest_plane(out, "depth", B, H, W, dev, _PREFIX, source="the depth")
    kept = _output(out, "kept", (B,), torch.int32, dev) if (return_kept or (out and "kept" in out)) else None
    nws = workspace_bytes(B, H, W)
    ws = _output(out, "workspace", (nws,), torch.uint8, dev)
    if state is None:
        state = make_state(seed, draw, dev)
    d = _lib.NconvDepthSparsify()
    d.B, d.H, d.W, d.mode = B, H, W, mode
    d.src, d.src_image_stride, d.src_row_stride = depth.data_ptr(), sbs, srs
    if mask is not None:
        d.mask, d.mask_image_stride, d.mask_row_stride = mask.data_ptr(), mbs, mrs
    d.state = state.data_ptr()
    d.n_dev = None if n_dev is None else n_dev.data_ptr()
    d.n, d.keep = n_host, keep_f
    d.all_pixels, d.floor = int(floor is None), (0.0 if floor is None else float(floor))
    d.key_mask, d.noise_threshold, d.noise_amp = key_mask, thr, float(noise_amp)
    rc = _lib.lib().nconv_depth_sparsify(ctypes.byref(d), _lib.ptr(dst), dbs, drs, _lib.ptr(kept), _lib.ptr(ws), nws,
                                         _lib.stream_handle(dev))
    _lib.check(rc, "nconv_depth_sparsify")
    return (dst, kept) if return_kept else dst


class Sparsifier:
    """sparsify for a fixed (H, W) and batch size B with the output, the workspace and a device state
    (seed_lo, seed_hi, draw) kept between calls. With advance (the default) one in-place torch op adds 1
    to the draw after the library call, so consecutive calls, and the replays of a captured call, give
    new samples: replay k of a graph captured at draw d equals sparsify(..., draw=d + k). reset(draw)
    rewinds. options: sparsify's keyword arguments (floor, noise_frac, noise_amp, key_mask, keep, ...).
    Returns the kept tensors, overwritten by the next call."""

    def __init__(self, size, B=1, seed=0, draw=0, advance=True, **options):
        self.size, self.B = (int(size[0]), int(size[1])), int(B)
        self.seed, self.draw0, self.advance = int(seed), int(draw), bool(advance)
        for k in ("seed", "draw", "state", "out"):
            if k in options:
                raise TypeError(f"{_PREFIX}: Sparsifier takes no option {k!r}")
        self.options = options
        self.state, self._out = None, None

    def _prepare(self, device):
        if self.state is None or self.state.device != device:
            H, W = self.size
            self.state = make_state(self.seed, self.draw0, device)
            self._out = {"depth": torch.empty(self.B, 1, H, W, device=device),
                         "kept": torch.empty(self.B, dtype=torch.int32, device=device),
                         "workspace": torch.empty(workspace_bytes(self.B, H, W), dtype=torch.uint8, device=device)}

    def reset(self, draw=None):
        """Set the device draw counter (default: the constructor's) with one asynchronous copy."""
        if self.state is not None:
            words = state_words(self.seed, self.draw0 if draw is None else draw)
            self.state.copy_(torch.tensor(words, dtype=torch.int32).pin_memory(), non_blocking=True)
        elif draw is not None:
            self.draw0 = int(draw)

    def __call__(self, depth, n=None, *, mask=None, return_kept=False):
        if torch.is_tensor(depth) and depth.is_cuda:
            self._prepare(depth.device)
        r = sparsify(depth, n, mask=mask, state=self.state, return_kept=return_kept, out=self._out, **self.options)
        if self.advance:
            self.state[2:].add_(1)
        return r


class SparsifyBatch:
    """The reference's NYU sparse input (DataLoader_NYU.preprocess_depth) as a batch-dict stage for
    data.DevicePrefetcher(..., keys=(..., "mask", "n_keep"), ingest=SparsifyBatch(...)) over
    DataLoader_NYU(sparse="device") batches: batch['depth'] (the cropped ground truth) is replaced by
      'mask' in the batch     the depth where the mask is non-zero (mode ALL with the mask)
      'n_keep' in the batch   n_keep[b] random pixels of all H * W, as the reference zeroes as many random
                              pixels as the mask has zeros (COUNT_DEV with floor=None)
    with, add_noise, +-10 % noise on a tenth of the kept pixels (Bernoulli per pixel; the reference
    perturbs an exact count). 'mask' and 'n_keep' leave the batch, then chain (frames.Ingest(), ...) is
    called on it. The draw advances by one per batch; the state lives on the device."""

    def __init__(self, seed=0, add_noise=False, chain=None):
        self.seed, self.add_noise, self.chain = int(seed), bool(add_noise), chain
        self.state = None

    def __call__(self, batch):
        depth = batch["depth"]
        if self.state is None or self.state.device != depth.device:
            self.state = make_state(self.seed, 0, depth.device)
        noise = {"noise_frac": 0.1, "noise_amp": 0.1} if self.add_noise else {}
        batch = dict(batch)
        if "mask" in batch:
            batch["depth"] = sparsify(depth, mask=batch.pop("mask"), floor=None, state=self.state, **noise)
            batch.pop("n_keep", None)
        elif "n_keep" in batch:
            batch["depth"] = sparsify(depth, batch.pop("n_keep").to(torch.int32), floor=None, state=self.state, **noise)
        else:
            raise KeyError(f"{_PREFIX}: the batch carries neither 'mask' nor 'n_keep' (DataLoader_NYU(sparse='device'))")
        self.state[2:].add_(1)
        return self.chain(batch) if self.chain is not None else batch
