"""Training augmentation of a batch on the device (nconv_frame_augment, csrc/augment.hip): a random crop
window and a horizontal flip per image, applied alike to the RGB, the sparse depth, the ground truth, a
spare plane and a mask, the intrinsics rewritten to match, and photometric jitter on the RGB. One launch
per batch, no host synchronisation, a function of (inputs, seed, draw) alone.

    augment     one call
    Augmenter   the same with its outputs and a device-side (seed, draw) state kept between calls, so a
                call can be captured with torch.cuda.graph and every replay draws a new augmentation
    Augment     a batch-dict stage for data.DevicePrefetcher:
                SparsifyBatch(chain=Augment((h, w), chain=Ingest()))

The rule is include/nconv.h's; tests/augment_cases.py restates it in numpy and the GPU tests hold the
kernel to it bit for bit. The jitter is not torchvision's ColorJitter: brightness and three colour gains
multiply, contrast pivots on a constant (127.5) and not on the image mean, and there is no hue.
"""
import ctypes
import math

import torch

from . import _views
from .sparsify import make_state, state_words

_PREFIX = "augment"
_DOING = "the augmentation runs in libnconv"
_PLANES = ("depth", "gt", "extra")  # the descriptor's plane[0..2]


def flip_threshold(p):
    """floor(p * 2^32) in double, clamped to [0, 2^32]: an image is flipped iff its third Philox word is
    below it."""
    f = float(p)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"{_PREFIX}: flip = {p} outside [0, 1]")
    return min(max(int(math.floor(f * 4294967296.0)), 0), 1 << 32)


def _modes(crop):
    from . import _lib
    if isinstance(crop, str):
        crop = (crop, crop)
    try:
        my, mx = crop
        return _lib.AUGMENT_CROPS[my], _lib.AUGMENT_CROPS[mx]
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"{_PREFIX}: crop = {crop!r}; a mode or a (rows, columns) pair of modes out of "
                         f"{sorted(_lib.AUGMENT_CROPS)}") from None


def _amplitude(v, what):
    f = float(v)
    if not 0.0 <= f <= 1.0:  # a NaN fails too
        raise ValueError(f"{_PREFIX}: {what} = {v} outside [0, 1]")
    return f


def _rgb_view(x):
    """(B, H, W, image, channel, row stride in elements) of a (3, H, W) or (B, 3, H, W) view."""
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[1] != 3 or x.stride(3) != 1:
        raise ValueError(f"{_PREFIX}: rgb of shape {tuple(x.shape)} / strides {x.stride()} is not a (3, H, W) or "
                         "(B, 3, H, W) set of unit-stride rows")
    return x.shape[0], x.shape[2], x.shape[3], x.stride(0), x.stride(1), x.stride(2)


def augment(rgb=None, depth=None, gt=None, extra=None, mask=None, k=None, *, size, state=None, seed=0, draw=0,
            crop=("random", "random"), flip=0.5, brightness=0.0, contrast=0.0, color=0.0, pivot=127.5,
            rgb_max=255.0, return_params=False, out=None, src_size=None):
    """Crop, flip and jitter a batch: a dict with an entry for every source given, under its name.

    rgb: fp32 (3, H, W) or (B, 3, H, W); depth, gt, extra: fp32 (H, W), (1, H, W) or (B, 1, H, W); mask:
    uint8, shaped like a plane, (H, W) or (1, H, W) beside B > 1 meaning one mask for the batch; k: fp32
    (B, 3, 3) (or (3, 3) for one image). All on one device, any views of unit-stride rows, all of one
    source size (H, W) and batch B. size = (h, w), no larger than the source: the outputs are
    (B, 3, h, w), (B, 1, h, w) and (B, 3, 3), contiguous. src_size = (H, W) is needed only where k is the
    one source (the window depends on it); beside images it must be theirs.
    crop: a mode or a (rows, columns) pair out of 'random', 'center', 'min' (the first rows / columns) and
    'max' (the last: KITTI keeps the bottom rows). flip: the probability of a horizontal flip; k's cx is
    mirrored with it. brightness, contrast, color: jitter amplitudes in [0, 1] on the rgb, all zero: the
    rgb is copied bit for bit. With v * g_b * gain_c, then (.. - pivot) * g_c + pivot, clamped to
    [0, rgb_max], every gain uniform in 1 +- its amplitude; this is not torchvision's ColorJitter.
    The draw is Philox4x32-10 keyed by the 64-bit seed at counter (image, 0 / 1, draw, 1): `state`, a (3,)
    int32 device tensor (seed_lo, seed_hi, draw), replaces seed and draw and is only read; without it the
    three words are uploaded from pinned memory, with no synchronisation.
    return_params: also 'params' (B, 4) int32 {y0, x0, flip, 0} and 'gains' (B, 5) fp32
    {g_b, g_c, gain_r0, gain_r1, gain_r2}. out: an optional dict of preallocated outputs under the same
    names; none may overlap a source. One kernel launch, no host synchronisation, and no allocation when
    out is complete and state is given: capturable with torch.cuda.graph."""
    from . import _lib
    srcs = {"rgb": rgb, "depth": depth, "gt": gt, "extra": extra, "mask": mask, "k": k}
    given = {n: t for n, t in srcs.items() if t is not None}
    if not given:
        raise ValueError(f"{_PREFIX}: no source given (rgb, depth, gt, extra, mask or k)")
    for n, t in given.items():
        _views.require_tensor(t, n, (torch.uint8,) if n == "mask" else (torch.float32,), _PREFIX)
    geo = {}  # name -> (B, H, W)
    d = _lib.NconvFrameAugment()
    if rgb is not None:
        B, H, W, d.rgb_image_stride, d.rgb_channel_stride, d.rgb_row_stride = _rgb_view(rgb)
        geo["rgb"] = (B, H, W)
    for i, n in enumerate(_PLANES):
        if n in given:
            B, H, W, d.plane[i].image_stride, d.plane[i].row_stride = _views.plane_view(given[n], n, _PREFIX)
            geo[n] = (B, H, W)
    if mask is not None:
        mB, H, W, mbs, d.mask_row_stride = _views.plane_view(mask, "mask", _PREFIX)
        geo["mask"] = (mB, H, W)
    if k is not None:
        if tuple(k.shape[-2:]) != (3, 3) or k.dim() not in (2, 3) or not k.is_contiguous():
            raise ValueError(f"{_PREFIX}: k must be a contiguous (B, 3, 3) or (3, 3) tensor, got {tuple(k.shape)}")
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{_PREFIX}: size = {size!r} is not an (h, w) pair") from None
    ref = next((n for n in geo if n != "mask"), None)
    if ref is not None:
        B = geo[ref][0]
    else:  # a mask and / or k alone
        B = geo["mask"][0] if k is None else (1 if k.dim() == 2 else k.shape[0])
    if src_size is not None:
        H, W = (int(v) for v in src_size)
    elif geo:
        H, W = next(iter(geo.values()))[1:]
    else:
        raise ValueError(f"{_PREFIX}: k alone does not tell the source size: pass src_size=(H, W)")
    for n, g in geo.items():
        if g[1:] != (H, W) or not (g[0] == B or (n == "mask" and g[0] == 1)):
            raise ValueError(f"{_PREFIX}: {n} of shape {tuple(given[n].shape)} does not match "
                             f"{ref or 'the rest'} (batch {B}, source size {H} x {W})")
    if k is not None and (1 if k.dim() == 2 else k.shape[0]) != B:
        raise ValueError(f"{_PREFIX}: k of shape {tuple(k.shape)} does not match the batch of {B}")
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"{_PREFIX}: size = {(h, w)} must be at least (1, 1) and no larger than the source {(H, W)}")
    d.mode_y, d.mode_x = _modes(crop)
    d.flip_threshold = flip_threshold(flip)
    d.brightness, d.contrast, d.color = (_amplitude(v, n) for v, n in ((brightness, "brightness"),
                                                                       (contrast, "contrast"), (color, "color")))
    pivot, rgb_max = float(pivot), float(rgb_max)
    if pivot != pivot or not rgb_max >= 0.0:
        raise ValueError(f"{_PREFIX}: pivot = {pivot} / rgb_max = {rgb_max}: a NaN, or a negative rgb_max")
    d.pivot, d.rgb_max = pivot, rgb_max
    if state is not None:
        _views.require_tensor(state, "state", (torch.int32,), _PREFIX)
        if tuple(state.shape) != (3,) or not state.is_contiguous():
            raise ValueError(f"{_PREFIX}: state must be a contiguous (3,) vector, got {tuple(state.shape)}")
        given["state"] = state
    first = next(iter(given))
    dev = given[first].device
    for n, t in given.items():
        _views.on_device(t, n, _PREFIX, _DOING)
        if t.device != dev:
            raise RuntimeError(f"{_PREFIX}: {n} on {t.device}, {first} on {dev}")
    res = {}
    for n in srcs:
        if n in given:
            shape = (B, 3, 3) if n == "k" else (B, 3 if n == "rgb" else 1, h, w)
            res[n] = _views.output(out, n, shape, torch.uint8 if n == "mask" else torch.float32, dev, _PREFIX, source=first)
    want_report = return_params or (out is not None and ("params" in out or "gains" in out))
    if want_report:
        res["params"] = _views.output(out, "params", (B, 4), torch.int32, dev, _PREFIX, source=first)
        res["gains"] = _views.output(out, "gains", (B, 5), torch.float32, dev, _PREFIX, source=first)
    if state is None:
        state = make_state(seed, draw, dev)
    d.B, d.H, d.W, d.h, d.w = B, H, W, h, w
    d.state = state.data_ptr()
    if rgb is not None:
        d.rgb, d.rgb_out = rgb.data_ptr(), res["rgb"].data_ptr()
    for i, n in enumerate(_PLANES):
        if n in given:
            d.plane[i].src, d.plane[i].out = given[n].data_ptr(), res[n].data_ptr()
    if mask is not None:
        d.mask, d.mask_out = mask.data_ptr(), res["mask"].data_ptr()
        d.mask_image_stride = mbs if geo["mask"][0] == B and B > 1 else 0
    if k is not None:
        d.k, d.k_out = k.data_ptr(), res["k"].data_ptr()
    if want_report:
        d.params, d.gains = res["params"].data_ptr(), res["gains"].data_ptr()
    rc = _lib.lib().nconv_frame_augment(ctypes.byref(d), _lib.stream_handle(dev))
    _lib.check(rc, "nconv_frame_augment")
    return res


class Augmenter:
    """augment for a fixed source size, output size and batch size B, with the outputs and a device
    state (seed_lo, seed_hi, draw) kept between calls. With advance (the default) one in-place torch op
    adds 1 to the draw after the library call, so consecutive calls, and the replays of a captured call,
    give new augmentations: replay r of a graph captured at draw d equals augment(..., draw=d + r).
    reset(draw) rewinds. options: augment's keyword arguments (crop, flip, brightness, ...). Returns
    augment's dict with 'params' and 'gains', the tensors overwritten by the next call."""

    def __init__(self, src_size, size, B=1, seed=0, draw=0, advance=True, **options):
        self.src_size, self.size = (int(src_size[0]), int(src_size[1])), (int(size[0]), int(size[1]))
        self.B, self.seed, self.draw0, self.advance = int(B), int(seed), int(draw), bool(advance)
        for key in ("seed", "draw", "state", "out", "size", "src_size", "return_params"):
            if key in options:
                raise TypeError(f"{_PREFIX}: Augmenter takes no option {key!r}")
        if not (1 <= self.size[0] <= self.src_size[0] and 1 <= self.size[1] <= self.src_size[1]):
            raise ValueError(f"{_PREFIX}: size = {self.size} must be at least (1, 1) and no larger than the source "
                             f"{self.src_size}")
        self.options = options
        self.state, self._out = None, None

    def _prepare(self, device, names):
        if self.state is None or self.state.device != device:
            self.state = make_state(self.seed, self.draw0, device)
            self._out = {"params": torch.empty(self.B, 4, dtype=torch.int32, device=device),
                         "gains": torch.empty(self.B, 5, device=device)}
        h, w = self.size
        for n in names:
            if n not in self._out:
                shape = (self.B, 3, 3) if n == "k" else (self.B, 3 if n == "rgb" else 1, h, w)
                self._out[n] = torch.empty(shape, dtype=torch.uint8 if n == "mask" else torch.float32, device=device)

    def reset(self, draw=None):
        """Set the device draw counter (default: the constructor's) with one asynchronous copy."""
        if self.state is not None:
            words = state_words(self.seed, self.draw0 if draw is None else draw)
            self.state.copy_(torch.tensor(words, dtype=torch.int32).pin_memory(), non_blocking=True)
        elif draw is not None:
            self.draw0 = int(draw)

    def __call__(self, rgb=None, depth=None, gt=None, extra=None, mask=None, k=None):
        srcs = {"rgb": rgb, "depth": depth, "gt": gt, "extra": extra, "mask": mask, "k": k}
        given = {n: t for n, t in srcs.items() if t is not None}
        first = next(iter(given.values()), None)
        if torch.is_tensor(first) and first.is_cuda:
            self._prepare(first.device, given)
        r = augment(**srcs, size=self.size, src_size=self.src_size, state=self.state, out=self._out,
                    return_params=True, **self.options)
        if self.advance:
            self.state[2:].add_(1)
        return r


class Augment:
    """augment as a batch-dict stage for data.DevicePrefetcher(..., ingest=...): chain (frames.Ingest(),
    ...) runs first, then the 'rgb', 'depth', 'gt', 'mask' and 'k' the batch holds are replaced by their
    cropped, flipped (and, the rgb, jittered) versions of size (h, w); every other entry passes through.
    The draw advances by one per batch; the state lives on the device. return_params=True adds 'params'
    and 'gains' to the batch. A batch that carries 'n_keep' (DataLoader_NYU(sparse="device") without a
    mask) is refused when the output is smaller than the source: the count describes the uncropped
    image. Sample first, SparsifyBatch(chain=Augment((h, w), chain=Ingest())), or use the 'mask' form.
    options: augment's keyword arguments (crop, flip, brightness, contrast, color, ...)."""

    KEYS = ("rgb", "depth", "gt", "mask", "k")

    def __init__(self, size, seed=0, chain=None, return_params=False, **options):
        self.size, self.seed, self.chain = (int(size[0]), int(size[1])), int(seed), chain
        self.return_params = bool(return_params)
        for key in ("draw", "state", "out"):
            if key in options:
                raise TypeError(f"{_PREFIX}: Augment takes no option {key!r}")
        self.options = options
        self.state = None

    def __call__(self, batch):
        if self.chain is not None:
            batch = self.chain(batch)
        srcs = {n: batch[n] for n in self.KEYS if torch.is_tensor(batch.get(n))}
        if not srcs:
            raise KeyError(f"{_PREFIX}: the batch carries none of {self.KEYS}")
        if "n_keep" in batch:
            H, W = next((t.shape[-2:] for n, t in srcs.items() if n != "k"), self.size)
            if self.size[0] < H or self.size[1] < W:
                raise ValueError(f"{_PREFIX}: the batch carries 'n_keep', a count over the uncropped {H} x {W} image, "
                                 f"and the output is {self.size[0]} x {self.size[1]}: the count no longer describes "
                                 "the crop. Use the 'mask' form of DataLoader_NYU(sparse='device'), or sample before "
                                 "augmenting: SparsifyBatch(chain=Augment(...))")
        dev = next(iter(srcs.values())).device
        if dev.type == "cuda" and (self.state is None or self.state.device != dev):
            self.state = make_state(self.seed, 0, dev)
        r = augment(**srcs, size=self.size, state=self.state, return_params=self.return_params, **self.options)
        self.state[2:].add_(1)  # (a CPU batch was refused above)
        out = dict(batch)
        out.update(r)
        return out
