"""Depth-completion evaluation figures on device: the KITTI completion benchmark's MAE / RMSE (mm)
and iMAE / iRMSE (1/km), and the NYU convention's REL, squared REL, RMSE(log) and delta < 1.25^k.

The reference reports only its validation loss (utils.py:18-40). Here one libnconv call
(nconv_depth_metrics, csrc/metrics.hip: two launches, no host synchronisation) reduces a batch to
twelve raw sums per image, in the fixed order of include/nconv.h:

    0 n_valid   1 n_pos   2 sum|e|   3 sum e^2   4 sum|e|/g   5 sum e^2/g   6 sum|1/p - 1/g|
    7 sum(1/p - 1/g)^2    8 sum(ln p - ln g)^2   9-11 #{max(p/g, g/p) < 1.25, 1.25^2, 1.25^3}

with g the target, p the (clamped) prediction, e = p - g, over the valid pixels (g > 0 and inside
[gt_min, gt_max]) for 0 and 2-5 and over the valid pixels with p > 0 for 1 and 6-11.

  depth_metric_sums   the (B, 12) float64 sums of one batch (device only: there is no PyTorch path)
  DepthMetrics        a running total over batches; update() never synchronises and is capturable
                      in a hipGraph; compute() is the one synchronisation. compute / merge /
                      from_sums / per_image are plain tensor arithmetic and work on CPU tensors.
"""
import torch
import torch.distributed as dist

from . import _views

NSUMS = 12
# figures over the valid pixels (mean over n) and over the positive ones (mean over n_pos)
FIGURES = ("mae", "rmse", "rel", "sqrel", "imae", "irmse", "rmse_log", "d1", "d2", "d3")


def _bound(v, name):
    """A bound as the C ABI takes it: None or 0 = absent."""
    if v is None:
        return 0.0
    v = float(v)
    if not v >= 0.0:
        raise ValueError(f"{name} must be >= 0 (0 or None: no bound), got {v}")
    return v


def _bounds(gt_min, gt_max, clamp):
    lo, hi = (None, None) if clamp is None else clamp
    b = (_bound(gt_min, "gt_min"), _bound(gt_max, "gt_max"), _bound(lo, "clamp[0]"), _bound(hi, "clamp[1]"))
    if b[0] and b[1] and b[0] > b[1]:
        raise ValueError(f"gt_min {b[0]} > gt_max {b[1]}")
    if b[2] and b[3] and b[2] > b[3]:
        raise ValueError(f"clamp {b[2]} > {b[3]}")
    return b


def _operand(x, what):
    """(B, H, W, image stride, row stride) of an fp32 device operand."""
    if torch.is_tensor(x):  # a tensor's device is checked before its dtype
        _views.on_device(x, what, "depth metrics", "the sums are computed by libnconv")
    _views.require_tensor(x, what, (torch.float32,), "depth metrics", expected="float32")
    return _views.plane_view(x, what, "depth metrics")


def _launch(pred, gt, bounds, want_sums, accum):
    from . import _lib
    B, H, W, pbs, prs = _operand(pred, "pred")
    Bg, Hg, Wg, gbs, grs = _operand(gt, "gt")
    if (B, H, W) != (Bg, Hg, Wg):
        raise ValueError(f"depth metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    if pred.device != gt.device:
        raise RuntimeError(f"depth metrics: pred on {pred.device}, gt on {gt.device}")
    if accum is not None:
        if not (torch.is_tensor(accum) and accum.dtype == torch.float64 and accum.shape == (NSUMS,)
                and accum.is_contiguous()):
            raise TypeError("depth metrics: accum must be a contiguous (12,) float64 tensor")
        if accum.device != pred.device:
            raise RuntimeError(f"depth metrics: accum on {accum.device}, pred on {pred.device}")
    lib = _lib.lib()
    nbytes = lib.nconv_depth_metrics_workspace_bytes(B, H, W)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=pred.device)
    sums = torch.empty((B, NSUMS), dtype=torch.float64, device=pred.device) if want_sums else None
    rc = lib.nconv_depth_metrics(_lib.ptr(pred), pbs, prs, _lib.ptr(gt), gbs, grs, B, H, W, *bounds,
                                 _lib.ptr(sums), _lib.ptr(accum), _lib.ptr(ws), nbytes,
                                 _lib.stream_handle(pred.device))
    _lib.check(rc, "nconv_depth_metrics")
    return sums


def depth_metric_sums(pred, gt, *, gt_min=None, gt_max=None, clamp=None, accum=None):
    """The twelve raw sums of each image of a batch: (B, 12) float64 on pred's device.

    pred, gt: fp32 device tensors of the same shape, (H, W), (1, H, W) or (B, 1, H, W), rows of unit
    stride (pred may be a cropped view, e.g. DNET's output). gt_min / gt_max: validity window of
    the target; clamp = (lo, hi): the prediction is clamped into it first; None or 0 = no bound.
    accum: an optional (12,) float64 device tensor increased by the images' rows in order."""
    return _launch(pred, gt, _bounds(gt_min, gt_max, clamp), True, accum)


def _figures(sums, unit_m):
    """{figure: float64 tensor (...)} from sums (..., 12); an empty denominator gives nan."""
    s = sums.to(torch.float64)
    if s.shape[-1] != NSUMS:
        raise ValueError(f"depth metrics: expected (..., {NSUMS}) sums, got {tuple(sums.shape)}")
    unit_m = float(unit_m)
    n, npos = s[..., 0], s[..., 1]
    nan = torch.full_like(n, float("nan"))

    def mean(x, d):
        return torch.where(d > 0, x / torch.where(d > 0, d, torch.ones_like(d)), nan)

    f = {"n": n, "n_pos": npos,
         "mae": mean(s[..., 2], n), "rmse": mean(s[..., 3], n).sqrt(),
         "rel": mean(s[..., 4], n), "sqrel": mean(s[..., 5], n),
         "imae": mean(s[..., 6], npos), "irmse": mean(s[..., 7], npos).sqrt(),
         "rmse_log": mean(s[..., 8], npos).sqrt(),
         "d1": mean(s[..., 9], npos), "d2": mean(s[..., 10], npos), "d3": mean(s[..., 11], npos)}
    # unit_m metres per tensor unit: errors in mm, inverse errors in 1/km
    f["mae_mm"] = f["mae"] * (1000.0 * unit_m)
    f["rmse_mm"] = f["rmse"] * (1000.0 * unit_m)
    f["imae_1/km"] = f["imae"] * (1000.0 / unit_m)
    f["irmse_1/km"] = f["irmse"] * (1000.0 / unit_m)
    return f


class DepthMetrics:
    """Running depth-completion metrics over batches (a validation loop's accumulator).

        m = DepthMetrics(gt_max=80.0, clamp=(0.9, 80.0))
        for batch in loader: m.update(model(batch["depth"]), batch["gt"])     # no synchronisation
        m.all_reduce()                                                        # data-parallel runs
        print(m.compute(unit_m=1.0))                                          # the one synchronisation

    state is the (12,) float64 total of the raw sums (see the module docstring)."""

    def __init__(self, gt_min=None, gt_max=None, clamp=None, device=None):
        self.bounds = _bounds(gt_min, gt_max, clamp)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.state = torch.zeros(NSUMS, dtype=torch.float64, device=device)

    def update(self, pred, gt):
        """state += the sums of this batch (nconv_depth_metrics on the current stream)."""
        _launch(pred, gt, self.bounds, False, self.state)
        return self

    def reset(self):
        self.state.zero_()
        return self

    def merge(self, other):
        self.state += other.state.to(self.state.device)
        return self

    def all_reduce(self, group=None):
        """Sum state over the process group (every rank ends with the whole validation set's sums)."""
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    @classmethod
    def from_sums(cls, sums, gt_min=None, gt_max=None, clamp=None):
        """An object whose state is the total of sums, (12,) or (..., 12), on the tensor's device."""
        if sums.shape[-1] != NSUMS:
            raise ValueError(f"depth metrics: expected (..., {NSUMS}) sums, got {tuple(sums.shape)}")
        m = cls(gt_min, gt_max, clamp, device=sums.device)
        m.state += sums.detach().to(torch.float64).reshape(-1, NSUMS).sum(0)
        return m

    def compute(self, unit_m=1.0):
        """{figure: float}: n, n_pos, mae, rmse, rel, sqrel (means over n), imae, irmse, rmse_log,
        d1, d2, d3 (means over n_pos) in the tensors' units, and mae_mm, rmse_mm, imae_1/km,
        irmse_1/km for tensors of unit_m metres per unit. nan where the denominator is empty."""
        return {k: float(v) for k, v in _figures(self.state.cpu(), unit_m).items()}

    @staticmethod
    def per_image(sums, unit_m=1.0):
        """compute()'s figures for each row of a (B, 12) tensor of sums: {figure: list of B floats}."""
        if sums.dim() != 2:
            raise ValueError(f"depth metrics: expected (B, {NSUMS}) sums, got {tuple(sums.shape)}")
        return {k: v.tolist() for k, v in _figures(sums.detach().cpu(), unit_m).items()}
