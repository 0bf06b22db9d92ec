"""Shared cases, operands and float64 budgets of the dense autograd function's parity test
(tests/test_gpu_dense_train.py::test_dense_conv_fn_forward_backward), used by the GPU test, by
tools/bwd_kappa.py and by the CPU checks of tests/test_bwd_bound_cpu.py."""
import torch
import torch.nn.functional as F

# kind (0 3x3, 1 1x1, 2 ConvTranspose 4x4 s2), stride, C0, C1 (second source), Cout, H, W, relu, bias
CASES = [
    (0, 1, 32, 32, 32, 19, 45, True, True),     # ConvBlock fuse_conv1 on cat(rgb_feat, depth_feat)
    (0, 1, 64, 64, 64, 12, 40, False, False),   # UpCat conv 128 -> 64 (BatchNorm follows)
    (0, 1, 1, 0, 32, 13, 33, True, True),       # depth_conv 1 -> 32
    (0, 1, 64, 0, 64, 9, 70, True, True),       # rgb_conv 64 -> 64
    (0, 2, 32, 0, 64, 17, 43, False, True),     # encoder 3x3 s2, odd sizes (cropped transposed dgrad)
    (0, 2, 64, 0, 64, 16, 40, False, True),     # encoder 3x3 s2, even sizes
    (0, 1, 3, 0, 32, 16, 40, False, True),      # encoder0 3 -> 32
    (1, 1, 3, 0, 32, 11, 35, False, False),     # encoder0 shortcut 1x1
    (1, 2, 64, 0, 64, 15, 41, False, False),    # shortcut 1x1 s2, odd sizes
    (2, 2, 1, 64, 64, 7, 20, False, False),     # Basic2dTrans on cat(depth, features): 65 -> 64
    (2, 2, 1, 32, 32, 9, 19, False, True),      # 33 -> 32, with bias
    (0, 1, 32, 0, 1, 14, 37, False, False),     # 3x3 to one channel through the generic tiles
    (0, 1, 1, 32, 32, 11, 37, True, True),      # 33 input channels, the depth channel first (a chunk
                                                #   straddling the sources; two weight-gradient n-groups)
    (0, 2, 33, 0, 64, 13, 29, False, True),     # stride 2, 33 input channels, odd sizes
]

FWD_REL = 1e-6  # the project's forward figure: |gpu - ref| <= 1e-6 * (|x| (*) |w| + |b|), DESIGN 2

# Seed offsets of the ReLU cases, chosen (tests/test_bwd_bound_cpu.py checks them without a GPU) so
# that no float64 pre-activation lies within the forward bound of zero: the GPU's ReLU decision is
# then the reference's wherever the forward is within its bound. {case index: offset}
SEED_OFFSET = {0: 100000, 3: 100000}


def case_id(case):
    kind, stride, c0, c1, cout, H, W, relu, bias = case
    return f"k{kind}s{stride}_{c0}+{c1}to{cout}_{H}x{W}" + ("_relu" if relu else "") + ("_bias" if bias else "")


def case_seed(case):
    kind, stride, c0, c1, cout, H, W, relu, bias = case
    return kind * 1000 + c0 * 10 + cout + H + SEED_OFFSET.get(CASES.index(case), 0)


def r32(t):
    return None if t is None else t.float().double()


def _conv(case, x, w, b):
    kind, stride = case[0], case[1]
    if kind == 2:
        return F.conv_transpose2d(x, w, b, 2, 1)
    return F.conv2d(x, w, b, stride, w.shape[-1] // 2)


class DenseProblem:
    """fp32-rounded float64 operands (x0, x1, w, b), the output gradient gy, and the float64
    reference of one case."""

    def __init__(self, case, seed=None):
        kind, stride, c0, c1, cout, H, W, relu, bias = case
        self.case, self.relu = case, relu
        g = torch.Generator().manual_seed(case_seed(case) if seed is None else seed)
        B, cin = 2, c0 + c1
        x0 = torch.randn(B, c0, H, W, generator=g, dtype=torch.float64)
        x1 = torch.randn(B, c1, H, W, generator=g, dtype=torch.float64) if c1 else None
        if kind == 2:
            w = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64) * 0.1
        else:
            k = 3 if kind == 0 else 1
            w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * 0.1
        b = torch.randn(cout, generator=g, dtype=torch.float64) if bias else None
        self.ops = [r32(t) for t in (x0, x1, w, b)]
        with torch.no_grad():
            shape = _conv(case, self._x(self.ops), self.ops[2], None).shape
        self.gy = r32(torch.randn(shape, generator=g, dtype=torch.float64))

    @staticmethod
    def _x(ops):
        return torch.cat([ops[0], ops[1]], 1) if ops[1] is not None else ops[0]

    def run(self, dtype=torch.float64):
        """(pre-activation, output, [grad x0, x1, w, b]) of the plain op sequence in dtype, the ReLU
        decided by this run's own pre-activation; everything returned as float64."""
        leaves = [t.to(dtype).clone().requires_grad_(True) if t is not None else None for t in self.ops]
        pre = _conv(self.case, self._x(leaves), leaves[2], leaves[3])
        y = torch.relu(pre) if self.relu else pre
        y.backward(self.gy.to(dtype))
        return (pre.detach().double(), y.detach().double(),
                [None if t is None else t.grad.double() for t in leaves])

    def forward_bound(self):
        """1e-6 * (|x| (*) |w| + |b|) per output element."""
        x, w, b = self._x(self.ops), self.ops[2], self.ops[3]
        with torch.no_grad():
            return FWD_REL * _conv(self.case, x.abs(), w.abs(), None if b is None else b.abs())

    def majorants(self, mask):
        """(|g| (*)^T |w| for x0 and x1, wgrad(|x|, |g|), sum |g|) with g = gy * mask."""
        g = (self.gy * mask).abs()
        x = self._x(self.ops).abs().requires_grad_(True)
        w = self.ops[2].abs().requires_grad_(True)
        a_x, a_w = torch.autograd.grad(_conv(self.case, x, w, None), [x, w], g)
        c0 = self.ops[0].shape[1]
        a_x1 = a_x[:, c0:] if self.ops[1] is not None else None
        return [a_x[:, :c0], a_x1, a_w, g.sum((0, 2, 3)) if self.ops[3] is not None else None]

    def relu_margin_violations(self):
        """Pre-activations of the float64 reference within the forward bound of zero."""
        pre, _, _ = self.run()
        return int((pre.abs() <= self.forward_bound()).sum()) if self.relu else 0

    def kappa_ref(self):
        """Weight / bias gradient of the float32 run against the float64 one, relative to the
        majorant. The float32 run's ReLU takes the float64 decision (the margin condition makes
        them equal)."""
        pre, _, ref = self.run()
        pre32, _, g32 = self.run(torch.float32)
        mask = (pre > 0) if self.relu else torch.ones_like(pre, dtype=torch.bool)
        assert not self.relu or torch.equal(pre32 > 0, mask)
        A = self.majorants(mask)
        return {lab: float(((g - r).abs() / (a + 1e-30)).max())
                for lab, r, g, a in zip(("g_x0", "g_x1", "g_w", "g_b"), ref, g32, A) if r is not None and lab[2] in "wb"}
