"""GPU parity of the whole DNET / SETP1_NCONV path against the oracle (dnet_forward = restated
models/step1.py:51-94) — forward at several sizes and both crops, training-mode EnforcePos drift,
and the fwd+bwd gradients of a step-1 training loss.

Tolerances: forward elementwise |gpu-ref| <= 1e-4*|ref| + 1e-6 (fp32 kernels vs fp64 oracle: the
north star's 1e-4 relative; measured in round 5 every element of every case, bf16x3 included, lies
below 1e-4*|ref| - 1e-6, profiles/r5_dnet_output_error_margins.tsv; the absolute term was 1e-4);
gradients normwise max|gpu-ref|/max|ref| <= 1e-3.
"""
import os
import sys

import pytest
import torch

from oracle import nconv_ref as R

pytestmark = pytest.mark.gpu


def sparse_depth(g, B, H, W, density=0.05, dtype=torch.float32):
    d = torch.rand(B, 1, H, W, generator=g, dtype=dtype) * 79 + 1
    return d * (torch.rand(B, 1, H, W, generator=g, dtype=dtype) < density)


def make_net(nconv_amd, crop, dev):
    torch.manual_seed(0)
    net = nconv_amd.SETP1_NCONV(crop=crop).to(dev)
    # one training-mode forward: EnforcePos makes the weights positive (what training produces)
    net.train()
    with torch.no_grad():
        net(torch.zeros(1, 1, 32, 32, device=dev))
    net.eval()
    return net


def _report(what, err, ref):
    """(tolerance study) NCONV_TOL_REPORT=path appends the absolute term each comparison needs
    beside 1e-4 relative."""
    rep = os.environ.get("NCONV_TOL_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write(f"{what}\t{err.max().item():.3e}\t{(err - 1e-4 * ref.abs()).max().item():.3e}\t"
                     f"{ref.abs().max().item():.3e}\n")


def oracle_params(net):
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    return R.dnet_params_from_state_dict(sd)


@pytest.mark.parametrize("crop", ["literal", "generalized"])
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (2, 50, 70), (1, 33, 47), (1, 352, 1216)])
def test_dnet_eval_forward(nconv_amd, gpu, crop, B, H, W):
    net = make_net(nconv_amd, crop, gpu)
    g = torch.Generator().manual_seed(H * 1000 + W)
    S = sparse_depth(g, B, H, W)
    with torch.no_grad():
        out = net(S.to(gpu)).double().cpu()
    ref = R.dnet_forward(S.double(), oracle_params(net), crop)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = (out - ref).abs()
    _report(f"eval {crop} {B}x{H}x{W}", err, ref)
    bound = 1e-4 * ref.abs() + 1e-6
    assert (err <= bound).all(), f"max err {err.max():.3e} ratio {(err / bound).max():.3f}"


def test_dnet_grad_path_matches_fused_tail(nconv_amd, gpu):
    """The autograd path (separate nconv6 / nconv7 + slicing) equals the fused inference tail."""
    net = make_net(nconv_amd, "literal", gpu)
    g = torch.Generator().manual_seed(7)
    S = sparse_depth(g, 2, 64, 96).to(gpu)
    with torch.no_grad():
        a = net(S)
    b = net(S.clone().requires_grad_(True)).detach()
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def _graph_has(fn, name, depth=6):
    if fn is None or depth < 0:
        return False
    if name in type(fn).__name__:
        return True
    return any(_graph_has(f, name, depth - 1) for f, _ in fn.next_functions)


@pytest.mark.parametrize("H,W", [(64, 96), (45, 67)])
def test_whole_graph_autograd_matches_per_layer(nconv_amd, gpu, H, W, monkeypatch):
    """DNETFn (one autograd node, shared-tensor gradients accumulated in the dgrad kernels) against
    one NConvLayerFn node per layer (PyTorch adds the two consumers' gradients): same kernels, so
    outputs are bitwise equal and gradients agree to fp32 round-off of the accumulation (1e-6
    relative per tensor; 1e-5 for nconv7's, fused into nconv6's backward); the input gradient of S
    too."""
    g = torch.Generator().manual_seed(21)
    S = sparse_depth(g, 2, H, W).to(gpu)
    gt = (torch.rand(2, 1, H, W, generator=g) * 80).to(gpu)
    # the same forward kernels in both (the fused head's composed D2 rounds differently; it is
    # checked against the oracle in test_dnet_train_gradients and bitwise in the layer tests)
    monkeypatch.setattr(sys.modules[nconv_amd.DNET.__module__], "FUSE_HEAD_FWD", False)
    monkeypatch.setattr(sys.modules[nconv_amd.DNET.__module__], "FUSE_TAIL_FWD", False)
    res = []
    for whole in (True, False):
        net = make_net(nconv_amd, "generalized", gpu)
        net.d_net.whole_graph_autograd = whole
        x = S.clone().requires_grad_(True)
        out = net(x)
        assert _graph_has(out.grad_fn, "DNETFn") == whole
        nconv_amd.train.calculate_loss(out[0], gt[0], True).backward()
        res.append((out.detach(), x.grad, {k: v.grad for k, v in net.named_parameters() if v.grad is not None}))
    (oa, ga, pa), (ob, gb, pb) = res
    assert torch.equal(oa, ob)
    assert set(pa) == set(pb) and len(pa) == 18
    for k, a, b in [("S", ga, gb)] + [(k, pa[k], pb[k]) for k in pa]:
        # nconv7's weight gradient is computed inside nconv6's backward by DNETFn (a reassociated sum)
        tol = 1e-5 if k.startswith("d_net.nconv7.") else 1e-6
        assert (a - b).abs().max().item() <= tol * b.abs().max().item() + 1e-30, k


@pytest.mark.parametrize("H,W", [(64, 96), (45, 67)])
def test_materialised_pool_matches_pool_on_load(nconv_amd, gpu, H, W, monkeypatch):
    """DNETFn's exact-fp32 training graph with the 2x2 max-pools materialised (nconv_fwd_pooled
    argmax codes; pooled-sized down-layer input gradients routed into the producer's {gN, gD} by
    nconv_bwd_ex) against pooling on load with full-resolution accumulation: the same sums in the
    same order, so outputs and every gradient are bitwise equal (odd sizes: rows / columns no
    window covers get no pooled gradient in both) -- except the weight gradients the pooled graph
    computes inside a neighbour's kernel (nconv7's in nconv6's backward, nconv1's in nconv2's when S
    needs no gradient), which are the same sums reassociated (normwise 1e-5)."""
    g = torch.Generator().manual_seed(22)
    S = sparse_depth(g, 2, H, W).to(gpu)
    gt = (torch.rand(2, 1, H, W, generator=g) * 80).to(gpu)
    dnet = sys.modules[nconv_amd.DNET.__module__]
    res = []
    monkeypatch.setattr(dnet, "FUSE_TAIL_BWD", False)
    monkeypatch.setattr(dnet, "FUSE_HEAD_FWD", False)  # (the fused head's D2 rounds differently)
    monkeypatch.setattr(dnet, "FUSE_TAIL_FWD", False)
    for pooled in (True, False):
        monkeypatch.setattr(dnet, "_materialise_pool", lambda S_, v=pooled: v)
        net = make_net(nconv_amd, "generalized", gpu)
        x = S.clone().requires_grad_(True)
        out = net(x)
        nconv_amd.train.calculate_loss(out[0], gt[0], True).backward()
        res.append((out.detach(), x.grad, {k: v.grad for k, v in net.named_parameters() if v.grad is not None}))
    (oa, ga, pa), (ob, gb, pb) = res
    assert torch.equal(oa, ob) and torch.equal(ga, gb)
    assert set(pa) == set(pb) and len(pa) == 18

    def close(a, b, k):  # fused-in weight gradients (nconv1, nconv7): fp32 reassociation only
        rel = ((a - b).abs().max() / b.abs().max()).item()
        assert rel <= 1e-5, (k, rel)

    for k in pa:
        assert torch.equal(pa[k], pb[k]), k

    # S without gradient: nconv1's weight gradient fused into nconv2's input gradient (sparse
    # correlation over the depth samples, nconv_bwd_ex head): every other gradient bitwise as
    # above, nconv1's within fp32 reassociation (normwise 1e-5)
    monkeypatch.setattr(dnet, "_materialise_pool", lambda S_: True)
    net = make_net(nconv_amd, "generalized", gpu)
    out = net(S)
    nconv_amd.train.calculate_loss(out[0], gt[0], True).backward()
    pc = {k: v.grad for k, v in net.named_parameters() if v.grad is not None}
    assert torch.equal(out.detach(), oa) and set(pc) == set(pa)
    for k in pc:
        if k.startswith("d_net.nconv1."):
            close(pc[k], pa[k], k)
        else:
            assert torch.equal(pc[k], pa[k]), k

    # nconv7's backward fused into nconv6's (nconv_bwd_ex tail, exactly-2x sizes): nconv6's output
    # gradient formed in-kernel with the 1x1 dgrad's own operations; nconv7's weight gradient
    # reassociated, its bias gradient a torch sum of its output gradient (normwise 1e-5 each)
    if H % 8 == 0 and W % 8 == 0:
        monkeypatch.setattr(dnet, "FUSE_TAIL_BWD", True)
        net = make_net(nconv_amd, "generalized", gpu)
        x = S.clone().requires_grad_(True)
        out = net(x)
        nconv_amd.train.calculate_loss(out[0], gt[0], True).backward()
        pt = {k: v.grad for k, v in net.named_parameters() if v.grad is not None}
        assert torch.equal(out.detach(), oa) and set(pt) == set(pa)
        close(x.grad, ga, "S")
        for k in pt:
            close(pt[k], pa[k], k)


@pytest.mark.parametrize("H,W", [(64, 96), (48, 200)])
def test_tail_train_matches_layers(nconv_amd, gpu, H, W):
    """The training forward's fused tail (nconv_fwd_tail over nconv7's whole grid, writing nconv6's
    outputs too) against nconv6 (phase form) and nconv7 as separate launches: bitwise, the zero
    border included."""
    dnet = sys.modules[nconv_amd.DNET.__module__]
    N = nconv_amd.nconv
    net = make_net(nconv_amd, "generalized", gpu)
    d = net.d_net
    g = torch.Generator().manual_seed(H + W)
    B = 2
    x2 = (torch.rand(B, 8, H, W, generator=g) * 5).to(gpu)
    c2 = torch.rand(B, 8, H, W, generator=g).to(gpu)
    x7 = (torch.rand(B, 8, H // 2, W // 2, generator=g) * 5).to(gpu)
    c7 = torch.rand(B, 8, H // 2, W // 2, generator=g).to(gpu)
    l6, l7 = d.nconv6, d.nconv7
    s6 = torch.empty(8, device=gpu)
    s7 = torch.empty(1, device=gpu)
    N.weight_prep([l6.weight.detach(), l7.weight.detach()], [False, False], [s6, s7])
    w6 = d._phase_weights(gpu)[2]
    sp6, sp7 = l6.spec(nconv_amd._lib.UPCAT_UP_FIRST), l7.spec()
    W6, W7 = (l6.weight.detach(), l6.bias.detach(), s6), (l7.weight.detach(), l7.bias.detach(), s7)
    x8, c8, x9, c9 = dnet._tail_train(sp6, sp7, x2, c2, x7, c7, W6, W7, w6)
    r8, rc8 = N.layer_forward_raw(sp6, x2, c2, x7, c7, *W6, wphase=w6)
    r9, rc9 = N.layer_forward_raw(sp7, r8, rc8, None, None, *W7)
    torch.cuda.synchronize()
    for a, r in ((x8, r8), (c8, rc8), (x9, r9), (c9, rc9)):
        assert a.shape == r.shape and torch.equal(a, r)


def test_enforcepos_drift(nconv_amd, gpu):
    """Training-mode forward applies softplus(beta=10) to every layer's weight, once per forward."""
    torch.manual_seed(0)
    net = nconv_amd.SETP1_NCONV().to(gpu)
    before = {k: v.detach().double().cpu().clone() for k, v in net.named_parameters() if k.endswith("weight")
              and "bnorm" not in k}
    net.train()
    net(torch.zeros(1, 1, 16, 16, device=gpu))
    for k, w0 in before.items():
        w1 = dict(net.named_parameters())[k].detach().double().cpu()
        torch.testing.assert_close(w1, R.softplus_pos(w0), rtol=2e-6, atol=2e-7)
    net.eval()
    w_eval = {k: v.detach().clone() for k, v in net.named_parameters()}
    net(torch.zeros(1, 1, 16, 16, device=gpu))
    for k, v in net.named_parameters():
        assert torch.equal(v.detach(), w_eval[k]), "eval mode must not touch the weights"


@pytest.fixture(params=["fp32", "bf16x3"])
def bwd_math(request, nconv_amd, monkeypatch):
    monkeypatch.setattr(nconv_amd.nconv, "BACKWARD_MATH", nconv_amd.nconv._MATH_NAMES[request.param])
    return request.param


def _train_gradients_vs_oracle(nconv_amd, gpu, B, H, W, crop, whole_batch_loss, seed=11):
    """One step-1 training forward + calculate_loss + backward on the GPU and the same in the fp64
    oracle on the GPU's pool branch (see test_dnet_train_gradients); returns the per-tensor report
    lines (normwise errors, 'FAIL' past 1e-3) after checking the EnforcePos-drifted weights."""
    net = make_net(nconv_amd, crop, gpu)
    net.train()
    g = torch.Generator().manual_seed(seed)
    S = sparse_depth(g, B, H, W)
    params0 = oracle_params(net)  # the forward below applies EnforcePos once more
    net.d_net.capture = {}
    out = net(S.to(gpu))
    cap, net.d_net.capture = net.d_net.capture, None
    idx = {k: tuple(torch.nn.functional.max_pool2d(t, 2, 2, return_indices=True)[1].cpu() for t in v)
           for k, v in cap.items()}

    params = {n: (R.softplus_pos(w).detach().requires_grad_(True), b.detach().requires_grad_(True))
              for n, (w, b) in params0.items()}
    ref = R.dnet_forward(S.double(), params, crop, pool_idx=idx)
    gt = torch.rand(ref.shape, generator=g, dtype=torch.float64) * 80
    gt = gt * (torch.rand(ref.shape, generator=g, dtype=torch.float64) < 0.3)
    sel = (lambda t: t) if whole_batch_loss else (lambda t: t[0])
    R.calculate_loss(sel(ref), sel(gt), True).backward()
    nconv_amd.train.calculate_loss(sel(out), sel(gt).to(gpu, torch.float32), True).backward()
    torch.cuda.synchronize()
    named = dict(net.named_parameters())
    report = []
    for n, (w, b) in params.items():
        for lab, ref_t in (("weight", w), ("bias", b)):
            got = named[f"d_net.{n}.{lab}"].grad.double().cpu()
            rel = ((got - ref_t.grad).abs().max() / ref_t.grad.abs().max().clamp_min(1e-30)).item()
            report.append(f"{n}.{lab}: {rel:.2e}" + ("" if rel <= 1e-3 else "  <-- FAIL"))
        torch.testing.assert_close(named[f"d_net.{n}.weight"].detach().double().cpu(), w.detach(),
                                   rtol=2e-6, atol=2e-7)
    return report


@pytest.mark.timeout(300)
def test_dnet_train_gradients_config4b_full_size(nconv_amd, gpu):
    """The bench's training leg at its own batch (config 4b: B=8 352x1216, generalized crop,
    calculate_loss on the whole batch as train_step1.py:63, exact fp32 backward -- the deferred
    split-K weight-gradient reduction over 3.4 M pixels, the fused nconv1 / nconv7 gradients, the
    materialised pools): all 18 gradients normwise within 1e-3 of the fp64 oracle on the GPU's
    pool branch."""
    report = _train_gradients_vs_oracle(nconv_amd, gpu, 8, 352, 1216, "generalized", True, seed=13)
    print("\n".join(report))
    assert len(report) == 18
    assert not any(r.endswith("FAIL") for r in report), "\n".join(report)


@pytest.mark.parametrize("H,W", [(64, 96), (45, 67), (264, 100)])  # 264: full-height rows (>= 256)
def test_dnet_train_gradients(nconv_amd, gpu, H, W, bwd_math):
    """Step-1 training gradients (EnforcePos + calculate_loss on [0] + backward) vs the fp64 oracle.

    Near an isolated depth sample every window holds the same single sample, so neighbouring
    outputs equal that depth up to rounding and the 2x2 max-pool winner is decided by rounding
    noise (any two fp32 implementations, e.g. the reference on CPU and on GPU, disagree there).
    The max-pool gradient is discontinuous in exactly those places, so the fp64 oracle is run on
    the branch the GPU took: its pool winners are forced to the GPU's (computed by torch's own
    max_pool2d on the GPU's activations). Tie-breaking itself is tested bit-exactly elsewhere
    (test_gpu_layers, integer-valued pooling cases). Tolerance: normwise 1e-3 per tensor."""
    report = _train_gradients_vs_oracle(nconv_amd, gpu, 2, H, W, "literal", False)
    print("\n".join(report))
    assert not any(r.endswith("FAIL") for r in report), "\n".join(report)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_inference_streams_split_matches_one_stream(nconv_amd, gpu, n):
    """The whole inference chain on batch slices in n streams (DNET.inference_streams; the
    exact-fp32 default is 2) writes the same bits as one stream, eager and graphed (n = 8 > B:
    one frame per stream)."""
    net = make_net(nconv_amd, "generalized", gpu)
    g = torch.Generator().manual_seed(37)
    S = sparse_depth(g, 5, 96, 160).to(gpu)
    with torch.no_grad():
        net.d_net.inference_streams = 1
        a = net(S)
        net.d_net.inference_streams = n
        b = net(S)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            c = net(S)
        graph.replay()
        torch.cuda.synchronize()
        net.d_net.inference_streams = None
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("B,shares,bounds", [(1, None, [0, 1]), (2, (100, 1), [0, 2, 2]), (2, (1, 100), [0, 0, 2])])
def test_inference_split_with_an_empty_slice(nconv_amd, gpu, B, shares, bounds):
    """Two configured inference streams where a slice holds no frame -- B = 1 (one stream used), or
    shares that round one slice to zero frames (the second stream idle; or the first, every frame
    on the side stream) -- write the same bits as one stream (16 x 16: the fused path's smallest)."""
    net = make_net(nconv_amd, "generalized", gpu)
    d = net.d_net
    S = sparse_depth(torch.Generator().manual_seed(41), B, 16, 16, density=0.3).to(gpu)
    with torch.no_grad():
        d.inference_streams = 1
        a, ac = net.forward_with_confidence(S)
        d.inference_streams, d.inference_shares = 2, shares
        assert d.split_bounds(B, d._n_streams(B), shares, 2) == bounds
        b, bc = net.forward_with_confidence(S)
        c = net(S)
        torch.cuda.synchronize()
    assert a.shape == (B, 1, 16, 16) and torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(ac, bc)


# ---- full-size configurations (BASELINE.json configs[1] and configs[4]) ----------------------------
_ORACLE_CACHE = {}


def _oracle_out(net, S, crop):
    key = (tuple(S.shape), crop, float(S.sum()))
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE.clear()
        _ORACLE_CACHE[key] = R.dnet_forward(S.double(), oracle_params(net), crop)
    return _ORACLE_CACHE[key]


@pytest.fixture(params=["fp32", "bf16x9", "bf16x3"])
def fwd_math(request, nconv_amd, monkeypatch):
    monkeypatch.setattr(nconv_amd.nconv, "FORWARD_MATH", nconv_amd.nconv._MATH_NAMES[request.param])
    return request.param


@pytest.mark.parametrize("B,H,W,crop", [(8, 352, 1216, "generalized"), (1, 1024, 2048, "generalized"),
                                        (1, 1024, 2048, "literal")])
def test_dnet_full_size_vs_oracle(nconv_amd, gpu, fwd_math, B, H, W, crop):
    """Config 2 (B=8 352x1216: per-image buffer resources, the persistent grids' tile walk across
    images) and the config-5 plane (1024x2048; the literal crop returns 480x640 there) against the
    fp64 oracle, both arithmetics."""
    net = make_net(nconv_amd, crop, gpu)
    g = torch.Generator().manual_seed(B * 7 + H)
    S = sparse_depth(g, B, H, W)
    with torch.no_grad():
        out = net(S.to(gpu)).double().cpu()
    ref = _oracle_out(net, S, crop)
    assert out.shape == ref.shape == (B, 1) + ((H, W) if crop == "generalized" else (min(480, H + 1), min(640, W + 1)))
    err = (out - ref).abs()
    _report(f"full {fwd_math} {crop} {B}x{H}x{W}", err, ref)
    bound = 1e-4 * ref.abs() + 1e-6
    assert (err <= bound).all(), f"max err {err.max():.3e} ratio {(err / bound).max():.3f}"


def test_config5_batch16_matches_per_frame(nconv_amd, gpu, fwd_math):
    """Config 5 shape (B=16, 1024x2048, generalized crop): the batched forward is finite and
    bitwise equal to sixteen B=1 forwards (frames are independent; checks the per-image offset /
    resource arithmetic at a 2 M-pixel plane and 16 images)."""
    net = make_net(nconv_amd, "generalized", gpu)
    g = torch.Generator().manual_seed(55)
    S = sparse_depth(g, 16, 1024, 2048).to(gpu)
    with torch.no_grad():
        out = net(S)
        assert out.shape == (16, 1, 1024, 2048) and torch.isfinite(out).all()
        for i in range(16):
            assert torch.equal(net(S[i:i + 1]), out[i:i + 1]), f"frame {i}"


@pytest.mark.parametrize("frozen", [("nconv6.weight", "nconv6.bias"), ("nconv6.weight",), ("nconv6.bias",),
                                    ("nconv7.weight",)])
def test_frozen_layers_fused_tail_matches_unfused(nconv_amd, gpu, monkeypatch, frozen):
    """Individually frozen layers around the fused tail backward (nconv7's backward inside
    nconv6's): every trainable gradient equals the unfused path's (nconv6 and nconv7 as two
    backward launches) within 1e-5 normwise -- in particular nconv7's weight gradient when nconv6's
    weight and bias are both frozen, which the fused form cannot produce (it accumulates nconv7's
    weight gradient inside nconv6's weight-gradient pass), so DNETFn must not take it then."""
    g = torch.Generator().manual_seed(91)
    S = sparse_depth(g, 2, 64, 96).to(gpu)
    gt = (torch.rand(2, 1, 64, 96, generator=g) * 80).to(gpu)
    grads = {}
    for fused in (True, False):
        monkeypatch.setattr(nconv_amd.dnet, "FUSE_TAIL_BWD", fused)
        net = make_net(nconv_amd, "generalized", gpu)
        for n, p in net.d_net.named_parameters():
            p.requires_grad_(n not in frozen)
        net.train()
        out = net(S)
        nconv_amd.train.calculate_loss(out, gt, True).backward()
        torch.cuda.synchronize()
        grads[fused] = {n: (p.grad.detach().clone() if p.grad is not None else None)
                        for n, p in net.d_net.named_parameters() if "bnorm" not in n}
    for n, a in grads[True].items():
        b = grads[False][n]
        assert (a is None) == (b is None) == (n in frozen), n
        if a is None:
            continue
        assert torch.isfinite(a).all(), n
        rel = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
        assert rel <= 1e-5, f"{n}: {rel:.2e}"


def test_weight_prologue_bitwise_separate_launches(nconv_amd, gpu):
    """nconv_weight_prologue (one launch) writes bitwise what nconv_weight_prep (no softplus),
    nconv_head_weights and nconv_phase_weights write as separate launches."""
    N = nconv_amd.nconv
    net = make_net(nconv_amd, "generalized", gpu)
    layers = [getattr(net.d_net, n) for n in nconv_amd.dnet.LAYERS]
    ws = [m.weight.detach() for m in layers]
    sa = [torch.empty(w.shape[0], device=gpu) for w in ws]
    sb = [torch.empty(w.shape[0], device=gpu) for w in ws]
    N.weight_prep(ws, [False] * len(ws), sa)
    l1, l2 = layers[0], layers[1]
    sp1, sp2 = l1.spec(nconv_amd._lib.THRESH, 0.01), l2.spec()
    S = torch.zeros(1, 1, 32, 32, device=gpu)
    ha = N.head_weights(sp1, sp2, S, ws[0], l1.bias.detach(), sa[0], ws[1], l2.bias.detach(), sa[1])
    pws = [ws[5], ws[6], ws[7]]
    pa = [torch.empty(1024, device=gpu) for _ in range(3)]
    N.phase_weights(pws, [8, 8, 0], pa)
    hb = torch.full((N.HEAD_WEIGHTS_FLOATS,), float("nan"), device=gpu)
    pb = [torch.full((1024,), float("nan"), device=gpu) for _ in range(3)]
    N.weight_prologue(ws, sb, head=(ws[0], ws[1], hb), phase=(pws, [8, 8, 0], pb))
    torch.cuda.synchronize()
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)
    assert torch.equal(ha.view(torch.int32), hb.view(torch.int32))
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (8, 352, 1216)])
def test_dnet_eval_merged_prologue_bitwise(nconv_amd, gpu, B, H, W):
    """The eval forward with its one-launch weight prologue equals the separate-launch path
    bitwise, and a weight changed in place between forwards is picked up (no stale prologue)."""
    net = make_net(nconv_amd, "generalized", gpu)
    d = net.d_net
    g = torch.Generator().manual_seed(B * 7 + H)
    S = sparse_depth(g, B, H, W).to(gpu)
    with torch.no_grad():
        d.merged_prologue = False
        a = net(S)
        d.merged_prologue = True
        b = net(S)
        assert torch.equal(a, b)
        d.nconv6.weight.mul_(1.5)
        d.nconv2.weight.mul_(0.75)
        c = net(S)
        d.merged_prologue = False
        e = net(S)
    assert torch.equal(c, e) and not torch.equal(b, c)
