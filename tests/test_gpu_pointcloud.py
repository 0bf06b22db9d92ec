"""GPU: nconv_backproject_map / nconv_backproject_points (csrc/backproject.hip) against the numpy
reference of pointcloud_cases, and DNET.forward_with_confidence against the per-layer chain and a
float64 restatement. The back-projection arithmetic is exact in the reference's terms, so every
comparison of it is torch.equal (floats compared as their bit patterns: NaN marks the invalid pixels
of the organised form). Sources are slices of larger allocations (every base alignment, odd row
strides); outputs are the middle of sentinel-filled buffers whose guards must come back intact."""
import numpy as np
import pytest
import torch

import pointcloud_cases as PC
from oracle import nconv_ref as R

pytestmark = pytest.mark.gpu

GUARD = 5                       # rows before and after every output
S_XYZ, S_RGB, S_IDX, S_OFF = -7777.0, 0xA5, -99, -5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, ref):
    """A device fp32 tensor equals a numpy float32 array bit for bit."""
    return got.shape == tuple(ref.shape) and torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(np.ascontiguousarray(ref))))


def _guarded_out(dev, cap, B, rgb, index, n_ws):
    """({name: whole buffer}, out dict of their middle slices)."""
    g = GUARD
    whole = {"xyz": torch.full((cap + 2 * g, 3), S_XYZ, device=dev),
             "offsets": torch.full((B + 1 + 2 * g,), S_OFF, dtype=torch.int32, device=dev),
             "workspace": torch.full((n_ws + 2 * 16 * g,), S_RGB, dtype=torch.uint8, device=dev)}
    if rgb:
        whole["rgb"] = torch.full((cap + 2 * g, 3), S_RGB, dtype=torch.uint8, device=dev)
    if index:
        whole["index"] = torch.full((cap + 2 * g,), S_IDX, dtype=torch.int32, device=dev)
    out = {k: (v[16 * g:16 * g + n_ws] if k == "workspace" else v[g:v.shape[0] - g]) for k, v in whole.items()}
    return whole, out


SENTINEL = {"xyz": S_XYZ, "rgb": S_RGB, "index": S_IDX, "offsets": S_OFF, "workspace": S_RGB}


def _guards_intact(whole):
    for k, v in whole.items():
        g = 16 * GUARD if k == "workspace" else GUARD
        edge = torch.cat([v[:g].reshape(-1), v[v.shape[0] - g:].reshape(-1)])
        if not bool((edge == SENTINEL[k]).all()):
            return False
    return True


def _check_points(P, dev, depth, k, ref, *, cap=None, **kw):
    """backproject(...) into guarded buffers == ref (points_ref) up to the capacity; the rest of the
    buffers keeps its sentinel; offsets are the true ones. Returns the PointCloud."""
    B, H, W = len(ref["offsets"]) - 1, depth.shape[-2], depth.shape[-1]
    total = int(ref["offsets"][-1])
    capacity = B * H * W if cap is None else cap
    whole, out = _guarded_out(dev, capacity, B, kw.get("color") is not None, kw.get("with_index", False),
                              P.workspace_bytes(B, H, W))
    pc = P.backproject(depth, k, max_points=cap, out=out, **kw)
    n = min(total, capacity)
    assert pc.xyz.data_ptr() == out["xyz"].data_ptr() and pc.capacity == capacity
    assert torch.equal(pc.offsets.cpu(), torch.from_numpy(ref["offsets"]))
    assert pc.count() == total and pc.truncated() == (total > capacity)
    assert _same(pc.xyz[:n], ref["xyz"][:n])
    assert bool((pc.xyz[n:] == S_XYZ).all())
    if kw.get("color") is not None:
        assert torch.equal(pc.rgb[:n].cpu(), torch.from_numpy(ref["rgb"][:n]))
        assert bool((pc.rgb[n:] == S_RGB).all())
    else:
        assert pc.rgb is None
    if kw.get("with_index"):
        assert torch.equal(pc.index[:n].cpu(), torch.from_numpy(ref["index"][:n]))
        assert bool((pc.index[n:] == S_IDX).all())
    else:
        assert pc.index is None
    assert _guards_intact(whole)
    return pc


def _check_map(P, dev, depth, k, ref_xyz, **kw):
    B = ref_xyz.shape[0]
    buf = torch.full((B + 2,) + tuple(ref_xyz.shape[1:]), S_XYZ, device=dev)
    got = P.backproject_map(depth, k, out=buf[1:1 + B], **kw)
    assert got.data_ptr() == buf[1].data_ptr() and _same(got, ref_xyz)
    assert bool((buf[0] == S_XYZ).all()) and bool((buf[-1] == S_XYZ).all())


def _view(dev, rng, values, left, fill):
    big, cut = PC.allocation(rng, values, left, fill)
    return cut(torch.from_numpy(big).to(dev))


@pytest.mark.parametrize("W", PC.SWEEP_W)
def test_sweep(nconv_amd, gpu, W):
    """B x H x base alignment for one width; the validity pattern, the confidence gate, the colour
    form, reverse, the shape of k and the index cycle over the cases. Both kernels on every case."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(300 + W)
    n = 0
    for B in PC.SWEEP_B:
        for H in PC.SWEEP_H:
            for left in PC.SWEEP_LEFT:
                pattern = PC.PATTERNS[n % len(PC.PATTERNS)]
                zlim = dict(z_min=1.0, z_max=50.0) if pattern == "edges" else {}
                z = PC.depth_values(rng, B, H, W, pattern, **zlim)
                k = PC.intrinsics(rng, B if n % 2 else None)
                kw = dict(zlim)
                tkw = dict(zlim)
                if n % 3 == 1:
                    conf = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.nan], dtype=np.float32), (B, H, W))
                    kw.update(conf=conf, conf_min=0.5)
                    tkw.update(conf=_view(gpu, rng, conf, (left + 1) % 4, 1.0)[:, None], conf_min=0.5)
                color = None
                if n % 4 == 1:
                    color = rng.uniform(-20, 280, (B, 3, H, W)).astype(np.float32)
                    color[rng.random(color.shape) < 0.1] = np.nan
                elif n % 4 in (2, 3):
                    color = rng.integers(0, 256, (B, H, W, 3), dtype=np.int64).astype(np.uint8)
                rev = bool((n // 4) % 2)
                ref = PC.points_ref(z, k, color=color, reverse=rev, **kw)
                td = _view(gpu, rng, z, left, 5.0)[:, None]  # the guard depths are valid ones: a stray read shows
                tk = torch.from_numpy(k).to(gpu)
                pkw = dict(tkw, with_index=bool(n % 2))
                if color is not None:
                    pkw.update(color=_view(gpu, rng, color, left if n % 4 != 3 else (left + 2) % 4, 77), reverse=rev)
                _check_points(P, gpu, td, tk, ref, **pkw)
                _check_map(P, gpu, td, tk, PC.map_ref(z, k, **kw)[0], **tkw)
                n += 1


@pytest.mark.parametrize("pattern", PC.PATTERNS)
def test_validity_patterns(nconv_amd, gpu, pattern):
    """Every pattern on a shape of several rows and three segments per row (the last partial):
    contiguous with W % 4 == 0 (the wide loads), an aligned view whose rows end inside a lane's four
    pixels (wide loads beside element-wide ones) and an unaligned slice."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(len(pattern) + 40)
    B, H, W = 2, 5, 600
    zlim = dict(z_min=1.0, z_max=50.0) if pattern == "edges" else {}
    z = PC.depth_values(rng, B, H, W, pattern, **zlim)
    k = PC.intrinsics(rng, B)
    ref = PC.points_ref(z, k, **zlim)
    tk = torch.from_numpy(k).to(gpu)
    for td in (torch.from_numpy(z).to(gpu)[:, None], _view(gpu, rng, z, 1, 5.0)[:, None]):
        pc = _check_points(P, gpu, td, tk, ref, with_index=True, **zlim)
        _check_map(P, gpu, td, tk, PC.map_ref(z, k, **zlim)[0], **zlim)
    wide = torch.full((B, 1, H, W), 5.0, device=gpu)
    wide.copy_(torch.from_numpy(z)[:, None])
    for w in (W - 1, W - 3):  # 16-byte aligned base and strides, the last lane of a row holds 3 / 1 pixels
        zw = np.ascontiguousarray(z[:, :, :w])
        _check_points(P, gpu, wide[..., :w], tk, PC.points_ref(zw, k, **zlim), with_index=True, **zlim)
        _check_map(P, gpu, wide[..., :w], tk, PC.map_ref(zw, k, **zlim)[0], **zlim)
    if pattern == "none":
        assert pc.offsets.cpu().tolist() == [0] * (B + 1) and pc.count() == 0
    if pattern == "all":
        assert pc.count() == B * H * W and not pc.truncated()
    if pattern == "edges":
        kept = z.reshape(-1)[pc.index[:pc.count()].cpu().numpy()]
        assert not (kept == 1.0).any() and (kept == 50.0).any() and (z == 1.0).any()


def test_confidence_gate(nconv_amd, gpu):
    """conf == conf_min passes, just below does not, NaN does not; the gate and the depth window combine."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(11)
    B, H, W = 2, 3, 300
    z = PC.depth_values(rng, B, H, W, "p50")
    cmin = np.float32(0.3)
    pool = np.array([cmin, np.nextafter(cmin, np.float32(0)), np.nextafter(cmin, np.float32(1)), 0.0, 1.0, np.nan,
                     np.inf, -np.inf], dtype=np.float32)
    conf = pool[rng.integers(0, len(pool), (B, H, W))]
    k = PC.intrinsics(rng)
    ref = PC.points_ref(z, k, conf=conf, conf_min=float(cmin))
    assert 0 < ref["offsets"][-1] < PC.points_ref(z, k)["offsets"][-1]
    td, tk = torch.from_numpy(z).to(gpu)[:, None], torch.from_numpy(k).to(gpu)
    for tc in (torch.from_numpy(conf).to(gpu)[:, None], _view(gpu, rng, conf, 3, 1.0)[:, None]):
        pc = _check_points(P, gpu, td, tk, ref, conf=tc, conf_min=float(cmin), with_index=True)
    c_kept = conf.reshape(-1)[pc.index[:pc.count()].cpu().numpy()]
    assert (c_kept == cmin).any() and (c_kept >= cmin).all()
    _check_map(P, gpu, td, tk, PC.map_ref(z, k, conf=conf, conf_min=float(cmin))[0], conf=tc, conf_min=float(cmin))
    # conf_min = 0 (the default) still drops a NaN confidence
    ref0 = PC.points_ref(z, k, conf=conf)
    _check_points(P, gpu, td, tk, ref0, conf=tc)


def test_intrinsics_forms(nconv_amd, gpu):
    """One camera (3, 3) for the batch and one per image (B, 3, 3); only fx, fy, cx, cy are read (the
    other entries are NaN here); (H, W) and (1, H, W) depths are one image."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(12)
    B, H, W = 3, 4, 70
    z = PC.depth_values(rng, B, H, W, "p50")
    k1, kb = PC.intrinsics(rng), PC.intrinsics(rng, B)
    assert np.isnan(kb[:, 0, 1]).all() and len({float(v) for v in kb[:, 0, 0]}) == B
    td = torch.from_numpy(z).to(gpu)[:, None]
    for k in (k1, kb):
        _check_points(P, gpu, td, torch.from_numpy(k).to(gpu), PC.points_ref(z, k))
    same = np.broadcast_to(k1, (B, 3, 3)).copy()
    _check_points(P, gpu, td, torch.from_numpy(same).to(gpu), PC.points_ref(z, k1))
    r1 = PC.points_ref(z[:1], kb[1])
    for d1 in (td[0, 0], td[0]):
        _check_points(P, gpu, d1, torch.from_numpy(kb[1]).to(gpu), r1)
        _check_map(P, gpu, d1, torch.from_numpy(kb[1:2]).to(gpu), PC.map_ref(z[:1], kb[1])[0])
    with pytest.raises(ValueError, match="k must be"):
        P.backproject(td, torch.from_numpy(kb[:2]).to(gpu))


@pytest.mark.parametrize("form", ["f32", "u8"])
def test_colour(nconv_amd, gpu, form):
    """Both source forms, contiguous (wide loads) and sliced, with and without reverse; the fp32
    values -3, 254.5, 255.5, 300 and NaN among them."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(13)
    B, H, W = 2, 3, 260
    z = PC.depth_values(rng, B, H, W, "p50")
    z[0, 0, :len(PC.COLOR_SPECIAL)] = 2.0
    k = PC.intrinsics(rng, B)
    if form == "f32":
        color = rng.uniform(-20, 280, (B, 3, H, W)).astype(np.float32)
        color[0, :, 0, :len(PC.COLOR_SPECIAL)] = PC.COLOR_SPECIAL
    else:
        color = rng.integers(0, 256, (B, H, W, 3), dtype=np.int64).astype(np.uint8)
    td, tk = torch.from_numpy(z).to(gpu)[:, None], torch.from_numpy(k).to(gpu)
    for rev in (False, True):
        ref = PC.points_ref(z, k, color=color, reverse=rev)
        for tc in (torch.from_numpy(color).to(gpu), _view(gpu, rng, color, 1, 9), _view(gpu, rng, color, 0, 9)):
            pc = _check_points(P, gpu, td, tk, ref, color=tc, reverse=rev)
        if form == "f32":
            first = pc.rgb[:5].cpu()[:, 2 if rev else 0].tolist()
            assert first == [0, 254, 255, 255, 0]  # -3, 254.5 (tie to even), 255.5, 300, NaN
    with pytest.raises(ValueError, match="color"):
        P.backproject(td, tk, color=torch.zeros(B, 3, H, W + 1, device=gpu))
    with pytest.raises(TypeError, match="color"):
        P.backproject(td, tk, color=torch.zeros(B, 3, H, W, device=gpu, dtype=torch.float64))


def test_index_ties_the_two_kernels(nconv_amd, gpu):
    """index maps every point back to its pixel, and xyz equals backproject_map gathered there."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(14)
    B, H, W = 3, 9, 513
    z = PC.depth_values(rng, B, H, W, "special")
    k = PC.intrinsics(rng, B)
    td, tk = _view(gpu, rng, z, 2, 5.0)[:, None], torch.from_numpy(k).to(gpu)
    pc = P.backproject(td, tk, with_index=True)
    m = P.backproject_map(td, tk)
    n = pc.count()
    assert n == int(PC.valid_ref(z).sum()) and not pc.truncated()
    idx = pc.index[:n].long()
    assert bool((idx[1:] > idx[:-1]).all())
    gathered = m.permute(0, 2, 3, 1).reshape(-1, 3)[idx]
    assert torch.equal(_bits(pc.xyz[:n]), _bits(gathered))
    valid = torch.zeros(B * H * W, dtype=torch.bool, device=gpu)
    valid[idx] = True
    assert torch.equal(valid.cpu(), torch.from_numpy(PC.valid_ref(z).reshape(-1)))
    assert bool(torch.isnan(m.permute(0, 2, 3, 1).reshape(-1, 3)[~valid]).all())
    off = pc.host_offsets()
    for b in range(B):
        xyz_b, rgb_b, idx_b = pc.image(b)
        assert rgb_b is None and xyz_b.shape[0] == off[b + 1] - off[b]
        assert bool(((idx_b >= b * H * W) & (idx_b < (b + 1) * H * W)).all())


def test_capacity(nconv_amd, gpu):
    """max_points 0, 1, total - 1, total: the prefix is written, the rest keeps its sentinel, offsets
    report the true totals, truncated() is right."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(15)
    B, H, W = 2, 3, 300
    z = PC.depth_values(rng, B, H, W, "p50")
    k = PC.intrinsics(rng)
    color = rng.integers(0, 256, (B, H, W, 3), dtype=np.int64).astype(np.uint8)
    ref = PC.points_ref(z, k, color=color)
    total = int(ref["offsets"][-1])
    td, tk, tc = torch.from_numpy(z).to(gpu)[:, None], torch.from_numpy(k).to(gpu), torch.from_numpy(color).to(gpu)
    for cap in (0, 1, total - 1, total, total + 3):
        pc = _check_points(P, gpu, td, tk, ref, cap=cap, color=tc, with_index=True)
        assert pc.truncated() == (cap < total)
        got = sum(pc.image(b)[0].shape[0] for b in range(B))
        assert got == min(cap, total)
    with pytest.raises(ValueError, match="negative"):
        P.backproject(td, tk, max_points=-1)


def test_captured_in_a_graph(nconv_amd, gpu):
    """backproject and backproject_map into static buffers, captured in a hipGraph and replayed on new
    depths, equal the eager calls bit for bit: no allocation, no synchronisation inside."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(16)
    B, H, W = 2, 9, 300
    k = PC.intrinsics(rng, B)
    tk = torch.from_numpy(k).to(gpu)
    new = lambda: (PC.depth_values(rng, B, H, W, "p50"), rng.integers(0, 256, (B, H, W, 3), dtype=np.int64).astype(np.uint8))
    z0, c0 = new()
    s_z, s_c = torch.from_numpy(z0).to(gpu)[:, None], torch.from_numpy(c0).to(gpu)
    cap = B * H * W
    out = {"xyz": torch.zeros(cap, 3, device=gpu), "rgb": torch.zeros(cap, 3, dtype=torch.uint8, device=gpu),
           "index": torch.zeros(cap, dtype=torch.int32, device=gpu),
           "offsets": torch.zeros(B + 1, dtype=torch.int32, device=gpu),
           "workspace": torch.zeros(P.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)}
    m_out = torch.zeros(B, 3, H, W, device=gpu)
    P.backproject(s_z, tk, color=s_c, with_index=True, out=out)  # library loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        P.backproject(s_z, tk, color=s_c, with_index=True, out=out)
        P.backproject_map(s_z, tk, out=m_out)
    for _ in range(2):
        z1, c1 = new()
        s_z.copy_(torch.from_numpy(z1)[:, None])
        s_c.copy_(torch.from_numpy(c1))
        out["xyz"].fill_(S_XYZ)
        g.replay()
        torch.cuda.synchronize()
        eager = P.backproject(s_z, tk, color=s_c, with_index=True)
        n = eager.count()
        ref = PC.points_ref(z1, k, color=c1)
        assert n == int(ref["offsets"][-1]) and torch.equal(out["offsets"], eager.offsets)
        assert torch.equal(_bits(out["xyz"][:n]), _bits(eager.xyz[:n])) and _same(out["xyz"][:n], ref["xyz"])
        assert bool((out["xyz"][n:] == S_XYZ).all())
        assert torch.equal(out["rgb"][:n], eager.rgb[:n]) and torch.equal(out["index"][:n], eager.index[:n])
        assert torch.equal(_bits(m_out), _bits(P.backproject_map(s_z, tk)))


def test_argument_errors_on_the_device(nconv_amd, gpu):
    P = nconv_amd.pointcloud
    z, k = torch.ones(2, 1, 4, 8, device=gpu), torch.eye(3, device=gpu)
    with pytest.raises(ValueError, match="conf"):
        P.backproject(z, k, conf=torch.ones(2, 1, 4, 9, device=gpu))
    with pytest.raises(ValueError, match="z_max"):
        P.backproject(z, k, z_min=2.0, z_max=1.0)
    with pytest.raises(TypeError, match="out"):
        P.backproject(z, k, out={"xyz": torch.zeros(64, 4, device=gpu)})
    with pytest.raises(TypeError, match="out"):
        P.backproject_map(z, k, out=torch.zeros(2, 3, 8, 4, device=gpu))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        P.backproject(z, k.cpu())


# ---- DNET's output confidence ------------------------------------------------------------------------
def _sparse(g, B, H, W, density=0.2):
    d = torch.rand(B, 1, H, W, generator=g) * 79 + 1
    return d * (torch.rand(B, 1, H, W, generator=g) < density)


def _net(nconv_amd, crop, dev):
    torch.manual_seed(0)
    net = nconv_amd.SETP1_NCONV(crop=crop).to(dev)
    net.train()  # one training-mode forward: EnforcePos makes the weights positive (what training produces)
    with torch.no_grad():
        net(torch.zeros(1, 1, 32, 32, device=dev))
    return net.eval()


def _chain_confidence(nconv_amd, d, S):
    """nconv7's whole confidence grid from one nconv_fwd launch per layer (the unfused chain of
    DNET.forward), uncropped."""
    L = nconv_amd._lib
    f = nconv_amd.nconv.layer_forward_raw
    layers = [getattr(d, n) for n in nconv_amd.dnet.LAYERS]
    (l1, l2, d1, d2, d3, l4, l5, l6, l7) = layers
    (s1, s2, sd1, sd2, sd3, s4, s5, s6, s7) = d._prologue(layers, S)
    x1, c1 = f(l1.spec(L.THRESH, 0.01), S, None, None, None, l1.weight, l1.bias, s1)
    x1, c1 = f(l2.spec(), x1, c1, None, None, l2.weight, l2.bias, s2)
    x2, c2 = f(d1.spec(L.POOL2), x1, c1, None, None, d1.weight, d1.bias, sd1)
    x3, c3 = f(d2.spec(L.POOL2), x2, c2, None, None, d2.weight, d2.bias, sd2)
    x4, c4 = f(d3.spec(L.POOL2), x3, c3, None, None, d3.weight, d3.bias, sd3)
    x34, c34 = f(l4.spec(L.UPCAT_SKIP_FIRST), x3, c3, x4, c4, l4.weight, l4.bias, s4)
    x23, c23 = f(l5.spec(L.UPCAT_SKIP_FIRST), x2, c2, x34, c34, l5.weight, l5.bias, s5)
    xo, co = f(l6.spec(L.UPCAT_UP_FIRST), x1, c1, x23, c23, l6.weight, l6.bias, s6)
    xo, co = f(l7.spec(), xo, co, None, None, l7.weight, l7.bias, s7)
    return co


def _oracle_confidence(S, params):
    """DNET's forward (models/step1.py:51-92) in float64, layer by layer from oracle nconv2d, keeping
    the confidence the reference drops; uncropped."""
    F = torch.nn.functional

    def L(name, x, c):
        w, b = params[name]
        st, pad = R.DNET_GEOMETRY[name]
        return R.nconv2d(x, c, w, b, st, pad)

    P = lambda t: F.max_pool2d(t, 2, 2)
    up = lambda t, ref: F.interpolate(t, ref.shape[2:], mode="nearest")
    c0 = (S > 0.01).to(S.dtype)
    x1, c1 = L("nconv1", S, c0)
    x1, c1 = L("nconv2", x1, c1)
    x2, c2 = L("nconv_down1", P(x1), P(c1))
    x3, c3 = L("nconv_down2", P(x2), P(c2))
    x4, c4 = L("nconv_down3", P(x3), P(c3))
    x34, c34 = L("nconv4", torch.cat((x3, up(x4, c3)), 1), torch.cat((c3, up(c4, c3)), 1))
    x23, c23 = L("nconv5", torch.cat((x2, up(x34, c2)), 1), torch.cat((c2, up(c34, c2)), 1))
    xo, co = L("nconv6", torch.cat((up(x23, S), x1), 1), torch.cat((up(c23, S), c1), 1))
    xo, co = L("nconv7", xo, co)
    return xo, co


@pytest.mark.parametrize("fused_head", [True, False])
@pytest.mark.parametrize("crop", ["literal", "generalized"])
@pytest.mark.parametrize("B,H,W", [(1, 16, 20), (3, 16, 20), (1, 24, 36), (3, 24, 36)])
def test_dnet_forward_with_confidence(nconv_amd, gpu, B, H, W, crop, fused_head):
    """The depth is forward(S)'s bit for bit; the confidence agrees with the per-layer chain and with
    the float64 restatement within the forward's bound, 1e-4 |ref| + 1e-6 (test_gpu_dnet.py); it is
    0 in nconv7's zero border (where the crop reaches it), checked against the chain, and B = 3 goes
    through the two-stream batch split, every slice written."""
    net = _net(nconv_amd, crop, gpu)
    d = net.d_net
    d.fused_head = fused_head
    g = torch.Generator().manual_seed(1000 * H + W + B)
    S = _sparse(g, B, H, W)
    Sd = S.to(gpu)
    oh, ow = nconv_amd.crop_hw(H, W, crop)
    with torch.no_grad():
        want = net(Sd)
        depth, conf = net.forward_with_confidence(Sd)
        depth2, conf2 = d.forward_with_confidence(Sd)
        chain = _chain_confidence(nconv_amd, d, Sd)[:, :, 1:1 + oh, 1:1 + ow]
    assert d._n_streams(B) == (2 if B > 1 else 1)
    assert depth.shape == conf.shape == want.shape == (B, 1, oh, ow)
    assert torch.equal(depth, want) and torch.equal(depth2, want) and torch.equal(conf2, conf)
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    x64, c64 = _oracle_confidence(S.double(), R.dnet_params_from_state_dict(sd))
    x64, c64 = x64[:, :, 1:1 + oh, 1:1 + ow], c64[:, :, 1:1 + oh, 1:1 + ow]
    for name, ref in (("chain", chain.double().cpu()), ("float64", c64)):
        err = (conf.double().cpu() - ref).abs()
        bound = 1e-4 * ref.abs() + 1e-6
        assert (err <= bound).all(), f"{name}: max err {err.max():.3e} ratio {(err / bound).max():.3f}"
    assert ((depth.double().cpu() - x64).abs() <= 1e-4 * x64.abs() + 1e-6).all()
    assert float(conf.min()) >= 0.0 and float(conf.max()) > 0.0
    # nconv6 (3x3, no padding) covers rows 2 .. H-1 of nconv7's (H+2) x (W+2) grid and the crop starts at
    # 1: outside rows 1 .. H-2 / columns 1 .. W-2 the output lies in nconv7's zero border
    border = torch.ones(oh, ow, dtype=torch.bool)
    border[1:H - 1, 1:W - 1] = False
    assert border.any() and bool((chain.cpu()[:, 0][:, border] == 0).all())
    assert bool((conf.cpu()[:, 0][:, border] == 0).all())
    for b in range(B):  # every slice of the batch split was written: each image's confidence is its own
        with torch.no_grad():
            one = net.forward_with_confidence(Sd[b:b + 1])[1]
        assert torch.equal(one[0], conf[b])
    with pytest.raises(RuntimeError, match="inference only"):
        net.forward_with_confidence(Sd)


def test_end_to_end_confident_points(nconv_amd, gpu):
    """SETP1_NCONV.forward_with_confidence -> backproject(depth, k, conf=c, conf_min=...) on one small
    frame: the points are the reference's on the same tensors."""
    net = _net(nconv_amd, "generalized", gpu)
    g = torch.Generator().manual_seed(5)
    S = _sparse(g, 1, 32, 48, density=0.1).to(gpu)
    k = PC.intrinsics(np.random.default_rng(5))
    with torch.no_grad():
        depth, conf = net.forward_with_confidence(S)
    cmin = float(conf.median())
    pc = nconv_amd.backproject(depth, torch.from_numpy(k).to(gpu), conf=conf, conf_min=cmin, with_index=True)
    ref = PC.points_ref(depth[:, 0].cpu().numpy(), k, conf=conf[:, 0].cpu().numpy(), conf_min=cmin)
    n = int(ref["offsets"][-1])
    assert 0 < n < depth.numel() and pc.count() == n and not pc.truncated()
    assert _same(pc.xyz[:n], ref["xyz"]) and torch.equal(pc.index[:n].cpu(), torch.from_numpy(ref["index"]))
