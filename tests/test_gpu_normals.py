"""GPU: nconv_depth_normals / nconv_depth_normals_points (csrc/normals.hip) against the numpy reference
of normals_cases. The arithmetic is exact in the reference's terms, so every comparison is bit for bit
(floats as their int32 patterns: NaN marks the pixels without a normal). Sources are slices of larger
allocations whose surroundings hold valid-looking depths (every base alignment, odd row strides), so a
read outside the view changes the result; outputs are the middle of sentinel-filled buffers whose
guards must come back intact."""
import ctypes

import numpy as np
import pytest
import torch

import normals_cases as NC
import pointcloud_cases as PC

pytestmark = pytest.mark.gpu

GUARD = 5
S_F32, S_U8, S_IDX, S_OFF = -7777.0, 0xA5, -99, -5
EMPTY = (9, 200, 31)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, ref):
    """A device fp32 tensor equals a numpy float32 array bit for bit."""
    return got.shape == tuple(ref.shape) and torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(np.ascontiguousarray(ref))))


def _view(dev, rng, values, left, fill):
    big, cut = PC.allocation(rng, values, left, fill)
    return cut(torch.from_numpy(big).to(dev))


def _guarded(dev, shape, fill, dtype):
    """(whole buffer with GUARD rows before and after, its middle)."""
    whole = torch.full((shape[0] + 2 * GUARD,) + tuple(shape[1:]), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + shape[0]]


def _intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[whole.shape[0] - GUARD:] == fill).all())


def _check_map(P, dev, depth, k, ref, **kw):
    """normals, normal_image and the two from one call, into guarded buffers, against the reference map."""
    B, _, H, W = ref.shape
    pic = NC.picture_ref(ref, EMPTY)
    wm, m = _guarded(dev, (B, 3, H, W), S_F32, torch.float32)
    wi, im = _guarded(dev, (B, H, W, 3), S_U8, torch.uint8)
    got = P.normals(depth, k, out=m, **kw)
    assert got.data_ptr() == m.data_ptr() and _same(got, ref)
    got_im = P.normal_image(depth, k, empty=EMPTY, out=im, **kw)
    assert got_im.data_ptr() == im.data_ptr() and torch.equal(got_im.cpu(), torch.from_numpy(pic))
    assert _intact(wm, S_F32) and _intact(wi, S_U8)
    wm2, m2 = _guarded(dev, (B, 3, H, W), S_F32, torch.float32)
    wi2, im2 = _guarded(dev, (B, H, W, 3), S_U8, torch.uint8)
    both = P.normals_and_image(depth, k, empty=EMPTY, out={"normals": m2, "image": im2}, **kw)
    assert both[0].data_ptr() == m2.data_ptr() and both[1].data_ptr() == im2.data_ptr()
    assert torch.equal(_bits(m2), _bits(m)) and torch.equal(im2, im)
    assert _intact(wm2, S_F32) and _intact(wi2, S_U8)


def _check_packed(P, dev, depth, k, ref, valid, *, cap=None, with_index=False, **kw):
    """backproject(normals=True): the rows equal the map gathered at the index; the rest keeps its sentinel."""
    B, _, H, W = ref.shape
    index = np.flatnonzero(valid.reshape(-1)).astype(np.int32)
    capacity = B * H * W if cap is None else cap
    n = min(len(index), capacity)
    wn, nrm = _guarded(dev, (capacity, 3), S_F32, torch.float32)
    wx, idx = _guarded(dev, (capacity,), S_IDX, torch.int32)
    pc = P.backproject(depth, k, normals=True, with_index=with_index, max_points=cap,
                       out={"normals": nrm, "index": idx}, **kw)
    assert pc.normals.data_ptr() == nrm.data_ptr() and pc.count() == len(index)
    assert (pc.index is None) == (not with_index)
    assert torch.equal(idx[:n].cpu(), torch.from_numpy(index[:n])) and bool((idx[n:] == S_IDX).all())
    assert _same(pc.normals[:n], NC.packed_ref(ref, index[:n]))
    assert bool((pc.normals[n:] == S_F32).all()) and _intact(wn, S_F32) and _intact(wx, S_IDX)
    return pc


@pytest.mark.parametrize("W", NC.SWEEP_W)
def test_sweep(nconv_amd, gpu, W):
    """B x H x base alignment for one width; the validity pattern, the confidence gate, the
    discontinuity gate and the shape of k cycle over the cases (7, 2, 3 and 2 of them: pairwise coprime
    but for the two 2s, which are taken from different digits of the counter)."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(500 + W)
    n = 0
    for B in NC.SWEEP_B:
        for H in NC.SWEEP_H:
            for left in NC.SWEEP_LEFT:
                pattern = PC.PATTERNS[n % len(PC.PATTERNS)]
                zlim = dict(z_min=1.0, z_max=50.0) if pattern == "edges" else {}
                z = PC.depth_values(rng, B, H, W, pattern, **zlim)
                k = PC.intrinsics(rng, B if (n // 2) % 2 else None)
                jump_rel, jump_abs = NC.GATES[n % 3]
                kw = dict(zlim, jump_rel=jump_rel, jump_abs=jump_abs)
                tkw = dict(kw)
                if n % 2 == 1:
                    conf = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.nan], dtype=np.float32), (B, H, W),
                                      p=[0.05, 0.05, 0.3, 0.25, 0.3, 0.05])
                    kw.update(conf=conf, conf_min=0.5)
                    tkw.update(conf=_view(gpu, rng, conf, (left + 1) % 4, 1.0)[:, None], conf_min=0.5)
                ref = NC.normals_ref(z, k, **kw)
                td = _view(gpu, rng, z, left, 5.0)[:, None]  # the surroundings are valid depths: a stray read shows
                tk = torch.from_numpy(k).to(gpu)
                _check_map(P, gpu, td, tk, ref, **tkw)
                if H == 1 or W == 1:
                    assert np.isnan(ref).all()
                n += 1


def test_all_valid_and_negative_z_min(nconv_amd, gpu):
    """Every pixel valid on several rows and three segments per row: contiguous with W % 4 == 0 (the
    wide loads), rows that end inside a lane's four pixels, an unaligned slice. With a negative z_min
    the 0 a load outside the view returns would be a valid depth: the image border must still be one."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(41)
    B, H, W = 2, 5, 600
    z = rng.uniform(9.0, 11.0, (B, H, W)).astype(np.float32)
    z[rng.random(z.shape) < 0.02] = 0.0  # valid under z_min = -1 and within jump_abs of nothing
    k = PC.intrinsics(rng, B)
    tk = torch.from_numpy(k).to(gpu)
    wide = torch.full((B, 1, H, W), 5.0, device=gpu)
    wide.copy_(torch.from_numpy(z)[:, None])
    for kw in (dict(), dict(z_min=-1.0, jump_rel=0.0, jump_abs=20.0), dict(z_min=-1.0, jump_rel=0.0, jump_abs=0.0)):
        ref = NC.normals_ref(z, k, **kw)
        assert not np.isnan(ref).all()
        for td in (wide, _view(gpu, rng, z, 1, 5.0)[:, None]):
            _check_map(P, gpu, td, tk, ref, **kw)
        for w in (W - 1, W - 3):
            zw = np.ascontiguousarray(z[:, :, :w])
            _check_map(P, gpu, wide[..., :w], tk, NC.normals_ref(zw, k, **kw), **kw)


def test_smooth_surfaces(nconv_amd, gpu):
    """A tilted plane and a sphere cap at (2, 9, 261): bit-equal to the reference, and so within
    PLANE_ANGLE_TOL of the analytic plane normal (test_normals_cpu.py holds the reference to it)."""
    P = nconv_amd.pointcloud
    B, H, W = 2, 9, 261
    tk = torch.from_numpy(NC.K_SMOOTH).to(gpu)
    cases = NC.plane_cases(H, W)
    z = np.concatenate([cases[1][0], cases[2][0]])
    ref = NC.normals_ref(z, NC.K_SMOOTH, jump_rel=0.0, jump_abs=0.0)
    got = P.normals(torch.from_numpy(z).to(gpu)[:, None], tk, jump_rel=0.0, jump_abs=0.0)
    assert _same(got, ref) and not bool(torch.isnan(got).any())
    for b, (_, n) in enumerate(cases[1:]):
        a = NC.angle(got[b:b + 1].cpu().numpy(), np.broadcast_to(n.reshape(1, 3, 1, 1), (1, 3, H, W))).max()
        assert a <= NC.PLANE_ANGLE_TOL
    zs, ns = NC.sphere_cap((0.3, 0.0, 60.0), 50.0, NC.K_SMOOTH, B, H, W)
    ref = NC.normals_ref(zs, NC.K_SMOOTH)
    got = P.normals(torch.from_numpy(zs).to(gpu)[:, None], tk)
    assert _same(got, ref) and not bool(torch.isnan(got).any())
    img = P.normal_image(torch.from_numpy(zs).to(gpu)[:, None], tk)
    assert torch.equal(img.cpu(), torch.from_numpy(NC.picture_ref(ref)))
    assert int(img[..., 2].min()) > 250  # the cap faces the camera: blue


@pytest.mark.parametrize("pattern", ("p50", "special", "all"))
def test_packed_form(nconv_amd, gpu, pattern):
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(60 + len(pattern))
    B, H, W = 3, 5, 261
    z = PC.depth_values(rng, B, H, W, pattern)
    if pattern == "all":
        z = (z * np.float32(0.05) + np.float32(20.0)).astype(np.float32)  # 20 m .. 24 m: most neighbours pass the gate
    k = PC.intrinsics(rng, B)
    tk = torch.from_numpy(k).to(gpu)
    td = _view(gpu, rng, z, 3, 5.0)[:, None]
    valid = PC.valid_ref(z)
    total = int(valid.sum())
    for kw in (dict(), dict(jump_rel=0.0, jump_abs=0.0)):
        ref = NC.normals_ref(z, k, **kw)
        pc = _check_packed(P, gpu, td, tk, ref, valid, with_index=True, **kw)
        # the rows are the map's, gathered on the device at the cloud's own index
        m = P.normals(td, tk, **kw).permute(0, 2, 3, 1).reshape(-1, 3)[pc.index[:total].long()]
        assert torch.equal(_bits(torch.nan_to_num(m, nan=0.0)), _bits(pc.normals[:total]))
        assert torch.equal(_bits(pc.image_normals(1)), _bits(pc.normals[pc.host_offsets()[1]:pc.host_offsets()[2]]))
    ref = NC.normals_ref(z, k)
    for cap in (total // 2, 1, 0):  # a capacity below the count: the rows beyond it keep their sentinel
        pc = _check_packed(P, gpu, td, tk, ref, valid, cap=cap)
        assert pc.truncated() == (total > cap)
    # a confidence gate reaches the packed normals as it reaches the map
    conf = rng.choice(np.array([0.25, 0.75, np.nan], dtype=np.float32), (B, H, W), p=[0.2, 0.7, 0.1])
    tc = torch.from_numpy(conf).to(gpu)[:, None]
    _check_packed(P, gpu, td, tk, NC.normals_ref(z, k, conf=conf, conf_min=0.5), PC.valid_ref(z, conf, 0.5),
                  conf=tc, conf_min=0.5)


def test_points_entry_with_a_handmade_index(nconv_amd, gpu):
    """nconv_depth_normals_points itself: indices outside [0, B * H * W) give zeros and read nothing,
    rows from min(offsets[B], capacity) on are not written, a capacity of 0 launches nothing."""
    L, P = nconv_amd._lib, nconv_amd.pointcloud
    rng = np.random.default_rng(71)
    B, H, W = 2, 4, 37
    z = rng.uniform(10.0, 11.0, (B, H, W)).astype(np.float32)
    k = PC.intrinsics(rng)
    ref = NC.normals_ref(z, k)
    td, tk = _view(gpu, rng, z, 2, 5.0)[:, None], torch.from_numpy(k).to(gpu)
    total = B * H * W
    index = np.array([-1, total, 5, W + 5, total - 1, -2 ** 31, 2 ** 31 - 1, (H + 1) * W + 7, 0, 40, 41, 42], dtype=np.int32)
    inside = (index >= 0) & (index < total)
    want = np.zeros((len(index), 3), dtype=np.float32)
    want[inside] = NC.packed_ref(ref, index[inside])
    assert (want[inside] != 0).any()
    d, _ = P._descriptor(td, tk, None, 0.0, 0.0, PC.FLT_MAX)
    o = P._normals_opts(0.1, 0.0)
    t_idx = torch.from_numpy(index).to(gpu)
    call = lambda off, cap, nrm: L.lib().nconv_depth_normals_points(
        ctypes.byref(d), ctypes.byref(o), L.ptr(t_idx), L.ptr(off), cap, L.ptr(nrm), L.stream_handle(gpu))
    for count, cap in ((len(index), len(index)), (len(index) - 3, len(index)), (len(index) + 50, len(index) - 2),
                       (0, len(index))):
        off = torch.tensor([0, count // 2, count], dtype=torch.int32, device=gpu)
        whole, nrm = _guarded(gpu, (len(index), 3), S_F32, torch.float32)
        assert call(off, cap, nrm) == 0
        torch.cuda.synchronize()
        n = min(count, cap)
        assert _same(nrm[:n], want[:n]) and bool((nrm[n:] == S_F32).all()) and _intact(whole, S_F32)
    whole, nrm = _guarded(gpu, (len(index), 3), S_F32, torch.float32)
    off = torch.tensor([0, 6, 12], dtype=torch.int32, device=gpu)
    assert call(off, 0, nrm) == 0
    torch.cuda.synchronize()
    assert bool((whole == S_F32).all())


def test_captured_in_a_graph(nconv_amd, gpu):
    """normals, normal_image and backproject(normals=True) into static buffers, captured in one
    hipGraph on a single stream and replayed after the depth is rewritten in place: the reference of the
    new depth."""
    P = nconv_amd.pointcloud
    rng = np.random.default_rng(81)
    B, H, W = 2, 9, 300
    k = PC.intrinsics(rng, B)
    tk = torch.from_numpy(k).to(gpu)
    new = lambda: PC.depth_values(rng, B, H, W, "p50")
    s_z = torch.from_numpy(new()).to(gpu)[:, None]
    cap = B * H * W
    out = {"xyz": torch.zeros(cap, 3, device=gpu), "index": torch.zeros(cap, dtype=torch.int32, device=gpu),
           "normals": torch.zeros(cap, 3, device=gpu), "offsets": torch.zeros(B + 1, dtype=torch.int32, device=gpu),
           "workspace": torch.zeros(P.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)}
    m_out = torch.zeros(B, 3, H, W, device=gpu)
    i_out = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=gpu)
    P.normals(s_z, tk, out=m_out)  # library loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        P.normals(s_z, tk, out=m_out)
        P.normal_image(s_z, tk, empty=EMPTY, out=i_out)
        P.backproject(s_z, tk, normals=True, out=out)
    for _ in range(2):
        z1 = new()
        s_z.copy_(torch.from_numpy(z1)[:, None])
        out["normals"].fill_(S_F32)
        g.replay()
        torch.cuda.synchronize()
        ref = NC.normals_ref(z1, k)
        index = np.flatnonzero(PC.valid_ref(z1).reshape(-1))
        n = len(index)
        assert _same(m_out, ref) and torch.equal(i_out.cpu(), torch.from_numpy(NC.picture_ref(ref, EMPTY)))
        assert int(out["offsets"][-1]) == n
        assert _same(out["normals"][:n], NC.packed_ref(ref, index)) and bool((out["normals"][n:] == S_F32).all())
