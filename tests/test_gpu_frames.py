"""GPU: nconv_frame_ingest / nconv_depth_export_u16 (csrc/frame_io.hip) against the numpy reference
of frames_cases. The arithmetic is exact, so every comparison is torch.equal. Sources are slices of
larger allocations (every base alignment, odd row strides), outputs the middle slice of a larger
sentinel-filled buffer whose guard slices must come back untouched."""
import numpy as np
import pytest
import torch

import frames_cases as FC

pytestmark = pytest.mark.gpu


def _dev(big, view_of, dev):
    """The numpy allocation on the device and the same slice of it as `view_of` takes from big."""
    t = torch.from_numpy(big).to(dev)
    return t, view_of(t)


def _guarded(dev, shape, dtype=torch.float32):
    """(buffer, middle): a (B + 2, ...) sentinel-filled buffer and its contiguous [1:1+B] slice."""
    B = shape[0]
    if dtype == torch.float32:
        buf = torch.full((B + 2,) + tuple(shape[1:]), float("nan"), device=dev)
    else:
        buf = torch.from_numpy(np.full((B + 2,) + tuple(shape[1:]), 0xA5C3, dtype=np.uint16)).to(dev)
    return buf, buf[1:1 + B]


def _guards_intact(buf, dtype=torch.float32):
    g = torch.cat([buf[0].reshape(-1), buf[-1].reshape(-1)]).cpu()
    return bool(torch.isnan(g).all()) if dtype == torch.float32 else bool((g.view(torch.int16) == -23101).all())


def _check_ingest(F, dev, srcs, ref_kw, **kw):
    """ingest(**srcs) into guarded outputs == ingest_ref(**ref_kw); the returned tensors are the outs."""
    ref = FC.ingest_ref(**ref_kw)
    bufs = {k: _guarded(dev, v.shape) for k, v in ref.items()}
    got = F.ingest(**srcs, out={k: m for k, (_, m) in bufs.items()}, **kw)
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert got[k].data_ptr() == bufs[k][1].data_ptr()
        assert torch.equal(got[k].cpu(), torch.from_numpy(v)), (k, kw)
        assert _guards_intact(bufs[k][0]), (k, kw)


@pytest.mark.parametrize("w", FC.INGEST_W)
def test_ingest_sweep(nconv_amd, gpu, w):
    """B x h x left for one width: rgb + depth + gt, rgb alone and the planes alone (in the other
    slots), the plane dtype, the decode and reverse_rgb cycling over the cases."""
    F = nconv_amd.frames
    rng = np.random.default_rng(100 + w)
    n = 0
    for B in FC.INGEST_B:
        for h in FC.INGEST_H:
            for left in FC.INGEST_LEFT:
                cut = lambda t: t[:, 1:1 + h, left:left + w]
                dt = FC.PLANE_DTYPES[n % 3]
                decode = ("reference", "kitti16", (0, 0.75) if dt == np.float32 else (5, 0.75))[(n // 3) % 3]
                rev = bool(n % 2)
                rgb_big, rgb = FC.raw_allocation(rng, B, h, w, left, np.uint8, channels=3)
                d_big, d = FC.raw_allocation(rng, B, h, w, left, np.uint16)
                g_big, g = FC.raw_allocation(rng, B, h, w, left, dt)
                _, trgb = _dev(rgb_big, cut, gpu)
                _, td = _dev(d_big, cut, gpu)
                _, tg = _dev(g_big, cut, gpu)
                _check_ingest(F, gpu, dict(rgb=trgb, depth=td, gt=tg), dict(rgb=rgb, depth=d, gt=g, depth_decode=decode,
                                                                           reverse_rgb=rev),
                              depth_decode=decode, reverse_rgb=rev)
                _check_ingest(F, gpu, dict(rgb=trgb), dict(rgb=rgb, reverse_rgb=not rev), reverse_rgb=not rev)
                _check_ingest(F, gpu, dict(depth=tg, gt=td), dict(depth=g, gt=d, depth_decode=decode),
                              depth_decode=decode)
                n += 1


@pytest.mark.parametrize("decode", ["reference", "kitti16", (3, 0.375), (0, 1.0 / 256.0)])
@pytest.mark.parametrize("dtype", FC.PLANE_DTYPES)
def test_ingest_each_dtype_and_decode(nconv_amd, gpu, dtype, decode):
    """Every source dtype under every decode, aligned (contiguous, w % 4 == 0: the wide loads) and
    sliced; (B, 1, h, w) sources; fresh outputs when no out is given."""
    F = nconv_amd.frames
    if dtype == np.float32 and not isinstance(decode, str):
        decode = (0, decode[1])
    rng = np.random.default_rng(7)
    for (B, h, w, left) in ((3, 17, 64, 0), (3, 17, 65, 1)):
        big, v = FC.raw_allocation(rng, B, h, w, left, dtype)
        ref = FC.plane_ref(v, *FC.decode_of(decode, dtype))
        t = torch.from_numpy(big).to(gpu)[:, 1:1 + h, left:left + w]
        assert torch.equal(F.ingest(depth=t, depth_decode=decode)["depth"].cpu(), torch.from_numpy(ref))
        c = torch.from_numpy(np.ascontiguousarray(v)).to(gpu)
        got = F.ingest(gt=c[:, None], depth_decode=decode)
        assert set(got) == {"gt"} and got["gt"].shape == (B, 1, h, w) and got["gt"].dtype == torch.float32
        assert torch.equal(got["gt"].cpu(), torch.from_numpy(ref))


def test_ingest_values_cover_the_special_ones(nconv_amd, gpu):
    """0, 255, 256 and 65535 under both decodes, and every byte value, on one small frame."""
    F = nconv_amd.frames
    v = np.array([0, 255, 256, 65535, 257, 32768, 65280, 1], dtype=np.uint16).reshape(1, 2, 4)
    t = torch.from_numpy(v).to(gpu)
    for decode in ("reference", "kitti16"):
        got = F.ingest(depth=t, depth_decode=decode)["depth"].cpu()
        assert torch.equal(got, torch.from_numpy(FC.plane_ref(v, *FC.decode_of(decode, np.uint16))))
    assert F.ingest(depth=t, depth_decode="kitti16")["depth"].reshape(-1)[:4].tolist() == [0.0, 255 / 256, 1.0,
                                                                                           65535 / 256]
    rgb = np.arange(256 * 3, dtype=np.int64).reshape(1, 4, 64, 3).astype(np.uint8)
    got = F.ingest(rgb=torch.from_numpy(rgb).to(gpu), reverse_rgb=False)["rgb"].cpu()
    assert torch.equal(got, torch.from_numpy(FC.rgb_ref(rgb, reverse=False)))


@pytest.mark.parametrize("off,w,rs", [(1, 5, 17), (4, 5, 16), (0, 16, 48), (3, 17, 51)])
def test_ingest_view_ending_at_the_allocations_last_byte(nconv_amd, gpu, off, w, rs):
    """Sources whose last byte is the allocation's last byte: RGB (unaligned base; aligned base and
    strides with a row tail) and a uint16 plane behind an odd number of elements."""
    F = nconv_amd.frames
    rng = np.random.default_rng(off + w)
    B, h = 2, 3
    bs = h * rs + 4
    n = off + (B - 1) * bs + (h - 1) * rs + 3 * w
    flat = rng.integers(0, 256, n, dtype=np.int64).astype(np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[off:], (B, h, w, 3), (bs, rs, 3, 1))
    t = torch.from_numpy(flat).to(gpu)
    tv = t.as_strided((B, h, w, 3), (bs, rs, 3, 1), off)
    assert tv.data_ptr() + (B - 1) * bs + (h - 1) * rs + 3 * w == t.data_ptr() + t.numel()
    _check_ingest(F, gpu, dict(rgb=tv), dict(rgb=view))
    # uint16: strides in elements
    es, eb = rs, h * rs + 1
    n = off + (B - 1) * eb + (h - 1) * es + w
    flat = rng.integers(0, 65536, n, dtype=np.int64).astype(np.uint16)
    view = np.lib.stride_tricks.as_strided(flat[off:], (B, h, w), (2 * eb, 2 * es, 2))
    t = torch.from_numpy(flat).to(gpu)
    tv = t.as_strided((B, h, w), (eb, es, 1), off)
    assert tv.data_ptr() + 2 * ((B - 1) * eb + (h - 1) * es + w) == t.data_ptr() + 2 * t.numel()
    _check_ingest(F, gpu, dict(depth=tv), dict(depth=view, depth_decode="kitti16"), depth_decode="kitti16")


def test_ingest_geometry_errors(nconv_amd, gpu):
    F = nconv_amd.frames
    z16 = lambda *shape: torch.from_numpy(np.zeros(shape, dtype=np.uint16)).to(gpu)
    d = z16(2, 4, 8)
    with pytest.raises(ValueError, match="gt"):
        F.ingest(depth=d, gt=z16(2, 4, 9))
    with pytest.raises(ValueError, match="depth"):
        F.ingest(depth=z16(2, 4, 16)[:, :, ::2])
    with pytest.raises(TypeError):
        F.ingest(depth=d, out={"depth": torch.zeros(2, 1, 8, 4, device=gpu).transpose(2, 3)})
    with pytest.raises(RuntimeError, match="shift"):
        F.ingest(depth=d, depth_decode=(16, 1.0))


@pytest.mark.parametrize("W", FC.EXPORT_W)
def test_export_sweep(nconv_amd, gpu, W):
    """B x H for one width, contiguous and as the cropped view big[:, :, 1:1+H, 1:1+W], with ties,
    -0.0, negatives, overflow, +-inf and NaN among the values."""
    F = nconv_amd.frames
    rng = np.random.default_rng(200 + W)
    for B in FC.EXPORT_B:
        for H in FC.EXPORT_H:
            d = FC.export_values(rng, B, H, W)
            ref = torch.from_numpy(FC.export_ref(d, 256.0))
            plain = torch.from_numpy(d).to(gpu)
            big = torch.full((B, 1, H + 2, W + 3), 7.0, device=gpu)
            crop = big[:, :, 1:1 + H, 1:1 + W]
            crop.copy_(plain)
            for src in (plain, crop):
                buf, out = _guarded(gpu, (B, 1, H, W), torch.uint16)
                got = F.export_depth16(src, out=out)
                assert got.data_ptr() == out.data_ptr() and got.dtype == torch.uint16
                assert torch.equal(got.cpu(), ref), (B, H, W, src.is_contiguous())
                assert _guards_intact(buf, torch.uint16)
            fresh = F.export_depth16(crop)
            assert fresh.shape == (B, 1, H, W) and fresh.is_contiguous() and torch.equal(fresh.cpu(), ref)
            # another scale: the product is one fp32 rounding
            assert torch.equal(F.export_depth16(plain, scale=1000.0).cpu(), torch.from_numpy(FC.export_ref(d, 1000.0)))
            if B == 1:  # (H, W) and (1, H, W) operands are the same plane
                assert torch.equal(F.export_depth16(plain[0, 0]).cpu(), ref[0, 0])
                assert torch.equal(F.export_depth16(crop[0]).cpu(), ref[0])


def test_export_all_special_values(nconv_amd, gpu):
    d = np.tile(FC.EXPORT_SPECIAL, 3).reshape(1, 1, 1, -1)
    got = nconv_amd.export_depth16(torch.from_numpy(d).to(gpu)).cpu()
    assert torch.equal(got, torch.from_numpy(FC.export_ref(d)))
    k = len(FC.EXPORT_SPECIAL)
    assert got.reshape(-1)[:k].tolist() == FC.export_ref(FC.EXPORT_SPECIAL).tolist()
    assert got.reshape(-1)[:4].tolist() == [2, 4, 0, 2]  # ties go to the even neighbour


def test_ingest_then_export_captured_in_a_graph(nconv_amd, gpu):
    """ingest (static out) followed by export_depth16 on one of its outputs, captured in a hipGraph
    and replayed on new source bytes, equals the eager result."""
    F = nconv_amd.frames
    rng = np.random.default_rng(9)
    B, h, w = 2, 17, 65
    new = lambda: (rng.integers(0, 256, (B, h, w, 3), dtype=np.int64).astype(np.uint8),
                   rng.integers(0, 65536, (B, h, w), dtype=np.int64).astype(np.uint16))
    rgb0, d0 = new()
    s_rgb, s_d = torch.from_numpy(rgb0).to(gpu), torch.from_numpy(d0).to(gpu)
    out = {"rgb": torch.zeros(B, 3, h, w, device=gpu), "depth": torch.zeros(B, 1, h, w, device=gpu)}
    u16 = torch.from_numpy(np.zeros((B, 1, h, w), dtype=np.uint16)).to(gpu)
    F.ingest(rgb=s_rgb, depth=s_d, depth_decode="kitti16", out=out)  # library loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F.ingest(rgb=s_rgb, depth=s_d, depth_decode="kitti16", out=out)
        F.export_depth16(out["depth"], out=u16)
    for _ in range(2):
        rgb1, d1 = new()
        s_rgb.copy_(torch.from_numpy(rgb1))
        s_d.copy_(torch.from_numpy(d1))
        g.replay()
        torch.cuda.synchronize()
        eager = F.ingest(rgb=s_rgb, depth=s_d, depth_decode="kitti16")
        assert torch.equal(out["rgb"], eager["rgb"]) and torch.equal(out["depth"], eager["depth"])
        assert torch.equal(out["rgb"].cpu(), torch.from_numpy(FC.rgb_ref(rgb1)))
        assert torch.equal(u16.cpu(), F.export_depth16(eager["depth"]).cpu())
        # kitti16 then x 256: the stored values come back
        assert torch.equal(u16.cpu(), torch.from_numpy(d1[:, None]))


def test_end_to_end_model_on_ingested_frame(nconv_amd, gpu):
    """SETP1_NCONV on ingest of a uint16 frame == the same model on the host-converted fp32 tensor,
    bit for bit; export_depth16 of the result == export_ref."""
    torch.manual_seed(0)
    net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu).eval()
    rng = np.random.default_rng(4)
    v = (rng.integers(256, 20000, (2, 32, 48)) * (rng.random((2, 32, 48)) < 0.2)).astype(np.uint16)
    host = torch.from_numpy(FC.plane_ref(v, 0, 1.0 / 256.0))
    with torch.no_grad():
        want = net(host.to(gpu))
        dev_in = nconv_amd.ingest(depth=torch.from_numpy(v).to(gpu), depth_decode="kitti16")["depth"]
        assert torch.equal(dev_in.cpu(), host)
        got = net(dev_in)
    assert got.shape == want.shape and torch.equal(got, want)
    pred = got[:, :1] if got.shape[1] != 1 else got
    u16 = nconv_amd.export_depth16(pred)
    assert torch.equal(u16.cpu(), torch.from_numpy(FC.export_ref(pred.cpu().numpy())))
    assert int(u16.cpu().view(torch.int16).ne(0).sum()) > 0


def test_prefetcher_with_ingest_yields_the_host_converted_batches(nconv_amd, gpu):
    """A DataLoader of raw samples (10, batch 4) through DevicePrefetcher(..., ingest=Ingest()):
    the same batches, in order, as the host conversion; non-tensor entries pass through."""
    rng = np.random.default_rng(6)
    N, h, w = 10, 6, 20
    rgb = rng.integers(0, 256, (N, h, w, 3), dtype=np.int64).astype(np.uint8)
    dep = rng.integers(0, 65536, (N, h, w), dtype=np.int64).astype(np.uint16)
    gt = rng.integers(0, 65536, (N, h, w), dtype=np.int64).astype(np.uint16)

    class Raw(torch.utils.data.Dataset):
        def __len__(self):
            return N

        def __getitem__(self, i):
            return {"rgb": torch.from_numpy(rgb[i]), "depth": torch.from_numpy(dep[i]), "gt": torch.from_numpy(gt[i]),
                    "k": torch.full((3, 3), float(i)), "name": f"frame{i}", "idx": i}

    loader = torch.utils.data.DataLoader(Raw(), batch_size=4, shuffle=False)
    pre = nconv_amd.data.DevicePrefetcher(loader, gpu, ingest=nconv_amd.Ingest())
    assert len(pre) == 3
    seen = 0
    for batch in pre:
        n = batch["rgb"].shape[0]
        sl = slice(seen, seen + n)
        ref = FC.ingest_ref(rgb=rgb[sl], depth=dep[sl], gt=gt[sl])
        for k in ("rgb", "depth", "gt"):
            assert batch[k].device == gpu and batch[k].dtype == torch.float32
            assert torch.equal(batch[k].cpu(), torch.from_numpy(ref[k])), (k, seen)
        assert batch["k"].device == gpu and batch["k"][:, 0, 0].tolist() == [float(i) for i in range(seen, seen + n)]
        assert batch["name"] == [f"frame{i}" for i in range(seen, seen + n)]
        assert batch["idx"].tolist() == list(range(seen, seen + n)) and batch["idx"].device.type == "cpu"
        seen += n
    assert seen == N
    # without ingest the raw integers arrive as they are (today's behaviour for today's callers)
    b0 = next(iter(nconv_amd.data.DevicePrefetcher(loader, gpu)))
    assert b0["rgb"].dtype == torch.uint8 and b0["depth"].dtype == torch.uint16
