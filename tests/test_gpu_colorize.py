"""GPU: visualize.colorize / Colorizer / overlay (nconv_depth_colorize, csrc/colorize.hip) against the
numpy reference of tests/colorize_cases.py, byte for byte: the sweep over sizes, window radii, ranges,
tables, channel orders and backgrounds, on strided source views and into the middle of a sentinel-filled
buffer whose guard slices must come back untouched; per-image ranges in a mixed batch; one return in a
corner; launch counts and the absence of a synchronisation; hipGraph capture; compat save_depth on a
device tensor; one full-size call."""
import importlib.util
import os
import sys
import time

import numpy as np
import pytest
import torch

import colorize_cases as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


def _strided_f32(gpu, a, lead, pad):
    """a (B, H, W) on the device as a (B, 1, H, W) view `lead` elements into a NaN-filled allocation,
    rows W + pad apart, images H rows + 3 elements apart, ending exactly at the allocation's end."""
    B, H, W = a.shape
    rs = W + pad
    bs = H * rs + 3
    n = lead + (B - 1) * bs + (H - 1) * rs + W
    flat = torch.full((n,), float("nan"), device=gpu)
    v = flat.as_strided((B, 1, H, W), (bs, bs, rs, 1), lead)
    v.copy_(torch.from_numpy(a)[:, None])
    assert v.data_ptr() % 16 == 4 * lead
    return v


def _strided_u8(gpu, a, lead):
    """a (B, H, W, 3) uint8 on the device as an interleaved view `lead` bytes into a larger buffer, with
    an odd row stride and an odd image stride, ending exactly at the allocation's end."""
    B, H, W, _ = a.shape
    rs = (3 * W + 5) | 1
    bs = (H * rs + 7) | 1
    n = lead + (B - 1) * bs + (H - 1) * rs + 3 * W
    flat = torch.full((n,), 0x3C, dtype=torch.uint8, device=gpu)
    v = flat.as_strided((B, H, W, 3), (bs, rs, 3, 1), lead)
    v.copy_(torch.from_numpy(a))
    assert rs % 2 == 1 and bs % 2 == 1
    return v


def _guarded(gpu, B, H, W):
    """(buffer, middle): a (B + 2, H, W, 3) sentinel-filled buffer and its contiguous [1:1 + B] slice."""
    buf = torch.full((B + 2, H, W, 3), SENTINEL, dtype=torch.uint8, device=gpu)
    return buf, buf[1:1 + B]


def _check(nconv_amd, gpu, a, table, *, lead=0, pad=0, bg=None, overlay=False, **kw):
    """colorize of the strided view of `a` into a guarded output equals colorize_ref. table: a name or a
    (256, 3) array (uploaded as a custom table)."""
    B, H, W = a.shape
    named = isinstance(table, str)
    ref = CC.colorize_ref(a, nconv_amd.COLORMAPS[table] if named else table, background=bg, **kw)
    buf, out = _guarded(gpu, B, H, W)
    d = _strided_f32(gpu, a, lead, pad)
    cmap = table if named else torch.from_numpy(table).to(gpu)
    t_bg = None if bg is None else _strided_u8(gpu, bg, lead)
    if overlay:
        kw = {k: v for k, v in kw.items() if k != "floor"}
        got = nconv_amd.overlay(d, t_bg, cmap=cmap, out=out, **kw)
    else:
        got = nconv_amd.colorize(d, cmap=cmap, background=t_bg, out=out, **kw)
    assert got is out
    whole = buf.cpu().numpy()
    assert (whole[0] == SENTINEL).all() and (whole[-1] == SENTINEL).all()
    assert np.array_equal(whole[1:-1], ref), (a.shape, table if named else "custom", lead, pad, kw)
    return ref


# ---- the sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", CC.RADII)
@pytest.mark.parametrize("B", CC.BATCHES)
def test_sweep(nconv_amd, gpu, B, radius):
    """Every W x H of the lists (images smaller than the window among them), special values scattered
    through the planes; per shape four forms: the two ranges, floor None and 0, a builtin and a custom
    table, both channel orders, with and without a background; source offsets 0..3 elements."""
    rng = np.random.default_rng(100 * B + radius)
    case = 0
    for H in CC.HEIGHTS:
        for W in CC.WIDTHS:
            a = CC.plane(rng, B, H, W)
            bg = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
            name = CC.CMAPS[case % len(CC.CMAPS)]
            lead, pad = case % 4, (0, 1, 4, 7)[(case // 4) % 4]
            case += 1
            _check(nconv_amd, gpu, a, name, lead=lead, pad=pad, radius=radius)
            _check(nconv_amd, gpu, a, CC.custom_table(rng), lead=lead, pad=pad, radius=radius, vmin=5.0, vmax=60.0,
                   floor=0.0, order="bgr", bg=bg)
            _check(nconv_amd, gpu, a, name, lead=(lead + 1) % 4, pad=pad, radius=radius, floor=0.0, bg=bg)
            _check(nconv_amd, gpu, a, name, lead=lead, pad=pad, radius=radius, vmin=-10.0, vmax=40.0, order="bgr",
                   empty=(1, 2, 3))


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("name", CC.CMAPS)
def test_every_builtin_table(nconv_amd, gpu, name, order):
    """A ramp that reaches all 256 entries: the picture is the table itself."""
    a = np.arange(256, dtype=np.float32).reshape(1, 4, 64)
    ref = _check(nconv_amd, gpu, a, name, order=order)
    t = nconv_amd.COLORMAPS[name]
    assert np.array_equal(ref.reshape(256, 3), t[:, ::-1] if order == "bgr" else t)
    _check(nconv_amd, gpu, a, name, order=order, vmin=0.0, vmax=255.0, radius=1)


def test_ties_and_clamps(nconv_amd, gpu):
    """s == 1: k + 0.5 for every k, values beyond both ends, huge and non-finite values."""
    k = np.arange(256, dtype=np.float32)
    a = np.concatenate([k + 0.5, k, [-4.0, 300.0, 1e30, -1e30, np.nan, np.inf, -np.inf, -0.0]]).astype(np.float32)
    a = a.reshape(1, 8, 65)
    ref = _check(nconv_amd, gpu, a, "gray", vmin=0.0, vmax=255.0, empty=(9, 8, 7))
    want = np.rint(k + 0.5)
    want[want > 255] = 255
    assert np.array_equal(ref.reshape(-1, 3)[:256, 0], want.astype(np.uint8))
    # a range whose width overflows: s = 0, every index 0
    _check(nconv_amd, gpu, a, "turbo", vmin=-3e38, vmax=3e38)
    _check(nconv_amd, gpu, a, "turbo", vmin=5.0, vmax=5.0)
    _check(nconv_amd, gpu, a, "turbo", vmin=9.0, vmax=2.0, radius=2)


# ---- ranges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 2])
def test_batch_mix_keeps_ranges_apart(nconv_amd, gpu, radius):
    """An all-empty image, a constant image and a normal image in one batch, in every order."""
    rng = np.random.default_rng(5)
    H, W = 9, 67
    normal = CC.plane(rng, 1, H, W)[0]
    empty = np.where(rng.random((H, W)) < 0.5, np.float32(np.nan), np.float32(0.0))
    const = np.full((H, W), 7.25, dtype=np.float32)
    alone = CC.colorize_ref(normal[None], nconv_amd.COLORMAPS["inferno"], floor=0.0, radius=radius, empty=(3, 2, 1))
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        a = np.stack([(empty, const, normal)[q] for q in order])
        ref = _check(nconv_amd, gpu, a, "inferno", floor=0.0, radius=radius, empty=(3, 2, 1))
        assert np.array_equal(ref[order.index(2)], alone[0])
        assert (ref[order.index(0)] == np.array([3, 2, 1])).all()
        assert (ref[order.index(1)] == nconv_amd.COLORMAPS["inferno"][0]).all()


def test_second_call_carries_nothing_of_the_first(nconv_amd, gpu):
    """The same output and workspace for a wide range, then a narrow one."""
    rng = np.random.default_rng(6)
    B, H, W = 2, 9, 17
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=gpu)
    ws = torch.empty(nconv_amd.visualize.workspace_bytes(B), dtype=torch.uint8, device=gpu)
    for lo, hi in ((-100.0, 1000.0), (10.0, 11.0)):
        a = rng.uniform(lo, hi, (B, H, W)).astype(np.float32)
        got = nconv_amd.colorize(torch.from_numpy(a).to(gpu)[:, None], out=out, workspace=ws)
        assert got is out
        assert np.array_equal(got.cpu().numpy(), CC.colorize_ref(a, nconv_amd.COLORMAPS["inferno"]))


@pytest.mark.parametrize("corner", [(0, 0), (0, 16), (8, 0), (8, 16)])
def test_one_return_in_a_corner(nconv_amd, gpu, corner):
    a = np.zeros((1, 9, 17), dtype=np.float32)
    a[0][corner] = 12.5
    bg = np.random.default_rng(7).integers(0, 256, (1, 9, 17, 3)).astype(np.uint8)
    ref = _check(nconv_amd, gpu, a, "viridis", floor=0.0, radius=4, bg=bg, overlay=True)
    drawn = (ref != bg).any(axis=-1)[0]
    assert drawn.sum() >= 24 and drawn[corner]  # a 5 x 5 square clipped at the corner; the background may coincide
    assert (ref[0][drawn] == nconv_amd.COLORMAPS["viridis"][0]).all()


def test_overlay_default_radius(nconv_amd, gpu):
    rng = np.random.default_rng(8)
    a = CC.plane(rng, 2, 9, 68, fill=0.05, special=False)
    bg = rng.integers(0, 256, (2, 9, 68, 3)).astype(np.uint8)  # rows of 204 bytes: the 96-bit background loads
    got = nconv_amd.overlay(torch.from_numpy(a).to(gpu)[:, None], torch.from_numpy(bg).to(gpu))
    ref = CC.colorize_ref(a, nconv_amd.COLORMAPS["inferno"], floor=0.0, radius=1, background=bg)
    assert np.array_equal(got.cpu().numpy(), ref)
    # (H, W) and (1, H, W) planes are one image
    for d in (torch.from_numpy(a[0]).to(gpu), torch.from_numpy(a[:1]).to(gpu)):
        got = nconv_amd.colorize(d, floor=0.0)
        assert got.shape == (1, 9, 68, 3)
        assert np.array_equal(got.cpu().numpy(), CC.colorize_ref(a[:1], nconv_amd.COLORMAPS["inferno"], floor=0.0))


# ---- launches ----------------------------------------------------------------------------------------
def _device_events(fn):
    """The device-side events (kernels, memsets, copies) of fn(), by name."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_launch_counts(nconv_amd, gpu):
    rng = np.random.default_rng(9)
    B, H, W = 2, 9, 67
    d = torch.from_numpy(CC.plane(rng, B, H, W)).to(gpu)[:, None]
    bg = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)).to(gpu)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=gpu)
    ws = torch.empty(nconv_amd.visualize.workspace_bytes(B), dtype=torch.uint8, device=gpu)
    nconv_amd.colorize(d, out=out, workspace=ws)  # library and code objects loaded
    for radius in (0, 2):
        auto = _device_events(lambda: nconv_amd.colorize(d, radius=radius, background=bg, out=out, workspace=ws))
        fixed = _device_events(lambda: nconv_amd.colorize(d, radius=radius, background=bg, vmin=0.0, vmax=80.0,
                                                          out=out))
        print(f"radius {radius}: auto {auto}, fixed {fixed}")
        assert 1 <= len(auto) <= 3, auto
        assert len(fixed) == 1 and "colorize_map" in fixed[0], fixed
        assert any("colorize_map" in n for n in auto), auto


def test_call_does_not_synchronise(nconv_amd, gpu):
    """Behind tens of milliseconds of queued work the call returns while that work is still running: an
    event recorded before the call has not completed when the call is back."""
    rng = np.random.default_rng(10)
    B, H, W = 2, 9, 67
    a = CC.plane(rng, B, H, W)
    d = torch.from_numpy(a).to(gpu)[:, None]
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=gpu)
    ws = torch.empty(nconv_amd.visualize.workspace_bytes(B), dtype=torch.uint8, device=gpu)
    nconv_amd.colorize(d, out=out, workspace=ws)
    busy = torch.zeros(1 << 28, device=gpu)  # 1 GiB: each pass over it moves 2 GiB
    busy.add_(1.0)
    torch.cuda.synchronize()
    before = torch.cuda.Event()
    for _ in range(60):
        busy.add_(1.0)
    before.record()
    t0 = time.perf_counter()
    got = nconv_amd.colorize(d, radius=1, floor=0.0, out=out, workspace=ws)
    back = time.perf_counter() - t0
    still_running = not before.query()
    torch.cuda.synchronize()
    print(f"colorize returned after {back * 1e6:.0f} us; queued work still running: {still_running}")
    assert still_running
    assert np.array_equal(got.cpu().numpy(), CC.colorize_ref(a, nconv_amd.COLORMAPS["inferno"], floor=0.0, radius=1))


# ---- hipGraph ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
def test_captured_in_a_graph(nconv_amd, gpu, fixed):
    """A Colorizer captured once and replayed on depth and background refilled in place equals the
    reference each time: no allocation, no synchronisation, nothing kept between calls."""
    rng = np.random.default_rng(11)
    B, H, W = 3, 9, 67
    opts = dict(cmap="magma", floor=0.0, radius=1, order="bgr")
    if fixed:
        opts.update(vmin=2.0, vmax=50.0)
    col = nconv_amd.Colorizer((H, W), B=B, **opts)
    d = torch.zeros(B, 1, H, W, device=gpu)
    bg = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=gpu)
    first = col(d, bg)  # library loaded, output and workspace allocated before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = col(d, bg)
    assert res is first
    ref_opts = {k: v for k, v in opts.items() if k != "cmap"}
    for _ in range(2):
        a = CC.plane(rng, B, H, W) * np.float32(rng.uniform(0.5, 2.0))
        b = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
        d.copy_(torch.from_numpy(a)[:, None])
        bg.copy_(torch.from_numpy(b))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), CC.colorize_ref(a, nconv_amd.COLORMAPS["magma"], background=b, **ref_opts))


# ---- save_depth --------------------------------------------------------------------------------------
def test_save_depth_device_tensor(nconv_amd, gpu, tmp_path):
    from PIL import Image
    path = os.path.join(ROOT, "compat")
    sys.path.insert(0, path)
    saved = {k: sys.modules.get(k) for k in ("dataset", "dataset.kittiloader")}
    try:
        for k in saved:
            sys.modules.pop(k, None)
        spec = importlib.util.spec_from_file_location("compat_utils_under_test", os.path.join(path, "utils.py"))
        utils = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(utils)
    finally:
        sys.path.remove(path)
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v
    rng = np.random.default_rng(12)
    a = rng.uniform(0.0, 80.0, (1, 37, 71)).astype(np.float32)
    p = str(tmp_path / "d.png")
    full = torch.from_numpy(np.pad(a, ((0, 0), (1, 2), (1, 3)))).to(gpu)
    # the reference's call: a cropped (1, H, W) slice of the model's output
    for t, kw, name in ((full[:, 1:38, 1:72], {}, "inferno"), (full[0, 1:38, 1:72], dict(cmap="viridis"), "viridis")):
        utils.save_depth(t, p, **kw)
        img = Image.open(p)
        assert img.mode == "RGB" and np.array_equal(np.asarray(img), CC.colorize_ref(a, nconv_amd.COLORMAPS[name])[0])


# ---- full size ---------------------------------------------------------------------------------------
def test_full_size_overlay(nconv_amd, gpu):
    """352 x 1216, B = 2, radius 1 over a background: rows of five tiles, 44 tile rows per image."""
    rng = np.random.default_rng(13)
    B, H, W = 2, 352, 1216
    a = CC.plane(rng, B, H, W, fill=0.05)
    bg = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    d, t_bg = torch.from_numpy(a).to(gpu)[:, None], torch.from_numpy(bg).to(gpu)
    ref = CC.colorize_ref(a, nconv_amd.COLORMAPS["inferno"], floor=0.0, radius=1, background=bg)
    nconv_amd.overlay(d[:1], t_bg[:1])  # code objects loaded
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = nconv_amd.overlay(d, t_bg)
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    print(f"overlay at {B} x {H} x {W}: {took * 1e3:.3f} ms")
    assert np.array_equal(got.cpu().numpy(), ref)
    assert took < 0.25  # "well under a second": the call moves 12 MB
