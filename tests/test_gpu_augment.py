"""GPU: nconv_frame_augment against the numpy reference (tests/augment_cases.py) bit for bit, every output
inside a guard band: the geometry sweep with every crop mode pair, every flip setting, all tensors and
each one alone; strided, misaligned and shared views; the jitter, its clamp and the reported gains
against the C host's; KITTI size; determinism; Augmenter under torch.cuda.graph; Augment behind
DevicePrefetcher; refusals."""
import itertools

import numpy as np
import pytest
import torch

import augment_cases as AC
import frames_cases as FC
import host_harness
import sparsify_cases as SC

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
GUARD = {torch.float32: -7.0, torch.uint8: 0x5A, torch.int32: -77}
MODE_NAMES = ("random", "center", "min", "max")
MODE_PAIRS = tuple(itertools.product(MODE_NAMES, MODE_NAMES))
JITTER = dict(brightness=0.2, contrast=0.2, color=0.2)


def _sources(B, H, W, seed, shared_mask=False):
    m = AC.mask_u8(B, H, W, seed + 3)
    return dict(rgb=AC.image(B, H, W, seed), depth=AC.plane(B, H, W, seed + 1), gt=AC.plane(B, H, W, seed + 2, density=0.9),
                extra=AC.plane(B, H, W, seed + 5, density=1.0), mask=m[0] if shared_mask else m, k=AC.intrinsics(B, H, W, seed + 4))


def _plane_view(gpu, z, off):
    """z (B, C, H, W) as a window of a larger buffer of other values: row stride W + 5, a channel stride
    that skips every other plane where C > 1, the first element `off` elements past a 16-byte boundary."""
    B, C, H, W = z.shape
    cc, hh, ww = (2 * C - 1, H + 3, W + 5)
    t = torch.from_numpy(z)
    fill = 99 if t.dtype == torch.uint8 else 123.0
    lead = (off - ww - 2) % (16 // t.element_size())
    whole = torch.full((B * cc * hh * ww + lead + 3,), fill, dtype=t.dtype, device=gpu)
    big = whole[lead:lead + B * cc * hh * ww].view(B, cc, hh, ww)
    v = big[:, ::2, 1:1 + H, 2:2 + W]
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() * off
    return v


def _to_device(gpu, src, views):
    """The keyword arguments of augment for the numpy sources; views: strided windows, the fp32 bases one
    element off a 16-byte boundary and the mask at an odd byte offset."""
    kw = {}
    for n, a in src.items():
        if n == "k":
            kw[n] = torch.from_numpy(a).to(gpu)
        elif n == "mask" and a.ndim == 2:
            kw[n] = _plane_view(gpu, a[None, None], 3)[0, 0] if views else torch.from_numpy(a).to(gpu)
        else:
            a4 = a if a.ndim == 4 else a[:, None]
            kw[n] = _plane_view(gpu, a4, 3 if n == "mask" else 1) if views else torch.from_numpy(a4).to(gpu)
    if views and "mask" in kw:
        assert kw["mask"].data_ptr() % 4 == 3
    if views and "rgb" in kw:
        assert kw["rgb"].stride(1) > src["rgb"].shape[2] * kw["rgb"].stride(2)
    return kw


def _guarded(gpu, shape, dtype, lead):
    n = int(np.prod(shape))
    whole = torch.full((n + lead + 5,), GUARD[dtype], dtype=dtype, device=gpu)
    return whole, whole[lead:lead + n].view(shape)


def _run(nconv_amd, gpu, size, src, *, views=False, lead=0, check=True, **kw):
    """One call with every output inside a guard band; returns the outputs as numpy, (B, h, w) planes."""
    h, w = size
    dev = _to_device(gpu, src, views)
    B = next(t.shape[0] if t.dim() > 2 else 1 for n, t in dev.items() if not (n == "mask" and t.dim() == 2))
    wholes, out = {}, {}
    for n in list(dev) + ["params", "gains"]:
        shape = {"k": (B, 3, 3), "params": (B, 4), "gains": (B, 5), "rgb": (B, 3, h, w)}.get(n, (B, 1, h, w))
        dtype = torch.uint8 if n == "mask" else torch.int32 if n == "params" else torch.float32
        wholes[n], out[n] = _guarded(gpu, shape, dtype, lead)
    before = {n: t.clone() for n, t in dev.items()}
    r = nconv_amd.augment(**dev, size=size, out=out, **kw)
    torch.cuda.synchronize()
    assert set(r) == set(out) and all(r[n] is out[n] for n in out)
    for n, t in dev.items():  # the sources are only read
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t,
                           before[n].view(torch.int32) if t.dtype == torch.float32 else before[n]), n
    for n, whole in wholes.items():
        cnt = out[n].numel()
        g = GUARD[whole.dtype]
        assert bool((whole[:lead] == g).all()) and bool((whole[lead + cnt:] == g).all()), n
    got = {n: t.cpu().numpy() for n, t in out.items()}
    for n in ("depth", "gt", "extra", "mask"):
        if n in got:
            got[n] = got[n][:, 0]
    if check:
        _compare(got, src, size, **kw)
    return got


def _ref(src, size, **kw):
    kw = dict(kw)
    kw.pop("return_params", None)
    crop = kw.pop("crop", ("random", "random"))
    modes = tuple(AC.MODES[m] for m in ((crop, crop) if isinstance(crop, str) else crop))
    planes = {n: src[n] for n in ("depth", "gt", "extra") if n in src}
    H, W = next(a.shape[-2:] for n, a in src.items() if n != "k") if len(src) > 1 or "k" not in src else (None, None)
    return planes, modes, kw, (H, W)


def _compare(got, src, size, src_size=None, **kw):
    planes, modes, kw, hw = _ref(src, size, **kw)
    ref = AC.augment_ref(size, src.get("rgb"), planes, src.get("mask"), src.get("k"),
                         src_size=src_size or hw, modes=modes, **kw)
    assert set(ref) == set(got)
    for n in ref:
        assert AC.same_bits(got[n], ref[n]), (n, size, kw, modes, got["params"].tolist())
    return ref


def _pick_seed(B, H, W, h, w, need_offsets=True):
    """The first seed whose draw 0 (on the reference) flips some images of the batch and not others, with
    pairwise distinct (y0, x0) where the geometry leaves room for it."""
    room = (H - h + 1) * (W - w + 1) >= 2 * B
    for seed in range(1, 512):
        p = [AC.params_ref(seed, 0, b, H, W, h, w) for b in range(B)]
        if {q[2] for q in p} == {0, 1} and (not (room and need_offsets) or len({q[:2] for q in p}) == B):
            return seed, room
    raise AssertionError("no seed found")


# ---- the sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi", range(len(AC.GEOMETRIES)), ids=lambda i: "{}x{}-{}x{}".format(*AC.GEOMETRIES[i][0], *AC.GEOMETRIES[i][1]))
def test_sweep_matches_reference(nconv_amd, gpu, gi):
    (H, W), size = AC.GEOMETRIES[gi]
    B = 3
    src = _sources(B, H, W, seed=10 * gi)
    seed, room = _pick_seed(B, H, W, *size)
    # every flip setting, the crop mode pairs in rotation: 18 calls over the sweep cover all 16
    for fi, p in enumerate((0.0, 1.0, 0.5)):
        crop = MODE_PAIRS[(3 * gi + fi) % 16]
        got = _run(nconv_amd, gpu, size, src, seed=seed, flip=p, crop=crop, lead=fi % 2)
        if p != 0.5:
            assert (got["params"][:, 2] == int(p)).all()
    # random windows: flipped and unflipped images in one batch, distinct offsets where there is room
    got = _run(nconv_amd, gpu, size, src, seed=seed, flip=0.5, lead=1)
    assert set(got["params"][:, 2].tolist()) == {0, 1}
    if room:
        assert len({tuple(r[:2]) for r in got["params"].tolist()}) == B
    # each tensor alone (k alone needs the source size)
    for n in src:
        extra = dict(src_size=(H, W)) if n == "k" else {}
        _run(nconv_amd, gpu, size, {n: src[n]}, seed=seed, flip=0.5, **extra)
    _run(nconv_amd, gpu, size, {"rgb": src["rgb"]}, seed=seed, flip=0.5, **JITTER)


def test_every_mode_pair_is_covered_by_the_sweep():
    assert {MODE_PAIRS[(3 * gi + fi) % 16] for gi in range(len(AC.GEOMETRIES)) for fi in range(3)} == set(MODE_PAIRS)


# ---- views -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi", (0, 3, 5))
def test_strided_misaligned_and_shared_views(nconv_amd, gpu, gi):
    (H, W), size = AC.GEOMETRIES[gi]
    B = 3
    seed, _ = _pick_seed(B, H, W, *size)
    for shared in (False, True):
        src = _sources(B, H, W, seed=70 + gi, shared_mask=shared)
        for lead, kw in ((0, {}), (1, JITTER)):
            _run(nconv_amd, gpu, size, src, views=True, seed=seed, lead=lead, **kw)
    # the shared mask of a contiguous batch, and a mask alone at an odd address
    src = _sources(B, H, W, seed=75, shared_mask=True)
    _run(nconv_amd, gpu, size, src, seed=seed)
    _run(nconv_amd, gpu, size, {"mask": AC.mask_u8(B, H, W, 5)}, views=True, seed=seed, lead=1)


# ---- jitter ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_gains(nconv_amd, tmp_path_factory):
    """augment_params.h on the host: (seed, draw, b, amplitudes) -> the five gains' bits."""
    rows = host_harness.host_report(nconv_amd, tmp_path_factory, "augment_host", csrc=True)["draws"]
    return {tuple(r[:13]): r[16:] for r in rows}


def test_jitter_matches_reference_and_host_gains(nconv_amd, gpu, host_gains):
    B, (H, W), size = 4, (7, 13), (5, 9)
    src = {"rgb": AC.image(B, H, W, seed=90)}
    amps = [dict(brightness=0.2), dict(contrast=0.2), dict(color=0.2), JITTER, dict(brightness=1.0, contrast=1.0, color=1.0)]
    for kw in amps:
        got = _run(nconv_amd, gpu, size, src, seed=6, draw=3, **kw)
        assert (got["gains"] != 1).any() and got["rgb"].min() >= 0 and got["rgb"].max() <= 255
    # values that clamp at 0 and at 255: strong contrast pushes both ends out
    v = src["rgb"].copy()
    v[:, :, :, ::2], v[:, :, :, 1::2] = 2.0, 253.0
    for seed in range(4):
        _run(nconv_amd, gpu, size, {"rgb": v}, seed=seed, brightness=0.5, contrast=1.0, color=0.3, pivot=127.5)
    both = [AC.augment_ref(size, v, seed=s, brightness=0.5, contrast=1.0, color=0.3)["rgb"] for s in range(4)]
    assert any((r == 0).any() for r in both) and any((r == 255).any() for r in both)
    _run(nconv_amd, gpu, size, {"rgb": v}, seed=2, brightness=0.3, pivot=100.0, rgb_max=200.0)  # other constants
    # the gains the kernel reports are the host program's, for the rows of its table (7 x 13 -> 5 x 9 and KITTI)
    bits = lambda f: int(np.array([f], dtype=F32).view(U32)[0])
    seen = 0
    for (seed, draw, b, h_, w_, oh, ow, my, mx, thr, bri, con, col), want in host_gains.items():
        if (h_, w_, oh, ow) != (7, 13, 5, 9) or b != 3:
            continue
        amp = dict(brightness=float(np.array([bri], dtype=U32).view(F32)[0]), contrast=float(np.array([con], dtype=U32).view(F32)[0]),
                   color=float(np.array([col], dtype=U32).view(F32)[0]))
        got = _run(nconv_amd, gpu, size, src, seed=seed, draw=draw, crop=(MODE_NAMES[my], MODE_NAMES[mx]),
                   flip=thr / 4294967296.0, **amp)
        for bb in range(4):
            key = (seed, draw, bb, h_, w_, oh, ow, my, mx, thr, bri, con, col)
            assert [bits(g) for g in got["gains"][bb]] == host_gains[key]
        seen += 1
    assert seen == 9


# ---- KITTI size ------------------------------------------------------------------------------------
def test_kitti_size_matches_reference(nconv_amd, gpu):
    B, H, W = 2, 352, 1216
    src = _sources(B, H, W, seed=40)
    _run(nconv_amd, gpu, (256, 1216), src, seed=5, draw=2, crop=("max", "random"), **JITTER)
    got = _run(nconv_amd, gpu, (256, 1024), src, seed=5, draw=2, lead=1, **JITTER)
    assert got["params"][:, 1].max() > 0


# ---- determinism -----------------------------------------------------------------------------------
def test_deterministic_in_the_state_and_fresh_per_draw(nconv_amd, gpu):
    B, (H, W), size = 3, (9, 20), (3, 17)
    src = _sources(B, H, W, seed=50)
    dev = _to_device(gpu, src, False)
    mod = __import__("sys").modules[nconv_amd.augment.__module__]
    state = mod.make_state(0xABCDEF0123456789, 4, gpu)
    a = nconv_amd.augment(**dev, size=size, state=state, return_params=True, **JITTER)
    b = nconv_amd.augment(**dev, size=size, state=state, return_params=True, **JITTER)
    c = nconv_amd.augment(**dev, size=size, seed=0xABCDEF0123456789, draw=4, return_params=True, **JITTER)
    torch.cuda.synchronize()
    assert state.cpu().tolist() == mod.state_words(0xABCDEF0123456789, 4)  # only read
    for n in a:
        assert AC.same_bits(a[n].cpu().numpy(), b[n].cpu().numpy()) and AC.same_bits(a[n].cpu().numpy(), c[n].cpu().numpy()), n
    seen = {tuple(a["params"].cpu().numpy().reshape(-1).tolist())}
    for draw in (5, 6, 7):
        got = _run(nconv_amd, gpu, size, src, seed=0xABCDEF0123456789, draw=draw, **JITTER)
        seen.add(tuple(got["params"].reshape(-1).tolist()))
    assert len(seen) == 4


# ---- capture ---------------------------------------------------------------------------------------
def test_augmenter_under_graph_capture(nconv_amd, gpu):
    B, (H, W), size = 3, (37, 71), (20, 33)
    srcs = [_sources(B, H, W, seed=60 + 7 * r) for r in range(3)]
    for s in srcs:
        s.pop("extra")
    dev = _to_device(gpu, srcs[0], False)
    au = nconv_amd.Augmenter((H, W), size, B=B, seed=77, draw=5, **JITTER)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        au(**dev)  # warm-up: buffers and state exist before the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    au.reset(5)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = au(**dev)
    assert set(out) == set(dev) | {"params", "gains"}
    params = []
    for rep in range(3):
        fresh = _to_device(gpu, srcs[rep], False)
        for n in dev:
            dev[n].copy_(fresh[n])  # refilled in place: the graph reads the captured addresses
        g.replay()
        torch.cuda.synchronize()
        got = {n: t.cpu().numpy() for n, t in out.items()}
        for n in ("depth", "gt", "mask"):
            got[n] = got[n][:, 0]
        _compare(got, srcs[rep], size, seed=77, draw=5 + rep, **JITTER)
        params.append(tuple(got["params"].reshape(-1).tolist()))
    assert len(set(params)) == 3
    assert au.state.cpu().tolist()[2] == 8
    au.reset(5)
    g.replay()
    torch.cuda.synchronize()
    assert tuple(out["params"].cpu().numpy().reshape(-1).tolist()) == params[0]
    fixed = nconv_amd.Augmenter((H, W), size, B=B, seed=77, draw=5, advance=False, **JITTER)
    a = fixed(**dev)["params"].clone()
    assert torch.equal(a, fixed(**dev)["params"]) and tuple(a.cpu().numpy().reshape(-1).tolist()) == params[0]


# ---- behind the prefetcher -------------------------------------------------------------------------
def test_augment_behind_the_prefetcher(nconv_amd, gpu):
    B, H, W, size = 2, 37, 71, (24, 40)
    rng = np.random.default_rng(8)
    raw, batches = [], []
    for i in range(2):
        z = SC.plane(B, H, W, seed=61 + i, specials=False)
        rgb = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
        _, per = SC.masks(B, H, W, seed=62 + i)
        k = AC.intrinsics(B, H, W, seed=63 + i)
        raw.append((z, rgb, per, k))
        gt = torch.from_numpy(z)[:, None]
        batches.append({"rgb": torch.from_numpy(rgb), "depth": gt.clone(), "gt": gt.clone(), "mask": torch.from_numpy(per)[:, None],
                        "k": torch.from_numpy(k), "name": f"batch{i}"})
    stage = nconv_amd.SparsifyBatch(seed=13, chain=nconv_amd.Augment(size, seed=21, chain=nconv_amd.Ingest(), return_params=True,
                                                                    **JITTER))
    pf = nconv_amd.data.DevicePrefetcher(batches, gpu, keys=("rgb", "depth", "gt", "k", "mask", "n_keep"), ingest=stage)
    got = list(pf)
    torch.cuda.synchronize()
    assert len(got) == 2
    for i, (batch, (z, rgb, per, k)) in enumerate(zip(got, raw)):
        assert batch["name"] == f"batch{i}" and "mask" not in batch and batch["rgb"].shape == (B, 3, *size)
        sparse, _ = SC.sparsify_ref(z, mask=per, floor=None, seed=13, draw=i)
        ref = AC.augment_ref(size, FC.rgb_ref(rgb), {"depth": sparse, "gt": z}, None, k, seed=21, draw=i, **JITTER)
        for n in ("rgb", "k", "params", "gains"):
            assert AC.same_bits(batch[n].cpu().numpy(), ref[n]), (i, n)
        gt, depth = batch["gt"][:, 0].cpu().numpy(), batch["depth"][:, 0].cpu().numpy()
        assert AC.same_bits(gt, ref["gt"]) and AC.same_bits(depth, ref["depth"])
        kept = depth != 0
        assert kept.any() and not kept.all() and AC.same_bits(depth[kept], gt[kept])  # a subset of the cropped gt
    assert got[0]["params"].cpu().tolist() != got[1]["params"].cpu().tolist()  # the draw advances per batch
    # a count over the uncropped image does not survive a crop
    n_keep = {"depth": batches[0]["gt"].to(gpu), "gt": batches[0]["gt"].to(gpu),
              "n_keep": torch.tensor([100, 200], dtype=torch.int32, device=gpu)}
    with pytest.raises(ValueError, match="'mask' form"):
        nconv_amd.Augment(size)(n_keep)
    same = nconv_amd.Augment((H, W), flip=0.0)(n_keep)  # nothing is cropped away: the count still holds
    assert torch.equal(same["gt"], n_keep["gt"]) and same["n_keep"] is n_keep["n_keep"]


# ---- refusals --------------------------------------------------------------------------------------
def test_refuses_overlap_and_bad_outputs(nconv_amd, gpu):
    z = torch.ones(2, 1, 8, 16, device=gpu)
    flat = torch.ones(2 * 8 * 16 + 2 * 4 * 8, device=gpu)
    src = flat[:256].view(2, 1, 8, 16)
    with pytest.raises(RuntimeError, match="output plane\\[0\\] overlaps source plane\\[0\\]"):
        nconv_amd.augment(depth=src, size=(4, 8), out={"depth": flat[192:256].view(2, 1, 4, 8)})
    with pytest.raises(RuntimeError, match="output plane\\[1\\] overlaps source plane\\[0\\]"):
        nconv_amd.augment(depth=src, gt=z, size=(4, 8), out={"gt": flat[252:316].view(2, 1, 4, 8)})
    nconv_amd.augment(depth=src, size=(4, 8), out={"depth": flat[256:].view(2, 1, 4, 8)})  # adjacent is fine
    with pytest.raises(TypeError, match="out\\['depth'\\]"):
        nconv_amd.augment(depth=z, size=(4, 8), out={"depth": torch.ones(2, 1, 4, 9, device=gpu)})
    with pytest.raises(TypeError, match="out\\['rgb'\\]"):
        nconv_amd.augment(rgb=torch.ones(2, 3, 8, 16, device=gpu), size=(4, 8), out={"rgb": torch.ones(2, 1, 4, 8, device=gpu)})
    with pytest.raises(TypeError, match="out\\['mask'\\]"):
        nconv_amd.augment(mask=torch.ones(2, 1, 8, 16, dtype=torch.uint8, device=gpu), size=(4, 8),
                          out={"mask": torch.ones(2, 1, 4, 8, device=gpu)})
    with pytest.raises(TypeError, match="out\\['params'\\]"):
        nconv_amd.augment(depth=z, size=(4, 8), out={"params": torch.ones(2, 4, device=gpu)})
    with pytest.raises(TypeError, match="out\\['k'\\]"):
        nconv_amd.augment(depth=z, k=torch.ones(2, 3, 3, device=gpu), size=(4, 8), out={"k": torch.ones(2, 9, device=gpu)})
    r = nconv_amd.augment(depth=z[0, 0], size=(8, 16), flip=0.0)  # an (H, W) plane, nothing cropped
    torch.cuda.synchronize()
    assert set(r) == {"depth"} and r["depth"].shape == (1, 1, 8, 16) and torch.equal(r["depth"][0, 0], z[0, 0])
