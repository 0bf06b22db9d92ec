"""GPU: nconv_depth_ipbasic against the numpy reference (tests/ipbasic_cases.py) bit for bit: every
comparison on uint32 bits, outputs and workspaces inside guard bands, the source verified unchanged. The
sweep SHAPES x DENSITIES x a covering set of the options; cropped and 4-byte-shifted views and a
non-contiguous image stride; forced cases in the image corners, on both sides of a tile seam and at a
four-tile corner, columns with one or no valid pixel under extrapolate, the special values; overlap
refused; IPBasicFiller under torch.cuda.graph; IPBasicFill behind DevicePrefetcher; compat get_metrics on
IPBasic; launch counts."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import ipbasic_cases as IC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_F, GUARD_I = -7.0, -77
F32 = np.float32
TH, TW = IC.TILE


def _source(gpu, z, cropped, shifted):
    """z (B, H, W) as a (B, 1, H, W) device view: contiguous, or a window of a larger plane of other values
    (a non-contiguous image stride); shifted: the base one element past a 16-byte boundary."""
    B, H, W = z.shape
    lead = 1 if shifted else 0
    hh, ww = (H + 3, W + 5) if cropped else (H, W)
    whole = torch.full((B * hh * ww + lead + 3,), 50.0, device=gpu)
    big = whole[lead:lead + B * hh * ww].view(B, 1, hh, ww)
    v = big[:, :, 1:1 + H, 2:2 + W] if cropped else big
    v.copy_(torch.from_numpy(z)[:, None])
    return v


def _guarded(gpu, shape, dtype, guard, lead):
    n = int(np.prod(shape))
    whole = torch.full((n + lead + 5,), guard, dtype=dtype, device=gpu)
    return whole, whole[lead:lead + n].view(shape)


def _run(nconv_amd, gpu, z, options, cropped=False, shifted=False):
    """One call with guarded outputs and workspaces; the result (B, H, W) as numpy, after checking the
    guards and that the source is unchanged."""
    B, H, W = z.shape
    src = _source(gpu, z, cropped, shifted)
    lead = 1 if shifted else 0
    if cropped:
        dwhole = torch.full((B, 1, H + 2, W + 3), GUARD_F, device=gpu)
        dst = dwhole[:, :, 2:, 1:1 + W]
    else:
        dwhole, dst = _guarded(gpu, (B, 1, H, W), torch.float32, GUARD_F, lead)
    out = {"depth": dst}
    if options["extrapolate"]:
        wwhole, out["work"] = _guarded(gpu, (B, H, W), torch.float32, GUARD_F, lead)
        twhole, out["top"] = _guarded(gpu, (B, W), torch.int32, GUARD_I, lead)
    before = src.clone()
    r = nconv_amd.ipbasic_fill(src, out=out, **options)
    torch.cuda.synchronize()
    assert r is dst
    assert torch.equal(src.view(torch.int32), before.view(torch.int32))  # the source is only read
    inside = torch.zeros_like(dwhole, dtype=torch.bool)
    (inside[:, :, 2:, 1:1 + W] if cropped else inside[lead:lead + B * H * W]).fill_(True)
    assert bool((dwhole.reshape(-1)[~inside.reshape(-1)] == GUARD_F).all())
    if options["extrapolate"]:
        assert bool((wwhole[:lead] == GUARD_F).all()) and bool((wwhole[lead + B * H * W:] == GUARD_F).all())
        assert bool((twhole[:lead] == GUARD_I).all()) and bool((twhole[lead + B * W:] == GUARD_I).all())
    return dst[:, 0].cpu().numpy()


def _check(nconv_amd, gpu, z, options=None, what="", **view):
    o = dict(IC.DEFAULTS, **(options or {}))
    ref = IC.ipbasic_ref(z, **o)
    got = _run(nconv_amd, gpu, z, o, **view)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (what, o, view, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    return got


@pytest.mark.parametrize("shape", IC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sweep_matches_reference(nconv_amd, gpu, shape):
    B, H, W = shape
    filled = False
    for density in IC.DENSITIES:
        for o in IC.OPTION_SETS:
            z = IC.plane(B, H, W, seed=100 + H + W, density=density, max_depth=o["max_depth"])
            got = _check(nconv_amd, gpu, z, o, what=(shape, density))
            filled |= bool((got != 0).sum() > IC.sample_of(z, o["max_depth"]).sum())
    assert filled or H * W == 1


def test_every_kernel_beside_both_extrapolate_settings(nconv_amd, gpu):
    z = IC.plane(2, 71, 139, seed=9, density=0.05)
    for kernel in IC.KERNELS + (("cross", 3), ("full", 7), ("cross", 5), ("full", 5), ("diamond", 3)):
        for extrapolate in (False, True):
            _check(nconv_amd, gpu, z, dict(kernel=kernel, extrapolate=extrapolate), what="kernels")


@pytest.mark.parametrize("shape", ((3, 37, 71), (2, 71, 139)), ids=lambda s: "x".join(map(str, s)))
def test_views(nconv_amd, gpu, shape):
    B, H, W = shape
    z = IC.plane(B, H, W, seed=7, density=0.3)
    for o in (dict(), dict(extrapolate=True, keep_samples=True), dict(kernel=("cross", 7), blur=None)):
        for view in (dict(cropped=True), dict(shifted=True), dict(cropped=True, shifted=True)):
            _check(nconv_amd, gpu, z, o, what="views", **view)
    # an (H, W) plane and a (1, H, W) plane, and the plain return value
    for s in (torch.from_numpy(z[0]).to(gpu), torch.from_numpy(z[:1]).to(gpu)):
        r = nconv_amd.ipbasic_fill(s)
        assert r.shape == (1, 1, H, W) and IC.same_bits(r[0, 0].cpu().numpy(), IC.ipbasic_ref(z[:1])[0])


FORCED = (1, TH + 9, TW + 7)  # two tiles each way, the second ragged: the seams are at row TH and column TW


def _lone(points, depth=30.0, shape=FORCED):
    planes = []
    for y, x in points:
        z = np.zeros(shape, dtype=F32)
        z[0, y, x] = depth
        planes.append(z)
    return np.concatenate(planes, axis=0)


def test_forced_lone_samples_in_corners_and_at_seams(nconv_amd, gpu):
    """One sample per image: in each image corner, on both sides of the row seam and of the column seam,
    and on the four pixels around the four-tile corner. Every stage's window crosses the border or the
    seam there."""
    _, H, W = FORCED
    points = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (TH - 1, 20), (TH, 20), (20, TW - 1), (20, TW),
              (TH - 1, TW - 1), (TH - 1, TW), (TH, TW - 1), (TH, TW))
    z = _lone(points)
    for o in (dict(), dict(extrapolate=True), dict(kernel=("full", 7), median=False, blur=None),
              dict(kernel=("cross", 7), keep_samples=True), dict(kernel=("diamond", 7), extrapolate=True, blur=None)):
        got = _check(nconv_amd, gpu, z, o, what="lone")
        for n, (y, x) in enumerate(points):
            assert got[n, y, x] > 0 and (got[n] != 0).sum() >= 25
    # the default chain without median and blur gives the depth back exactly on the filled shape
    got = _check(nconv_amd, gpu, z, dict(median=False, blur=None), what="lone, exact")
    assert set(np.unique(got).tolist()) == {0.0, 30.0}


def test_forced_exact_constant(nconv_amd, gpu):
    z = np.zeros((2, TH + 24, TW + 40), dtype=F32)
    z[:, ::4, ::4] = 36.0
    for extrapolate in (False, True):
        got = _check(nconv_amd, gpu, z, dict(extrapolate=extrapolate), what="constant")
        assert IC.same_bits(got, np.full_like(z, 36.0))


def test_forced_extrapolation_columns(nconv_amd, gpu):
    """A column whose only valid pixel is in the last row, and columns with none: the neighbours are far
    enough away that nothing reaches them before the extrapolation (40 empty columns on either side)."""
    H, W = 2 * TH + 5, 100
    z = np.zeros((2, H, W), dtype=F32)
    z[0, H - 1, 50] = 12.5      # the last row only; every other column of image 0 has none
    z[1, 70, 50] = 40.0         # top below a tile seam; columns 0 .. 39 and 61 .. stay empty
    z[1, H - 1, 10] = 7.0
    ref = IC.ipbasic_ref(z, extrapolate=True, stages=True)
    assert ref["top"][0, 50] <= H - 1 - 3 and ref["top"][0, 0] == 0 and (ref["v3e"][0, :, 0] == 0).all()
    assert (ref["v3e"][0, :, 50] > 0).all() and (ref["v4"] == 0).any()
    for o in (dict(extrapolate=True), dict(extrapolate=True, median=False, blur=None),
              dict(extrapolate=True, kernel=("full", 3), keep_samples=True)):
        got = _check(nconv_amd, gpu, z, o, what="columns")
        assert (got[0, :, 50] > 0).all() and (got[0, :, 0] == 0).all()


def test_forced_specials(nconv_amd, gpu):
    """Every special value beside real samples in the interior, at a seam and in a corner, is no sample;
    a plane of one special value alone comes out as zeros."""
    _, H, W = FORCED
    sp = IC.specials()
    z = np.zeros((len(sp), H, W), dtype=F32)
    for n, v in enumerate(sp):
        for y, x in ((10, 20), (TH - 1, TW - 1), (TH, TW), (0, 0), (H - 1, W - 1)):
            z[n, y, x] = v
        z[n, 12, 22], z[n, TH + 1, TW - 2] = 25.0, 60.0
    for o in (dict(), dict(extrapolate=True, keep_samples=True), dict(median=False, blur=None)):
        got = _check(nconv_amd, gpu, z, o, what="specials")
        assert np.isfinite(got).all() and not np.signbit(got).any()
    for v in sp:
        got = _check(nconv_amd, gpu, np.full((1, 9, 70), v, dtype=F32), dict(extrapolate=True), what="all special")
        assert (got.view(np.uint32) == 0).all()


def test_refuses_overlap_and_bad_outputs(nconv_amd, gpu):
    z = torch.rand(2, 1, 8, 16, device=gpu) + 1.0
    before = z.clone()
    with pytest.raises(RuntimeError, match="overlaps src"):
        nconv_amd.ipbasic_fill(z, out={"depth": z})
    with pytest.raises(RuntimeError, match="overlaps src"):
        nconv_amd.ipbasic_fill(z[:, :, :6], out={"depth": z[:, :, 2:]})
    with pytest.raises(RuntimeError, match="workspace overlaps"):
        nconv_amd.ipbasic_fill(z[:1], extrapolate=True, out={"work": z[0]})
    with pytest.raises(TypeError, match="out\\['depth'\\]"):
        nconv_amd.ipbasic_fill(z, out={"depth": torch.ones(2, 1, 8, 15, device=gpu)})
    with pytest.raises(TypeError, match="out\\['work'\\]"):
        nconv_amd.ipbasic_fill(z, extrapolate=True, out={"work": torch.ones(2, 8, 15, device=gpu)})
    with pytest.raises(TypeError, match="out\\['top'\\]"):
        nconv_amd.ipbasic_fill(z, extrapolate=True, out={"top": torch.ones(2, 16, device=gpu)})
    torch.cuda.synchronize()
    assert torch.equal(z, before)


@pytest.mark.parametrize("extrapolate", (False, True), ids=("plain", "extrapolate"))
def test_filler_under_graph_capture(nconv_amd, gpu, extrapolate):
    B, H, W = 2, 71, 139
    za, zb = IC.plane(B, H, W, seed=51, density=0.3), IC.plane(B, H, W, seed=52, density=0.05)
    o = dict(extrapolate=extrapolate, kernel=("diamond", 7), keep_samples=extrapolate)
    src = torch.from_numpy(za)[:, None].to(gpu)
    flt = nconv_amd.IPBasicFiller((H, W), B=B, **o)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        flt(src)  # warm-up: the buffers exist before the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = flt(src)
    for z in (za, zb, za):
        src.copy_(torch.from_numpy(z)[:, None])
        out.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert IC.same_bits(out[:, 0].cpu().numpy(), IC.ipbasic_ref(z, **dict(IC.DEFAULTS, **o)))


def test_fill_stage_behind_the_prefetcher(nconv_amd, gpu):
    rng = np.random.default_rng(6)
    B, h, w = 2, 37, 71
    metres = IC.plane(2 * B, h, w, seed=61, density=0.3, with_specials=False)
    raw = np.rint(metres * 256.0).astype(np.uint16)
    batches = [{"depth": torch.from_numpy(raw[:B]), "gt": torch.from_numpy(raw[B:]), "name": "a",
                "k": torch.from_numpy(rng.random((B, 3, 3)).astype(F32))},
               {"depth": torch.from_numpy(raw[B:]), "gt": torch.from_numpy(raw[:B]), "name": "b",
                "k": torch.from_numpy(rng.random((B, 3, 3)).astype(F32))}]
    ingest = nconv_amd.Ingest(depth_decode="kitti16")
    stage = nconv_amd.IPBasicFill(chain=ingest, out_key="filled", extrapolate=True)
    got = list(nconv_amd.data.DevicePrefetcher(batches, gpu, ingest=stage))
    torch.cuda.synchronize()
    assert len(got) == 2
    for raw_batch, b in zip(batches, got):
        plain = ingest({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in raw_batch.items()})
        assert sorted(b) == sorted(list(raw_batch) + ["filled"]) and b["name"] == raw_batch["name"]
        assert torch.equal(b["depth"], plain["depth"]) and torch.equal(b["gt"], plain["gt"])
        assert torch.equal(b["k"].cpu(), raw_batch["k"])
        z = plain["depth"][:, 0].cpu().numpy()
        assert b["filled"].shape == (B, 1, h, w)
        assert IC.same_bits(b["filled"][:, 0].cpu().numpy(), IC.ipbasic_ref(z, extrapolate=True))
    # out_key=None replaces the key; without a chain the stage fills an fp32 batch as it is
    f = nconv_amd.IPBasicFill()({"depth": torch.from_numpy(metres[:B])[:, None].to(gpu), "x": 1})
    assert f["x"] == 1 and IC.same_bits(f["depth"][:, 0].cpu().numpy(), IC.ipbasic_ref(metres[:B]))


def _compat_utils():
    compat = os.path.join(ROOT, "compat")
    sys.path.insert(0, compat)
    try:
        spec = importlib.util.spec_from_file_location("nconv_compat_utils", os.path.join(compat, "utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(compat)
    return mod


def test_compat_get_metrics_scores_the_baseline(nconv_amd, gpu):
    utils = _compat_utils()
    B, H, W = 2, 40, 75
    loader, refs = [], []
    for seed in (21, 22):
        rng = np.random.default_rng(seed)
        gt = rng.uniform(2.0, 80.0, (B, H, W)).astype(F32)
        gt[:, :12] = 0
        depth = np.where(rng.random((B, H, W)) < 0.1, gt, F32(0)).astype(F32)
        loader.append({"depth": torch.from_numpy(depth)[:, None], "gt": torch.from_numpy(gt)[:, None]})
        refs.append(depth)
    kw = dict(gt_max=70.0)
    for o in (dict(), dict(extrapolate=True)):
        model = nconv_amd.IPBasic(**o)
        got = utils.get_metrics(model, loader, "cuda", **kw)
        hand = nconv_amd.DepthMetrics(device=gpu, **kw)
        for data, depth in zip(loader, refs):
            pred = torch.from_numpy(IC.ipbasic_ref(depth, **o))[:, None].to(gpu)
            hand.update(pred, data["gt"].to(gpu))
        want = hand.compute(1.0)
        assert got == want and got["n"] > 0 and 0 < got["rmse"] < 80, (o, got)


def _device_events(fn):
    """The device-side events (kernels, memsets, copies) of fn(), by name."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_launch_counts(nconv_amd, gpu):
    B, H, W = 2, 71, 139
    src = torch.from_numpy(IC.plane(B, H, W, seed=3, density=0.05))[:, None].to(gpu)
    out = {"depth": torch.empty(B, 1, H, W, device=gpu), "work": torch.empty(B, H, W, device=gpu),
           "top": torch.empty(B, W, dtype=torch.int32, device=gpu)}
    for extrapolate in (False, True):
        nconv_amd.ipbasic_fill(src, extrapolate=extrapolate, out=out)  # library and code objects loaded
    plain = _device_events(lambda: nconv_amd.ipbasic_fill(src, out=out))
    extra = _device_events(lambda: nconv_amd.ipbasic_fill(src, extrapolate=True, out=out))
    print(f"plain {plain}, extrapolate {extra}")
    assert len(plain) == 1 and "ipbasic_tile" in plain[0], plain
    assert 1 <= len(extra) <= 3 and all("ipbasic" in n for n in extra), extra
