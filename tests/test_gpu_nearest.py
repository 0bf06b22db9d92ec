"""GPU: nconv_depth_nearest against the brute-force numpy reference (tests/nearest_cases.py), every output
exactly: dst and dist as uint32 bits, index and dist2 as integers, each buffer (the workspace too) inside
guard bands, the source verified unchanged after every call. The sweep SHAPES x DENSITIES x FLOORS x
MAX_DISTANCES with an empty and a single-sample image in every batch; forced ties and the trap of the
search's stop condition; the special values; cropped and 4-byte-shifted views, a non-contiguous image
stride, every output alone, overlap refused; rows wider than the LDS path; NearestFiller under
torch.cuda.graph; NearestFill under compat get_metrics; NearestSample behind DevicePrefetcher;
nearest_sample(project_points(...)); the worst case (one sample in a 352 x 1216 image) in closed form."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import lidar_cases as LC
import nearest_cases as NC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_F, GUARD_I = -7.0, -77
F32 = np.float32
KEYS = ("dst", "index", "dist2", "dist")
_EXTRA = (("index", torch.int32, GUARD_I), ("dist2", torch.int32, GUARD_I), ("dist", torch.float32, GUARD_F))


def _source(gpu, z, cropped=False, shifted=False):
    """z (B, H, W) as a (B, 1, H, W) device view: contiguous, or a window of a larger plane of other values
    (a non-contiguous image stride); shifted: the base one element past a 16-byte boundary."""
    B, H, W = z.shape
    lead = 1 if shifted else 0
    hh, ww = (H + 3, W + 5) if cropped else (H, W)
    whole = torch.full((B * hh * ww + lead + 3,), 123.0, device=gpu)  # 123 m all around: a sample, if it were read
    big = whole[lead:lead + B * hh * ww].view(B, 1, hh, ww)
    v = big[:, :, 1:1 + H, 2:2 + W] if cropped else big
    v.copy_(torch.from_numpy(z)[:, None])
    return v


def _guarded(gpu, shape, dtype, guard, lead):
    n = int(np.prod(shape))
    whole = torch.full((n + lead + 5,), guard, dtype=dtype, device=gpu)
    return whole, whole[lead:lead + n].view(shape)


def _guards_intact(whole, guard, lead, n):
    return bool((whole[:lead] == guard).all()) and bool((whole[lead + n:] == guard).all())


def _run(nconv_amd, gpu, z, floor=0.0, max_distance=None, cropped=False, shifted=False):
    """One call with all four outputs and the workspace guarded; returns them as numpy after checking the
    guards and that the source is unchanged."""
    B, H, W = z.shape
    n = B * H * W
    src = _source(gpu, z, cropped, shifted)
    lead = 1 if shifted else 0
    if cropped:
        dwhole = torch.full((B, 1, H + 2, W + 3), GUARD_F, device=gpu)
        dst = dwhole[:, :, 2:, 1:1 + W]
    else:
        dwhole, dst = _guarded(gpu, (B, 1, H, W), torch.float32, GUARD_F, lead)
    out, wholes = {"depth": dst}, {}
    for key, dtype, guard in _EXTRA + (("work", torch.int32, GUARD_I),):
        wholes[key], out[key] = _guarded(gpu, (B, H, W), dtype, guard, lead)
    before = src.clone()
    r = nconv_amd.nearest_sample(src, floor=floor, max_distance=max_distance, return_index=True, return_dist2=True,
                                 return_dist=True, out=out)
    torch.cuda.synchronize()
    assert torch.equal(src.view(torch.int32), before.view(torch.int32))  # the source is only read
    assert r[0] is dst and r[1] is out["index"] and r[2] is out["dist2"] and r[3] is out["dist"]
    inside = torch.zeros_like(dwhole, dtype=torch.bool)
    (inside[:, :, 2:, 1:1 + W] if cropped else inside[lead:lead + n]).fill_(True)
    assert bool((dwhole.reshape(-1)[~inside.reshape(-1)] == GUARD_F).all())
    for key, _, guard in _EXTRA + (("work", torch.int32, GUARD_I),):
        assert _guards_intact(wholes[key], guard, lead, n), key
    return dict(dst=dst[:, 0].cpu().numpy(), index=out["index"].cpu().numpy(), dist2=out["dist2"].cpu().numpy(),
                dist=out["dist"].cpu().numpy())


def _compare(got, ref, what=""):
    for k in KEYS:
        if got.get(k) is None:
            continue
        bad = int((np.ascontiguousarray(got[k]).view(np.uint32) != np.ascontiguousarray(ref[k]).view(np.uint32)).sum())
        assert bad == 0, (what, k, bad)


def _check(nconv_amd, gpu, z, floor=0.0, max_distance=None, what="", **view):
    ref = NC.nearest_ref(z, floor, max_distance)
    got = _run(nconv_amd, gpu, z, floor, max_distance, **view)
    _compare(got, ref, (what, floor, max_distance, view))
    return got, ref


# ---- the sweep --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sweep_matches_reference(nconv_amd, gpu, shape):
    H, W = shape
    B = 3  # image 1 is empty, image 2 holds one sample at (H - 1, 0)
    limited = False
    for density in NC.DENSITIES:
        for floor in NC.FLOORS:
            z = NC.plane(B, H, W, seed=100 + H + W, density=density, background=np.nan if floor is None else 0.0)
            index, dist2 = NC.solve(z, floor)  # once per plane and floor: the limit is applied to it
            assert (index[1] == -1).all() and (index[2] == (H - 1) * W).all()
            for md in NC.MAX_DISTANCES:
                ref = NC.finish(z, index, dist2, NC.max_dist2_of(md))
                got = _run(nconv_amd, gpu, z, floor, md)
                _compare(got, ref, (shape, density, floor, md))
                limited |= bool(((ref["index"] == -1) & (index >= 0)).any())
    assert limited or H * W == 1


@pytest.mark.parametrize("W", (NC.LDS_W, NC.LDS_W + 1, NC.LDS_W + 70))
def test_rows_around_the_lds_limit(nconv_amd, gpu, W):
    """Rows of up to LDS_W columns are searched in LDS, wider ones through the cache: both sides of it."""
    z = NC.plane(3, 3, W, seed=W, density=0.01)
    z[0, 1, 40:W - 500] = 0  # a long empty stretch: searches of hundreds of columns
    for floor, md in ((0.0, None), (2.5, 5), (0.0, 300)):
        _check(nconv_amd, gpu, z, floor, md, what=("wide", W))


# ---- forced ties and traps --------------------------------------------------------------------------
def test_forced_ties_and_the_stop_condition(nconv_amd, gpu):
    cases = NC.forced_planes()
    z = np.concatenate([c[1] for c in cases])
    for md in (None, 5):  # max_dist2 = 25 is the d2 of the ties: "exceeds" holds for the limit as well
        got, _ = _check(nconv_amd, gpu, z, 0.0, md, what="forced")
        for n, (name, _, centre, want) in enumerate(cases):
            if md is None or got["dist2"][n, centre[0], centre[1]] <= 25:
                assert got["index"][n, centre[0], centre[1]] == want, (name, centre, md)
    # one sample of each pair removed by the floor: the other one wins
    got, _ = _check(nconv_amd, gpu, z, 7.5, None, what="forced, floor 7.5")
    assert (got["dst"][got["index"] >= 0] > 7.5).all()


def test_checkerboard_and_all_valid(nconv_amd, gpu):
    B, H, W = 2, 37, 71
    for md in (None, 0):
        got, _ = _check(nconv_amd, gpu, NC.checkerboard(B, H, W), 0.0, md, what="checkerboard")
    z = np.random.default_rng(3).uniform(0.5, 80.0, (B, H, W)).astype(F32)
    for md in (None, 0, 5):
        got, _ = _check(nconv_amd, gpu, z, 0.0, md, what="all valid")
        assert (got["index"].reshape(B, -1) == np.arange(H * W)).all() and (got["dist2"] == 0).all()
        assert NC.same_bits(got["dst"], z) and (got["dist"].view(np.uint32) == 0).all()


def test_invalid_values_are_never_nearest(nconv_amd, gpu):
    B, H, W = 2, 33, 70
    rng = np.random.default_rng(8)
    z = np.where(rng.random((B, H, W)) < 0.1, rng.uniform(3.0, 80.0, (B, H, W)), 0.0).astype(F32)
    sp = NC.specials()
    at = rng.choice(B * H * W, size=40 * sp.size, replace=False)
    z.reshape(-1)[at] = np.resize(sp, at.size)
    for floor in (0.0, 2.5):
        got, _ = _check(nconv_amd, gpu, z, floor, what="specials")
        valid = NC.sample_of(z, floor)
        picked = np.take_along_axis(valid.reshape(B, -1), got["index"].reshape(B, -1).astype(np.int64), axis=1)
        assert picked.all() and np.isfinite(got["dst"]).all() and (got["dst"] > floor).all()
        assert (got["dst"].view(np.uint32)[valid] == z.view(np.uint32)[valid]).all()  # the samples are kept
    # floor=None: negatives, zeros and denormals are samples; NaN and +-inf never
    zn = np.where(z == 0, F32(np.nan), z).astype(F32)
    zn.reshape(-1)[at] = np.resize(sp, at.size)
    got, _ = _check(nconv_amd, gpu, zn, None, what="specials, floor None")
    assert np.isfinite(got["dst"]).all() and (got["dst"] < 0).any()
    assert (got["dst"].view(np.uint32) == F32(-0.0).view(np.uint32)).any()  # -0.0 comes out bit for bit


# ---- views, optional outputs, refusals --------------------------------------------------------------
@pytest.mark.parametrize("shape", ((3, 37, 71), (2, 71, 139)), ids=lambda s: "x".join(map(str, s)))
def test_views(nconv_amd, gpu, shape):
    B, H, W = shape
    z = NC.plane(B, H, W, seed=7, density=0.05)
    for floor, md in ((0.0, None), (2.5, 5), (None, 1.5)):
        for view in (dict(cropped=True), dict(shifted=True), dict(cropped=True, shifted=True)):
            _check(nconv_amd, gpu, z, floor, md, what="views", **view)
    # an (H, W) plane and a (1, H, W) one, and the plain return value
    for s in (torch.from_numpy(z[0]).to(gpu), torch.from_numpy(z[:1]).to(gpu)):
        r = nconv_amd.nearest_sample(s)
        assert r.shape == (1, 1, H, W) and NC.same_bits(r[0, 0].cpu().numpy(), NC.nearest_ref(z[:1])["dst"][0])


def test_every_output_alone(nconv_amd, gpu):
    """The C entry point with one output at a time (the Python call always asks for dst), and the
    Python call with each extra alone."""
    B, H, W = 2, 37, 71
    z = NC.plane(B, H, W, seed=9, density=0.05)
    ref = NC.nearest_ref(z, 0.0, 5)
    src = _source(gpu, z, cropped=True)
    L = nconv_amd._lib
    d = L.NconvDepthNearest()
    d.B, d.H, d.W, d.floor, d.max_dist2 = B, H, W, 0.0, 25
    d.src, d.src_image_stride, d.src_row_stride = src.data_ptr(), src.stride(0), src.stride(2)
    for key, dtype, guard in (("dst", torch.float32, GUARD_F),) + _EXTRA:
        whole, buf = _guarded(gpu, (B, H, W), dtype, guard, 1)
        wwhole, work = _guarded(gpu, (B, H, W), torch.int32, GUARD_I, 1)
        p = {k: (L.ptr(buf) if k == key else None) for k in KEYS}
        rc = L.lib().nconv_depth_nearest(ctypes.byref(d), p["dst"], H * W, W, p["index"], p["dist2"], p["dist"],
                                         L.ptr(work), L.stream_handle(gpu))
        L.check(rc, "nconv_depth_nearest")
        torch.cuda.synchronize()
        assert _guards_intact(whole, guard, 1, B * H * W) and _guards_intact(wwhole, GUARD_I, 1, B * H * W)
        _compare({key: buf.cpu().numpy()}, ref, ("alone", key))
    for n, (flag, key) in enumerate((("return_index", "index"), ("return_dist2", "dist2"), ("return_dist", "dist"))):
        r = nconv_amd.nearest_sample(src, max_distance=5, **{flag: True})
        assert isinstance(r, tuple) and len(r) == 2 and r[0].shape == (B, 1, H, W) and r[1].shape == (B, H, W)
        _compare({"dst": r[0][:, 0].cpu().numpy(), key: r[1].cpu().numpy()}, ref, ("python, alone", key))
    r = nconv_amd.nearest_sample(src, max_distance=5, return_dist=True, return_index=True)
    _compare({"index": r[1].cpu().numpy(), "dist": r[2].cpu().numpy()}, ref, "index then dist")


def test_refuses_overlap_and_bad_outputs(nconv_amd, gpu):
    z = torch.rand(2, 1, 8, 16, device=gpu) + 1.0
    before = z.clone()
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        nconv_amd.nearest_sample(z, out={"depth": z})
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        nconv_amd.nearest_sample(z[:, :, :6], out={"depth": z[:, :, 2:]})
    plane = torch.zeros(2, 8, 16, dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="index overlaps work"):
        nconv_amd.nearest_sample(z, return_index=True, out={"index": plane, "work": plane})
    with pytest.raises(RuntimeError, match="dist overlaps dst"):
        d = torch.zeros(2, 1, 8, 16, device=gpu)
        nconv_amd.nearest_sample(z, return_dist=True, out={"depth": d, "dist": d[:, 0]})
    with pytest.raises(TypeError, match="out\\['depth'\\]"):
        nconv_amd.nearest_sample(z, out={"depth": torch.ones(2, 1, 8, 15, device=gpu)})
    with pytest.raises(TypeError, match="out\\['work'\\]"):
        nconv_amd.nearest_sample(z, out={"work": torch.ones(2, 8, 16, device=gpu)})
    with pytest.raises(RuntimeError, match="out\\['dist2'\\] on cpu"):
        nconv_amd.nearest_sample(z, return_dist2=True, out={"dist2": torch.ones(2, 8, 16, dtype=torch.int32)})
    torch.cuda.synchronize()
    assert torch.equal(z, before)


# ---- capture, module, stage, composition ------------------------------------------------------------
def test_filler_under_graph_capture(nconv_amd, gpu):
    B, H, W = 2, 37, 71
    za, zb = NC.plane(B, H, W, seed=51, density=0.3), NC.plane(B, H, W, seed=52, density=0.02)
    src = torch.from_numpy(za)[:, None].to(gpu)
    fill = nconv_amd.NearestFiller((H, W), B=B, max_distance=5, return_index=True, return_dist2=True, return_dist=True)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        fill(src)  # warm-up: the buffers and the workspace exist before the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = fill(src)
    assert len(outs) == 4 and outs[0].shape == (B, 1, H, W)
    for z in (za, zb, za):
        src.copy_(torch.from_numpy(z)[:, None])
        for t in outs:
            t.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        got = dict(dst=outs[0][:, 0].cpu().numpy(), index=outs[1].cpu().numpy(), dist2=outs[2].cpu().numpy(),
                   dist=outs[3].cpu().numpy())
        _compare(got, NC.nearest_ref(z, 0.0, 5), "replay")


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


def test_module_and_compat_get_metrics(nconv_amd, gpu):
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
    s = loader[0]["depth"].to(gpu)
    for o in (dict(), dict(max_distance=3.0), dict(floor=40.0)):
        model = nconv_amd.NearestFill(**o)
        assert torch.equal(model(s).view(torch.int32), nconv_amd.nearest_sample(s, **o).view(torch.int32))
        assert NC.same_bits(model(s)[:, 0].cpu().numpy(), NC.nearest_ref(refs[0], o.get("floor", 0.0), o.get("max_distance"))["dst"])
        kw = dict(gt_max=70.0)
        got = utils.get_metrics(model, loader, "cuda", **kw)
        hand = nconv_amd.DepthMetrics(device=gpu, **kw)
        for data, depth in zip(loader, refs):
            pred = torch.from_numpy(NC.nearest_ref(depth, o.get("floor", 0.0), o.get("max_distance"))["dst"])[:, None].to(gpu)
            hand.update(pred, data["gt"].to(gpu))
        want = hand.compute(1.0)
        assert got == want and got["n"] > 0 and 0 < got["rmse"] < 80, (o, got)


def test_nearest_stage_behind_the_prefetcher(nconv_amd, gpu):
    rng = np.random.default_rng(6)
    B, h, w = 2, 37, 71
    metres = NC.plane(2 * B, h, w, seed=61, density=0.1, with_specials=False)
    raw = np.rint(metres * 256.0).astype(np.uint16)
    batches = [{"depth": torch.from_numpy(raw[:B]), "gt": torch.from_numpy(raw[B:]), "name": "a",
                "k": torch.from_numpy(rng.random((B, 3, 3)).astype(F32))},
               {"depth": torch.from_numpy(raw[B:]), "gt": torch.from_numpy(raw[:B]), "name": "b",
                "k": torch.from_numpy(rng.random((B, 3, 3)).astype(F32))}]
    ingest = nconv_amd.Ingest(depth_decode="kitti16")
    stage = nconv_amd.NearestSample(chain=ingest, dist_key="dist", max_distance=6)
    got = list(nconv_amd.data.DevicePrefetcher(batches, gpu, ingest=stage))
    torch.cuda.synchronize()
    assert len(got) == 2
    for raw_batch, b in zip(batches, got):
        plain = ingest({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in raw_batch.items()})
        assert sorted(b) == sorted(list(raw_batch) + ["filled", "dist"]) and b["name"] == raw_batch["name"]
        assert torch.equal(b["depth"], plain["depth"]) and torch.equal(b["gt"], plain["gt"])
        assert torch.equal(b["k"].cpu(), raw_batch["k"])
        ref = NC.nearest_ref(plain["depth"][:, 0].cpu().numpy(), 0.0, 6)
        assert b["filled"].shape == (B, 1, h, w) and b["dist"].shape == (B, 1, h, w) and b["dist"].dtype == torch.float32
        _compare(dict(dst=b["filled"][:, 0].cpu().numpy(), dist=b["dist"][:, 0].cpu().numpy()), ref, "stage")
    # without a chain and without dist_key the stage fills an fp32 batch as it is
    f = nconv_amd.NearestSample()({"depth": torch.from_numpy(metres[:B])[:, None].to(gpu), "x": 1})
    assert sorted(f) == ["depth", "filled", "x"] and f["x"] == 1
    assert NC.same_bits(f["filled"][:, 0].cpu().numpy(), NC.nearest_ref(metres[:B])["dst"])


def test_composes_with_project_points(nconv_amd, gpu):
    B, H, W, rows = 3, 37, 71, 600
    pts, off, m, _ = LC.scan(np.random.default_rng(9), B, H, W, rows)
    p = LC.project_ref(pts, off, m, (H, W))
    args = (torch.from_numpy(pts).to(gpu), torch.from_numpy(off).to(gpu), torch.from_numpy(m).to(gpu), (H, W))
    filled, index, dist2 = nconv_amd.nearest_sample(nconv_amd.project_points(*args), return_index=True, return_dist2=True)
    torch.cuda.synchronize()
    ref = NC.nearest_ref(p["depth"][:, 0])
    assert 0 < (ref["dist2"] == 0).mean() < 0.5 and (ref["index"] >= 0).all()
    _compare(dict(dst=filled[:, 0].cpu().numpy(), index=index.cpu().numpy(), dist2=dist2.cpu().numpy()), ref, "scan")
    # the recipe of the distance strata: the mask of the pixels within 4 px of a return
    near = (dist2 <= 16)[:, None]
    assert near.shape == filled.shape and bool(near.any()) and not bool(near.all())


def test_worst_case_finishes(nconv_amd, gpu):
    """One sample in a corner of a 352 x 1216 image: every pixel searches its whole row. The reference in
    closed form; with a range limit as well."""
    shape = (1, 352, 1216)
    for at, md in (((351, 0), None), ((0, 1215), None), ((351, 0), 700.5)):
        z, ref = NC.single_ref(shape, at, 41.5, NC.max_dist2_of(md))
        got = _run(nconv_amd, gpu, z, 0.0, md)
        _compare(got, ref, ("worst", at, md))
        assert md is None or ((got["index"] == -1).any() and (got["index"] >= 0).any())
