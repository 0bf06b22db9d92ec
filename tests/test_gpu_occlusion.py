"""GPU: nconv_depth_occlusion against the numpy reference (tests/occlusion_cases.py) bit for bit: dst as
uint32 bits, removed, counts and index exactly, each inside guard bands. The sweep SHAPES x WINDOWS x
min_support x floor at two densities; cropped and 4-byte-shifted views, a non-contiguous image stride,
calls without the optional outputs; forced cases in the interior, across a tile seam and in the image
corners; overlap refused; OcclusionFilter under torch.cuda.graph; RemoveOccluded behind DevicePrefetcher;
remove_occluded(*project_points(...)) on a scan."""
import numpy as np
import pytest
import torch

import lidar_cases as LC
import occlusion_cases as OC

pytestmark = pytest.mark.gpu

GUARD_F, GUARD_I, GUARD_B = -7.0, -77, 0x5A
F32 = np.float32
TH, TW = OC.TILE


def _source(gpu, z, cropped, shifted):
    """z (B, H, W) as a (B, 1, H, W) device view: contiguous, or a window of a larger plane of other values
    (a non-contiguous image stride); shifted: the base one element past a 16-byte boundary."""
    B, H, W = z.shape
    lead = 1 if shifted else 0
    hh, ww = (H + 3, W + 5) if cropped else (H, W)
    whole = torch.full((B * hh * ww + lead + 3,), 123.0, device=gpu)
    big = whole[lead:lead + B * hh * ww].view(B, 1, hh, ww)
    v = big[:, :, 1:1 + H, 2:2 + W] if cropped else big
    v.copy_(torch.from_numpy(z)[:, None])
    return v


def _guarded(gpu, shape, dtype, guard, lead):
    n = int(np.prod(shape))
    whole = torch.full((n + lead + 5,), guard, dtype=dtype, device=gpu)
    return whole, whole[lead:lead + n].view(shape)


def _run(nconv_amd, gpu, z, window, *, jump=OC.JUMPS, min_support=1, floor=0.0, cropped=False, shifted=False,
         index=None, optional=True):
    """One call with guarded outputs; returns dict(dst, removed, counts, index) as numpy (None where not asked
    for) after checking the guards and that the source is unchanged."""
    B, H, W = z.shape
    src = _source(gpu, z, cropped, shifted)
    lead = 1 if shifted else 0
    if cropped:
        dwhole = torch.full((B, 1, H + 2, W + 3), GUARD_F, device=gpu)
        dst = dwhole[:, :, 2:, 1:1 + W]
    else:
        dwhole, dst = _guarded(gpu, (B, 1, H, W), torch.float32, GUARD_F, lead)
    out = {"depth": dst}
    ix = None
    if optional:
        rwhole, out["removed"] = _guarded(gpu, (B, H, W), torch.uint8, GUARD_B, 1 + lead)
        cwhole, out["counts"] = _guarded(gpu, (B, 2), torch.int32, GUARD_I, lead)
        if index is not None:
            iwhole, ix = _guarded(gpu, (B, H, W), torch.int32, GUARD_I, lead)
            ix.copy_(torch.from_numpy(index))
    before = src.clone()
    r = nconv_amd.remove_occluded(src, window, jump_abs=jump[0], jump_rel=jump[1], min_support=min_support, floor=floor,
                                  index=ix, return_removed=optional, return_counts=optional, out=out)
    torch.cuda.synchronize()
    assert torch.equal(src.view(torch.int32), before.view(torch.int32))  # the source is only read
    inside = torch.zeros_like(dwhole, dtype=torch.bool)
    (inside[:, :, 2:, 1:1 + W] if cropped else inside[lead:lead + B * H * W]).fill_(True)
    assert bool((dwhole.reshape(-1)[~inside.reshape(-1)] == GUARD_F).all())
    got = dict(dst=dst[:, 0].cpu().numpy(), removed=None, counts=None, index=None)
    if optional:
        assert r[0] is dst and r[1] is out["removed"] and r[2] is out["counts"]
        n = B * H * W
        assert bool((rwhole[:1 + lead] == GUARD_B).all()) and bool((rwhole[1 + lead + n:] == GUARD_B).all())
        assert bool((cwhole[:lead] == GUARD_I).all()) and bool((cwhole[lead + 2 * B:] == GUARD_I).all())
        got["removed"], got["counts"] = out["removed"].cpu().numpy(), out["counts"].cpu().numpy()
        if ix is not None:
            assert bool((iwhole[:lead] == GUARD_I).all()) and bool((iwhole[lead + n:] == GUARD_I).all())
            got["index"] = ix.cpu().numpy()
    else:
        assert r is dst
    return got


def _compare(got, ref, index=None, what=""):
    bad = int((got["dst"].view(np.uint32) != ref["dst"].view(np.uint32)).sum())
    assert bad == 0, (what, "dst", bad)
    if got["removed"] is not None:
        assert (got["removed"] == ref["removed"]).all(), (what, "removed")
        assert (got["counts"] == ref["counts"]).all(), (what, got["counts"], ref["counts"])
    if got["index"] is not None:
        assert (got["index"] == OC.index_ref(index, ref)).all(), (what, "index")


def _check(nconv_amd, gpu, z, window, *, jump=OC.JUMPS, min_support=1, floor=0.0, what="", **kw):
    ref = OC.occlusion_ref(z, window[0], window[1], jump[0], jump[1], min_support, floor)
    got = _run(nconv_amd, gpu, z, window, jump=jump, min_support=min_support, floor=floor, **kw)
    _compare(got, ref, kw.get("index"), (what, window, jump, min_support, floor))
    return got, ref


def _index_plane(z, seed=0):
    """A project_points-like index: a row number at every pixel, -1 at some of the empty ones."""
    ix = (np.arange(z.size, dtype=np.int32).reshape(z.shape) * 3 + 5)
    ix[(z == 0) & (np.random.default_rng(seed).random(z.shape) < 0.5)] = -1
    return ix


@pytest.mark.parametrize("shape", OC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sweep_matches_reference(nconv_amd, gpu, shape):
    B, H, W = shape
    removed_some = False
    for density in OC.DENSITIES:
        z = OC.plane(B, H, W, seed=100 + H + W, density=density)
        index = _index_plane(z)
        for window in OC.WINDOWS:
            for floor in OC.FLOORS:
                valid, support = OC.support_of(z, window[0], window[1], *OC.JUMPS, floor)  # once per window and floor
                for ms in OC.MIN_SUPPORTS:
                    ref = OC.finish(z, valid, support, ms)
                    got = _run(nconv_amd, gpu, z, window, min_support=ms, floor=floor, index=index)
                    _compare(got, ref, index, (shape, density, window, ms, floor))
                    removed_some |= bool(ref["removed"].any())
    assert removed_some or H * W == 1


@pytest.mark.parametrize("shape", ((3, 37, 71), (2, 71, 139)), ids=lambda s: "x".join(map(str, s)))
def test_views_and_optional_outputs(nconv_amd, gpu, shape):
    B, H, W = shape
    z = OC.plane(B, H, W, seed=7, density=0.3)
    index = _index_plane(z, 1)
    for window, ms, floor, jump in (((3, 3), 1, 0.0, OC.JUMPS), ((2, 5), 2, None, (0.25, 0.125)),
                                    ((16, 16), 7, 0.0, (0.0, 0.01))):
        kw = dict(jump=jump, min_support=ms, floor=floor)
        for view in (dict(cropped=True), dict(shifted=True), dict(cropped=True, shifted=True)):
            _check(nconv_amd, gpu, z, window, index=index, what="views", **kw, **view)
            _check(nconv_amd, gpu, z, window, optional=False, what="views, no optional output", **kw, **view)
        _check(nconv_amd, gpu, z, window, optional=False, what="no optional output", **kw)
        _check(nconv_amd, gpu, z, window, what="no index", **kw)
    # an (H, W) plane, an int window, floor=None, and the plain return value
    r = nconv_amd.remove_occluded(torch.from_numpy(z[0]).to(gpu), 2, floor=None)
    assert r.shape == (1, 1, H, W) and OC.same_bits(r[0, 0].cpu().numpy(), OC.occlusion_ref(z[:1], 2, 2, 1.0, 0.0, 1, None)["dst"][0])


# centres: the interior of a tile, the last row / column of the first tile and the first of the next (the
# window crosses the seam either way), and the four image corners
def _centres(H, W):
    return ((10, 20), (TH - 1, TW - 1), (TH, TW), (TH - 1, TW), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))


FORCED = (1, 40, 70)  # two tiles each way, the second ragged: the seams are at row 32 and column 64


def _inside(p, H, W):
    return 0 <= p[0] < H and 0 <= p[1] < W


def _stacked(nconv_amd, gpu, planes, window, **kw):
    """The forced planes of one test as the images of one batch: one call, one reference."""
    return _check(nconv_amd, gpu, np.concatenate(planes, axis=0), window, **kw)[0]


@pytest.mark.parametrize("window", ((3, 3), (2, 5), (16, 16), (16, 0), (0, 16)), ids=lambda w: f"{w[0]}x{w[1]}")
def test_forced_window_reach(nconv_amd, gpu, window):
    """A nearer return exactly rh rows or rw columns away removes the centre; at rh + 1 / rw + 1 it does not."""
    _, H, W = FORCED
    rh, rw = window
    planes, cases = [], []
    for ci, cj in _centres(H, W):
        for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            offsets = [((si * rh, sj * rw), True)]
            if si == sj:
                offsets += [((si * (rh + 1), sj * rw), False), ((si * rh, sj * (rw + 1)), False),
                            ((si * rh, 0), True), ((si * (rh + 1), 0), False), ((0, sj * rw), True), ((0, sj * (rw + 1)), False)]
            for (di, dj), want in offsets:
                q = (ci + di, cj + dj)
                if not _inside(q, H, W) or q == (ci, cj):
                    continue
                z = np.zeros(FORCED, dtype=F32)
                z[0, ci, cj], z[0, q[0], q[1]] = 30.0, 5.0
                planes.append(z)
                cases.append(((ci, cj), q, want))
    assert sum(c[2] for c in cases) >= 8 and sum(not c[2] for c in cases) >= 8
    got = _stacked(nconv_amd, gpu, planes, window, what="reach")
    for n, ((ci, cj), q, want) in enumerate(cases):
        assert bool(got["removed"][n, ci, cj]) == want, ((ci, cj), q, want)
        assert got["counts"][n].tolist() == [2, int(want)] and got["dst"][n, q[0], q[1]] == 5.0


def test_forced_strict_comparison(nconv_amd, gpu):
    """v_p bit-equal to lim(q) is kept (strict >); one ulp above is removed."""
    _, H, W = FORCED
    for vq, ja, jr in ((10.3, 0.7, 0.1), (5.0, 1.0, 0.0), (41.7, 0.0, 0.013), (1e-40, 0.0, 0.5)):
        lim = OC.lim_of(np.array([vq], dtype=F32), ja, jr)[0]
        up = np.nextafter(lim, F32(np.inf), dtype=F32)
        assert up > lim >= F32(vq)
        planes, cases = [], []
        for ci, cj in _centres(H, W):
            q = (ci + (2 if ci + 2 < H else -2), cj + (3 if cj + 3 < W else -3))
            for vp, want in ((lim, False), (up, True)):
                z = np.zeros(FORCED, dtype=F32)
                z[0, ci, cj], z[0, q[0], q[1]] = vp, vq
                planes.append(z)
                cases.append(((ci, cj), want))
        got = _stacked(nconv_amd, gpu, planes, (3, 3), jump=(ja, jr), what=("strict", vq))
        for n, ((ci, cj), want) in enumerate(cases):
            assert bool(got["removed"][n, ci, cj]) == want, (vq, ja, jr, (ci, cj), want)


@pytest.mark.parametrize("min_support", (2, 3, 7))
def test_forced_support_count(nconv_amd, gpu, min_support):
    """Exactly min_support - 1 supporters keep the centre, exactly min_support remove it."""
    _, H, W = FORCED
    offs = [(di, dj) for di in (-3, -1, 0, 2, 3) for dj in (-3, -2, 0, 1, 3) if (di, dj) != (0, 0)]
    planes, cases = [], []
    for ci, cj in _centres(H, W):
        qs = [(ci + di, cj + dj) for di, dj in offs if _inside((ci + di, cj + dj), H, W)]
        assert len(qs) >= min_support
        for k, want in ((min_support - 1, False), (min_support, True)):
            z = np.zeros(FORCED, dtype=F32)
            z[0, ci, cj] = 30.0
            for q in qs[:k]:
                z[0, q[0], q[1]] = 5.0
            for q in qs[k:k + 2]:
                z[0, q[0], q[1]] = 29.5  # valid neighbours that do not support
            planes.append(z)
            cases.append(((ci, cj), k, want))
    got = _stacked(nconv_amd, gpu, planes, (3, 3), min_support=min_support, what="count")
    for n, ((ci, cj), k, want) in enumerate(cases):
        assert bool(got["removed"][n, ci, cj]) == want, ((ci, cj), k)  # (the 29.5 m neighbours may go as well)


def test_forced_floor_none_border_and_halo(nconv_amd, gpu):
    """floor=None: zero and negative pixels are valid, but only those inside the image. The halo past the
    border (which the loads read as 0) supports nothing, so a plane of positive depths is not eaten from
    the border inwards; zeros and negatives on the border itself do support."""
    for shape in ((1, 5, 7), FORCED, (2, 37, 71)):
        B, H, W = shape
        z = np.full(shape, 7.0, dtype=F32)
        for window in ((3, 3), (16, 16), (2, 5)):
            got, _ = _check(nconv_amd, gpu, z, window, floor=None, what="ring", cropped=True)
            assert not got["removed"].any() and got["counts"].tolist() == [[H * W, 0]] * B
        # zeros and negatives on the border are valid neighbours: everything positive within reach goes
        zb = z.copy()
        zb[:, 0, 0], zb[:, H - 1, W - 1], zb[:, 0, W // 2], zb[:, H // 2, 0] = 0.0, -2.0, -0.0, -1e-40
        for window in ((3, 3), (16, 16)):
            got, ref = _check(nconv_amd, gpu, zb, window, floor=None, what="border values")
            assert got["removed"][:, 0, 1].all() and got["removed"][:, H - 1, W - 2].all()
            assert (got["dst"][:, H - 1, W - 1] == -2.0).all()
            _check(nconv_amd, gpu, zb, window, floor=0.0, what="border values, floor 0")
    # an isolated negative value is above its own lim: the centre is no candidate of its window
    z = np.full(FORCED, np.nan, dtype=F32)
    for ci, cj in _centres(*FORCED[1:]):
        z[0, ci, cj] = -2.0
    z[0, TH - 1, TW - 1] = z[0, TH - 1, TW] = np.nan  # keep the seam pair apart
    got, _ = _check(nconv_amd, gpu, z, (1, 1), jump=(0.5, 1.0), floor=None, what="own lim")
    assert not got["removed"].any() and got["counts"][0, 0] == 6


def test_forced_non_finite(nconv_amd, gpu):
    """NaN and +-inf centres are not valid (dst 0, index -1); as neighbours they support nothing."""
    _, H, W = FORCED
    specials = np.array([np.nan, np.inf, -np.inf], dtype=F32)
    for floor in OC.FLOORS:
        # floor None makes a zero a valid depth of 0 m, which would support: the background is 30 m there
        z = np.full(FORCED, 0.0 if floor is not None else 30.0, dtype=F32)
        want_kept = []
        for n, (ci, cj) in enumerate(_centres(H, W)):
            if (ci, cj) in ((TH, TW), (TH - 1, TW)):  # (TH - 1, TW - 1) and its neighbours lie across the seam
                continue
            di, dj = (1 if ci + 1 < H else -1), (1 if cj + 1 < W else -1)
            z[0, ci, cj] = 30.0
            z[0, ci + di, cj], z[0, ci, cj + dj], z[0, ci + di, cj + dj] = specials[n % 3], specials[(n + 1) % 3], specials[(n + 2) % 3]
            want_kept.append((ci, cj))
        index = _index_plane(z, 2)
        got, _ = _check(nconv_amd, gpu, z, (1, 1), floor=floor, index=index, what="non-finite")
        for ci, cj in want_kept:
            assert got["dst"][0, ci, cj] == 30.0 and got["index"][0, ci, cj] == index[0, ci, cj]
        bad = ~np.isfinite(z)
        assert (got["dst"].view(np.uint32)[bad] == 0).all() and (got["index"][bad] == -1).all() and not got["removed"][bad].any()
        # beside a real nearer return the centre still goes
        z[0, 10, 21] = 5.0
        got, _ = _check(nconv_amd, gpu, z, (1, 1), floor=floor, index=index, what="non-finite and one nearer")
        assert got["removed"][0, 10, 20] == 1 and got["index"][0, 10, 20] == -1


def test_refuses_overlap_and_bad_outputs(nconv_amd, gpu):
    z = torch.rand(2, 1, 8, 16, device=gpu) + 1.0
    before = z.clone()
    with pytest.raises(RuntimeError, match="overlaps src"):
        nconv_amd.remove_occluded(z, out={"depth": z})
    with pytest.raises(RuntimeError, match="overlaps src"):
        nconv_amd.remove_occluded(z[:, :, :6], out={"depth": z[:, :, 2:]})
    with pytest.raises(TypeError, match="out\\['depth'\\]"):
        nconv_amd.remove_occluded(z, out={"depth": torch.ones(2, 1, 8, 15, device=gpu)})
    with pytest.raises(TypeError, match="out\\['removed'\\]"):
        nconv_amd.remove_occluded(z, out={"removed": torch.ones(2, 8, 16, device=gpu)}, return_removed=True)
    with pytest.raises(TypeError, match="out\\['counts'\\]"):
        nconv_amd.remove_occluded(z, out={"counts": torch.ones(2, dtype=torch.int32, device=gpu)}, return_counts=True)
    torch.cuda.synchronize()
    assert torch.equal(z, before)


def test_filter_under_graph_capture(nconv_amd, gpu):
    B, H, W = 2, 37, 71
    za, zb = OC.plane(B, H, W, seed=51, density=0.3), OC.plane(B, H, W, seed=52, density=0.1)
    src = torch.from_numpy(za)[:, None].to(gpu)
    flt = nconv_amd.OcclusionFilter((H, W), B=B, window=(2, 5), min_support=2, floor=None, return_removed=True,
                                    return_counts=True)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        flt(src)  # warm-up: the buffers exist before the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, removed, counts = flt(src)
    for z in (za, zb, za):
        src.copy_(torch.from_numpy(z)[:, None])
        for t in (out, removed, counts):
            t.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        got = dict(dst=out[:, 0].cpu().numpy(), removed=removed.cpu().numpy(), counts=counts.cpu().numpy(), index=None)
        e = nconv_amd.remove_occluded(src, (2, 5), min_support=2, floor=None, return_removed=True, return_counts=True)
        assert torch.equal(out.view(torch.int32), e[0].view(torch.int32))
        assert torch.equal(removed, e[1]) and torch.equal(counts, e[2])
        _compare(got, OC.occlusion_ref(z, 2, 5, 1.0, 0.0, 2, None), what="replay")


def test_remove_occluded_stage_behind_the_prefetcher(nconv_amd, gpu):
    rng = np.random.default_rng(6)
    B, h, w = 2, 37, 71
    metres = OC.plane(2 * B, h, w, seed=61, density=0.3, specials=False)
    raw = np.rint(metres * 256.0).astype(np.uint16)
    batches = [{"depth": torch.from_numpy(raw[:B]), "gt": torch.from_numpy(raw[B:]), "name": "a",
                "k": torch.from_numpy(rng.random((B, 3, 3)).astype(F32))},
               {"depth": torch.from_numpy(raw[B:]), "gt": torch.from_numpy(raw[:B]), "name": "b",
                "k": torch.from_numpy(rng.random((B, 3, 3)).astype(F32))}]
    ingest = nconv_amd.Ingest(depth_decode="kitti16")
    stage = nconv_amd.RemoveOccluded(chain=ingest, window=(2, 5), jump_abs=0.5, jump_rel=0.01)
    got = list(nconv_amd.data.DevicePrefetcher(batches, gpu, ingest=stage))
    torch.cuda.synchronize()
    assert len(got) == 2
    removed = 0
    for raw_batch, b in zip(batches, got):
        plain = ingest({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in raw_batch.items()})
        want = nconv_amd.remove_occluded(plain["depth"], (2, 5), jump_abs=0.5, jump_rel=0.01)
        assert sorted(b) == sorted(raw_batch) and b["name"] == raw_batch["name"]
        assert b["depth"].shape == (B, 1, h, w) and torch.equal(b["depth"].view(torch.int32), want.view(torch.int32))
        assert torch.equal(b["gt"], plain["gt"]) and torch.equal(b["k"].cpu(), raw_batch["k"])
        z = plain["depth"][:, 0].cpu().numpy()
        ref = OC.occlusion_ref(z, 2, 5, 0.5, 0.01, 1, 0.0)
        assert OC.same_bits(b["depth"][:, 0].cpu().numpy(), ref["dst"])
        removed += int(ref["removed"].sum())
    assert removed > 0
    # without a chain the stage filters an fp32 batch as it is
    f = nconv_amd.RemoveOccluded()({"depth": torch.from_numpy(metres[:B])[:, None].to(gpu), "x": 1})
    assert f["x"] == 1 and OC.same_bits(f["depth"][:, 0].cpu().numpy(), OC.occlusion_ref(metres[:B], 3, 3, 1.0, 0.0, 1, 0.0)["dst"])


def test_composes_with_project_points(nconv_amd, gpu):
    """remove_occluded(*project_points(..., return_index=True)): the -1 entries of the index are exactly
    the removed and the empty pixels, and its other entries are the rows project_points named."""
    B, H, W, rows = 3, 37, 71, 1500
    pts, off, m, _ = LC.scan(np.random.default_rng(9), B, H, W, rows)
    p = LC.project_ref(pts, off, m, (H, W))
    args = (torch.from_numpy(pts).to(gpu), torch.from_numpy(off).to(gpu), torch.from_numpy(m).to(gpu), (H, W))
    depth, index = nconv_amd.project_points(*args, return_index=True)
    assert torch.equal(index.cpu(), torch.from_numpy(p["index"]))
    out = nconv_amd.remove_occluded(*nconv_amd.project_points(*args, return_index=True, out={"index": index}))
    torch.cuda.synchronize()
    ref = OC.occlusion_ref(p["depth"][:, 0], 3, 3, 1.0, 0.0, 1, 0.0)
    assert ref["removed"].sum() > 20
    assert OC.same_bits(out[:, 0].cpu().numpy(), ref["dst"])
    ix = index.cpu().numpy()
    assert ((ix == -1) == ((ref["removed"] != 0) | (p["index"] == -1))).all()
    assert (ix[ix >= 0] == p["index"][ix >= 0]).all()
    # the same with keywords and the removed mask
    d2, i2 = nconv_amd.project_points(*args, return_index=True)
    o2, rm = nconv_amd.remove_occluded(d2, index=i2, return_removed=True)
    assert torch.equal(o2, out) and torch.equal(i2, index) and (rm.cpu().numpy() == ref["removed"]).all()
