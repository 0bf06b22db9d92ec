"""GPU: nconv_depth_sparsify against the numpy reference (tests/sparsify_cases.py) bit for bit, depth and
kept, with guard bands around the outputs and the workspace: the shape sweep with every mode, the counts
around C_b, masks, both candidate rules, special values, cropped and misaligned views, in place; forced
ties; noise; a reused workspace; Sparsifier under torch.cuda.graph; SparsifyBatch behind
DevicePrefetcher."""
import numpy as np
import pytest
import torch

import sparsify_cases as SC

pytestmark = pytest.mark.gpu

GUARD_F, GUARD_I, GUARD_B = -7.0, -77, 0x5A
F32 = np.float32


def _source(gpu, z, cropped, shifted):
    """z (B, H, W) as a (B, 1, H, W) device view: contiguous, or a window of a larger plane of other values;
    shifted: the base one element past a 16-byte boundary."""
    B, H, W = z.shape
    lead = 1 if shifted else 0
    hh, ww = (H + 3, W + 5) if cropped else (H, W)
    whole = torch.full((B * hh * ww + lead + 3,), 123.0, device=gpu)
    big = whole[lead:lead + B * hh * ww].view(B, 1, hh, ww)
    v = big[:, :, 1:1 + H, 2:2 + W] if cropped else big
    v.copy_(torch.from_numpy(z)[:, None])
    assert v.data_ptr() % 16 == (4 * (lead + (ww + 2 if cropped else 0))) % 16
    return v


def _guarded(gpu, shape, dtype, guard, lead):
    n = int(np.prod(shape))
    whole = torch.full((n + lead + 5,), guard, dtype=dtype, device=gpu)
    return whole, whole[lead:lead + n].view(shape)


def _run(nconv_amd, gpu, z, n=None, *, mask=None, cropped=False, shifted=False, inplace=False, ws=None, **kw):
    """One call with guarded outputs; returns (depth (B, H, W), kept) as numpy after checking the guards."""
    B, H, W = z.shape
    src = _source(gpu, z, cropped, shifted)
    lead = 1 if shifted else 0
    if inplace:
        dst, dwhole = src, None
    elif cropped:
        dwhole = torch.full((B, 1, H + 2, W + 3), GUARD_F, device=gpu)
        dst = dwhole[:, :, 2:, 1:1 + W]
    else:
        dwhole, dst = _guarded(gpu, (B, 1, H, W), torch.float32, GUARD_F, lead)
    kwhole, kept = _guarded(gpu, (B,), torch.int32, GUARD_I, lead)
    nws = nconv_amd._lib.lib().nconv_depth_sparsify_workspace_bytes(B, H, W)
    wwhole, w = _guarded(gpu, (nws,), torch.uint8, GUARD_B, 8 * lead) if ws is None else ws
    if mask is not None:
        mask = torch.from_numpy(mask).to(gpu)
        mask = mask[:, None] if mask.dim() == 3 else mask
    if n is not None and np.ndim(n) == 1:
        n = torch.tensor(n, dtype=torch.int32, device=gpu)
    before = src.clone()
    r, k = nconv_amd.sparsify(src, n, mask=mask, return_kept=True, out={"depth": dst, "kept": kept, "workspace": w}, **kw)
    torch.cuda.synchronize()
    assert r is dst and k is kept
    if not inplace:
        assert torch.equal(src.view(torch.int32), before.view(torch.int32))  # the source is only read
        flat = dwhole.reshape(-1)
        inside = torch.zeros_like(dwhole, dtype=torch.bool)
        (inside[:, :, 2:, 1:1 + W] if cropped else inside[lead:lead + B * H * W]).fill_(True)
        assert bool((flat[~inside.reshape(-1)] == GUARD_F).all())
    assert bool((kwhole[:lead] == GUARD_I).all()) and bool((kwhole[lead + B:] == GUARD_I).all())
    assert bool((wwhole[:8 * lead] == GUARD_B).all()) and bool((wwhole[8 * lead + nws:] == GUARD_B).all())
    return dst[:, 0].cpu().numpy(), kept.cpu().numpy()


def _check(nconv_amd, gpu, z, n=None, *, mask=None, what="", **kw):
    ref_kw = {k: v for k, v in kw.items() if k not in ("cropped", "shifted", "inplace", "ws")}
    ref, rkept, _, noisy = SC.sparsify_ref(z, n, mask=mask, detail=True, **ref_kw)
    got, kept = _run(nconv_amd, gpu, z, n, mask=mask, **kw)
    assert (kept == rkept).all(), (what, n, kw, kept, rkept)
    assert SC.same_bits(got, ref, noisy), (what, n, kw, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
    return got, kept


def _counts(z, mask=None, floor=0.0):
    C = SC.candidates(z, mask, floor).reshape(z.shape[0], -1).sum(1)
    return sorted({v for v in (0, 1, int(C.min()) - 1, int(C.min()), int(C.max()), int(C.max()) + 5) if v >= 0})


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sweep_matches_reference(nconv_amd, gpu, shape):
    B, H, W = shape
    z = SC.plane(B, H, W, seed=10 + H)
    shared, per = SC.masks(B, H, W, seed=H)
    seed = (0x9E3779B9 << 32) | (0xC0FFEE00 + W)
    # every mode; the counts around C_b; both candidate rules
    _check(nconv_amd, gpu, z, seed=seed, what="all")
    _check(nconv_amd, gpu, z, seed=seed, floor=None, what="all, every pixel")
    for floor in (0.0, None, 20.0):
        for n in _counts(z, None, floor):
            _check(nconv_amd, gpu, z, n, seed=seed, draw=n, floor=floor, what="count")
    C = SC.candidates(z).reshape(B, -1).sum(1)
    per_image = [(-3, 0, 1, 10 ** 6)[b % 4] if b else int(C[0]) - 1 for b in range(B)]
    _check(nconv_amd, gpu, z, per_image, seed=seed, what="count_dev")
    _check(nconv_amd, gpu, z, [max(int(c) // 2, 0) for c in C], seed=seed, floor=None, what="count_dev")
    for keep in (0.0, 0.25, 0.999, 1.0):
        _check(nconv_amd, gpu, z, keep=keep, seed=seed, what="fraction")
    # masks, shared and per image
    for m in (shared, per):
        _check(nconv_amd, gpu, z, mask=m, seed=seed, what="mask, all")
        _check(nconv_amd, gpu, z, mask=m, seed=seed, floor=None, what="mask, all, every pixel")
        for n in _counts(z, m):
            _check(nconv_amd, gpu, z, n, mask=m, seed=seed, what="mask, count")
    # views, alignment, in place
    n = max(int(C.min()) // 2, 1)
    for kw in (dict(cropped=True), dict(shifted=True), dict(cropped=True, shifted=True), dict(inplace=True),
               dict(inplace=True, cropped=True), dict(inplace=True, shifted=True)):
        got, _ = _check(nconv_amd, gpu, z, n, seed=seed, noise_frac=0.3, what="views", **kw)
        _check(nconv_amd, gpu, z, n, seed=seed, floor=None, mask=per, what="views", **kw)
    # another draw or seed is another set (where there is a choice to make)
    if int(C.min()) >= 8:
        a = _run(nconv_amd, gpu, z, n, seed=seed, draw=0)[0]
        assert (a != _run(nconv_amd, gpu, z, n, seed=seed, draw=1)[0]).any()
        assert (a != _run(nconv_amd, gpu, z, n, seed=seed + 1, draw=0)[0]).any()


@pytest.fixture(scope="module")
def big_case():
    B, H, W = SC.BIG
    z = SC.plane(B, H, W, seed=77, density=0.3)
    _, per = SC.masks(B, H, W, seed=78)
    return z, per


def test_kitti_size_matches_reference(nconv_amd, gpu, big_case):
    z, per = big_case
    _check(nconv_amd, gpu, z, 20000, seed=5, draw=2, noise_frac=0.1, what="big, count")
    _check(nconv_amd, gpu, z, keep=0.37, seed=5, mask=per, floor=None, cropped=True, what="big, fraction")


@pytest.mark.parametrize("shape", ((3, 9, 13), (2, 64, 257)), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("key_mask", (0, 0xF0000000, 0xFFFF0000))
def test_ties_break_on_the_pixel_number(nconv_amd, gpu, shape, key_mask):
    B, H, W = shape
    z = SC.plane(B, H, W, seed=21)
    for floor in (0.0, None):
        for n in _counts(z, None, floor) + [H * W // 3]:
            got, kept = _check(nconv_amd, gpu, z, n, seed=3, floor=floor, key_mask=key_mask, what="ties")
    if key_mask == 0:  # raster-first
        got, kept = _run(nconv_amd, gpu, z, 7, seed=3, key_mask=0)
        cand = SC.candidates(z)
        for b in range(B):
            assert (np.flatnonzero(got[b].reshape(-1)) == np.flatnonzero(cand[b].reshape(-1))[:7]).all()


@pytest.mark.parametrize("shape", ((3, 9, 13), (2, 64, 257)), ids=lambda s: "x".join(map(str, s)))
def test_noise_matches_reference(nconv_amd, gpu, shape):
    B, H, W = shape
    z = SC.plane(B, H, W, seed=31)
    for frac, amp, floor in ((0.1, 0.1, 0.0), (0.5, 0.1, 0.0), (1.0, 0.25, 0.0), (0.5, 0.1, None), (1.0, 3.0, None)):
        ref, _, km, nm = SC.sparsify_ref(z, seed=9, noise_frac=frac, noise_amp=amp, floor=floor, detail=True)
        assert nm.any() and (frac < 1.0 or (nm == km).all())
        got, _ = _check(nconv_amd, gpu, z, seed=9, noise_frac=frac, noise_amp=amp, floor=floor, what="noise")
        finite = nm & np.isfinite(ref)
        assert finite.any() and (got[finite].view(np.uint32) == ref[finite].view(np.uint32)).all()
        _check(nconv_amd, gpu, z, H * W // 4, seed=9, noise_frac=frac, noise_amp=amp, floor=floor, what="noise, count")


def test_workspace_reuse_leaves_no_stale_state(nconv_amd, gpu):
    B, H, W = 2, 64, 257
    z = SC.plane(B, H, W, seed=41)
    nws = nconv_amd._lib.lib().nconv_depth_sparsify_workspace_bytes(B, H, W)
    ws = _guarded(gpu, (nws,), torch.uint8, GUARD_B, 0)
    for n, kw in ((5000, {}), (3, {}), (None, dict(keep=0.5)), (0, {}), (700, dict(key_mask=0xFF000000)), (5000, {})):
        _check(nconv_amd, gpu, z, n, seed=1, ws=ws, what="reuse", **kw)
    ws[1].fill_(0xFF)  # whatever the workspace held
    _check(nconv_amd, gpu, z, 5000, seed=1, ws=ws, what="reuse")


def test_sparsifier_under_graph_capture(nconv_amd, gpu):
    B, H, W = 2, 37, 71
    z = SC.plane(B, H, W, seed=51)
    src = torch.from_numpy(z)[:, None].to(gpu)
    sp = nconv_amd.Sparsifier((H, W), B=B, seed=77, draw=5, noise_frac=0.2)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        sp(src, 300)  # warm-up: buffers and state exist before the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    sp.reset(5)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, kept = sp(src, 300, return_kept=True)
    sets = []
    for rep in range(3):
        g.replay()
        torch.cuda.synchronize()
        ref, rkept, _, noisy = SC.sparsify_ref(z, 300, seed=77, draw=5 + rep, noise_frac=0.2, detail=True)
        got = out[:, 0].cpu().numpy()
        assert SC.same_bits(got, ref, noisy) and (kept.cpu().numpy() == rkept).all(), rep
        sets.append(got != 0)
    assert (sets[0] != sets[1]).any() and (sets[1] != sets[2]).any() and (sets[0] != sets[2]).any()
    assert sp.state.cpu().tolist()[2] == 8
    sp.reset(5)
    g.replay()
    torch.cuda.synchronize()
    ref, _, _, noisy = SC.sparsify_ref(z, 300, seed=77, draw=5, noise_frac=0.2, detail=True)
    assert SC.same_bits(out[:, 0].cpu().numpy(), ref, noisy)
    # advance=False: the same sample on every call
    fixed = nconv_amd.Sparsifier((H, W), B=B, seed=77, draw=5, advance=False, noise_frac=0.2)
    a = fixed(src, 300).clone()
    assert torch.equal(a.view(torch.int32), fixed(src, 300).view(torch.int32))
    assert SC.same_bits(a[:, 0].cpu().numpy(), ref, noisy)


def test_sparsify_batch_behind_the_prefetcher(nconv_amd, gpu):
    B, H, W = 2, 37, 71
    z = SC.plane(B, H, W, seed=61, specials=False)
    _, per = SC.masks(B, H, W, seed=62)
    n_keep = [H * W - 900, H * W - 17]
    gt = torch.from_numpy(z)[:, None]
    batches = [{"depth": gt.clone(), "gt": gt.clone(), "mask": torch.from_numpy(per)[:, None], "name": "a"},
               {"depth": gt.clone(), "gt": gt.clone(), "n_keep": torch.tensor(n_keep, dtype=torch.int32), "name": "b"}]
    seen = []

    def chain(batch):
        seen.append(sorted(batch))
        return batch
    for add_noise in (False, True):
        stage = nconv_amd.SparsifyBatch(seed=13, add_noise=add_noise, chain=chain)
        pf = nconv_amd.data.DevicePrefetcher(batches, gpu, keys=("depth", "gt", "mask", "n_keep"), ingest=stage)
        got = list(pf)
        torch.cuda.synchronize()
        assert len(got) == 2 and seen[-2:] == [["depth", "gt", "name"]] * 2
        noise = dict(noise_frac=0.1, noise_amp=0.1) if add_noise else {}
        ref0, _, _, ny0 = SC.sparsify_ref(z, mask=per, floor=None, seed=13, draw=0, detail=True, **noise)
        ref1, k1, _, ny1 = SC.sparsify_ref(z, n_keep, floor=None, seed=13, draw=1, detail=True, **noise)
        assert k1.tolist() == n_keep and (not add_noise or (ny0.any() and ny1.any()))
        assert SC.same_bits(got[0]["depth"][:, 0].cpu().numpy(), ref0, ny0)
        assert SC.same_bits(got[1]["depth"][:, 0].cpu().numpy(), ref1, ny1)
        if not add_noise:  # the reference's rule: the ground truth times the mask
            assert SC.same_bits(ref0, np.where(per != 0, z, F32(0)))
        for b in got:
            assert torch.equal(b["gt"].cpu(), gt) and b["depth"].shape == (B, 1, H, W)


def test_refuses_partial_overlap_and_bad_outputs(nconv_amd, gpu):
    z = torch.ones(2, 1, 8, 16, device=gpu)
    with pytest.raises(RuntimeError, match="overlaps src"):
        nconv_amd.sparsify(z[:, :, :6], 3, out={"depth": z[:, :, 2:]})
    with pytest.raises(TypeError, match="out\\['depth'\\]"):
        nconv_amd.sparsify(z, 3, out={"depth": torch.ones(2, 1, 8, 15, device=gpu)})
    with pytest.raises(TypeError, match="out\\['kept'\\]"):
        nconv_amd.sparsify(z, 3, out={"kept": torch.ones(2, device=gpu)}, return_kept=True)
    with pytest.raises(TypeError, match="out\\['workspace'\\]"):
        nconv_amd.sparsify(z, 3, out={"workspace": torch.ones(16, dtype=torch.uint8, device=gpu)})
    r = nconv_amd.sparsify(z[0, 0], 5, seed=4)  # an (H, W) plane
    assert r.shape == (1, 1, 8, 16) and int((r != 0).sum()) == 5
