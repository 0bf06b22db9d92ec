"""CPU: the Philox known answers on the numpy reference and on a C host of csrc/philox.h; the invariants
of the reference selection (exact counts, nesting, raster-first, views); its uniformity and noise share
at KITTI size; the two entry points exported, declared and bound with the C struct's layout under an
unchanged ABI number; every malformed call fails on the host with -22 before any launch; the Python
function refuses CPU tensors and malformed arguments; DataLoader_NYU(sparse="device") samples carry the
right keys and sparse="host" is bit-identical to the reference's preprocess_depth."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

import host_harness
import sparsify_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
NEW = ("nconv_depth_sparsify_workspace_bytes", "nconv_depth_sparsify")
F32, U32 = np.float32, np.uint32


# ---- Philox ----------------------------------------------------------------------------------------
def test_philox_known_answers_reference():
    for ctr, key, want in SC.KNOWN_ANSWERS:
        assert SC.words_hex(SC.philox4x32_10(*ctr, *key)) == want
    # vectorised = element by element
    p = np.array([0, 1, 0xFFFFFFFF, 12345], dtype=np.uint64)
    w = SC.philox4x32_10(p, 3, 7, 0, 0xDEADBEEF, 0x1234)
    for i, pi in enumerate(p):
        one = SC.philox4x32_10(int(pi), 3, 7, 0, 0xDEADBEEF, 0x1234)
        assert [int(x[i]) for x in w] == [int(x) for x in one]


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "sparsify_host", csrc=True)


def test_philox_known_answers_host(host_report):
    for name, (_, _, want) in zip(("kat_zeros", "kat_ones", "kat_pi"), SC.KNOWN_ANSWERS):
        assert host_report[name] == want


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    S = nconv_amd._lib.NconvDepthSparsify
    want = host_harness.ctypes_layout(S, "nconv_depth_sparsify")
    c = {k: v for k, v in host_report.items() if k.startswith("nconv_depth_sparsify")}
    assert len(c) == 20 and c == want


def test_host_calls(host_report):
    assert host_report["abi"] == [27, 27]
    need, none = host_report["workspace_bytes"]
    assert need == 6 * (2048 * 4 + 16) and none == 0
    for key, msg in (("rc_workspace", "workspace too small"), ("rc_row_stride", "row stride"), ("rc_state", "null state"),
                     ("rc_mode", "unknown mode"), ("rc_overlap", "overlaps src"),
                     ("rc_dst_image_stride", "dst: image stride"), ("rc_mask_row_stride", "mask: row stride"),
                     ("rc_mask_image_stride", "mask: image stride"), ("rc_stride_cap", "too large")):
        rc, err = host_report[key]
        assert rc == -22 and msg in err, (key, rc, err)


# ---- the reference ---------------------------------------------------------------------------------
def test_reference_counts_and_nesting():
    B, H, W = 3, 9, 13
    z = SC.plane(B, H, W, seed=3)
    cand = SC.candidates(z)
    C = cand.reshape(B, -1).sum(1)
    assert (C > 5).all() and (C < H * W).all()
    prev = np.zeros((B, H, W), dtype=bool)
    for n in (0, 1, 5, int(C.min()) - 1, int(C.min()), int(C.max()) + 5):
        out, kept, km, nm = SC.sparsify_ref(z, n, seed=11, detail=True)
        assert (kept == np.minimum(n, C)).all() and (km.reshape(B, -1).sum(1) == kept).all()
        assert not (km & ~cand).any() and not nm.any()
        assert SC.same_bits(out[km], z[km]) and (out[~km].view(U32) == 0).all()
        assert (km | prev).sum() == km.sum()  # nested in n for one seed
        prev = km
    assert (prev == cand).all()  # n >= C_b keeps every candidate
    out, kept = SC.sparsify_ref(z)
    assert (kept == C).all() and SC.same_bits(out, np.where(cand, z, F32(0)))
    out, kept = SC.sparsify_ref(z, [4, -2, 1000])
    assert kept.tolist() == [4, 0, int(C[2])]
    out, kept = SC.sparsify_ref(z, keep=0.5)
    assert kept.tolist() == [int(np.floor(0.5 * c)) for c in C]
    # all_pixels: NaN, inf and empty pixels are candidates and are copied bit for bit
    out, kept, km, _ = SC.sparsify_ref(z, H * W - 3, floor=None, detail=True)
    assert (kept == H * W - 3).all() and SC.same_bits(out[km], z[km])


def test_reference_masks_order_and_views():
    B, H, W = 3, 9, 13
    z = SC.plane(B, H, W, seed=4)
    shared, per = SC.masks(B, H, W)
    for m in (shared, per):
        cand = SC.candidates(z, m)
        assert (cand == (SC.candidates(z) & (np.broadcast_to(m, z.shape) != 0))).all()
        _, _, km, _ = SC.sparsify_ref(z, 7, mask=m, detail=True)
        assert not (km & ~cand).any() and (km.reshape(B, -1).sum(1) == np.minimum(7, cand.reshape(B, -1).sum(1))).all()
    # key_mask = 0: the first n candidates in raster order
    _, _, km, _ = SC.sparsify_ref(z, 6, key_mask=0, detail=True)
    cand = SC.candidates(z)
    for b in range(B):
        first = np.flatnonzero(cand[b].reshape(-1))[:6]
        assert (np.flatnonzero(km[b].reshape(-1)) == first).all()
    # a coarse key ties: the kept set differs from the full key's and still has exactly n members
    _, kept, k4, _ = SC.sparsify_ref(z, 6, key_mask=0xF0000000, detail=True)
    assert (kept == 6).all() and (k4 != SC.sparsify_ref(z, 6, detail=True)[2]).any()
    # another draw, seed or image index gives another set
    base = SC.sparsify_ref(z, 20, seed=5, draw=0, detail=True)[2]
    assert (base != SC.sparsify_ref(z, 20, seed=5, draw=1, detail=True)[2]).any()
    assert (base != SC.sparsify_ref(z, 20, seed=5 + (1 << 32), draw=0, detail=True)[2]).any()
    same = np.repeat(z[:1], 2, axis=0)
    k2 = SC.sparsify_ref(same, 20, seed=5, floor=None, detail=True)[2]
    assert (k2[0] != k2[1]).any()
    # a view and its copy agree: the words belong to the logical pixel number
    big = SC.plane(B, H + 4, W + 6, seed=5)
    view = big[:, 2:2 + H, 3:3 + W]
    a, b = SC.sparsify_ref(view, 9, noise_frac=0.5), SC.sparsify_ref(view.copy(), 9, noise_frac=0.5)
    assert SC.same_bits(a[0], b[0]) and (a[1] == b[1]).all()


def test_reference_noise_arithmetic():
    z = SC.plane(2, 37, 71, seed=6, specials=False)
    out, kept, km, nm = SC.sparsify_ref(z, 900, noise_frac=0.25, noise_amp=0.1, seed=2, detail=True)
    assert nm.any() and not (nm & ~km).any()
    quiet = km & ~nm
    assert SC.same_bits(out[quiet], z[quiet])
    rel = (out[nm].astype(np.float64) - z[nm]) / z[nm]
    assert (np.abs(rel) <= 0.1 * (1 + 2.0 ** -20)).all() and rel.min() < -0.05 and rel.max() > 0.05
    assert SC.noise_threshold(0.0) == 0 and SC.noise_threshold(1.0) == 0xFFFFFFFF
    assert SC.noise_threshold(0.1) == int(np.floor(0.1 * 2.0 ** 32))


@pytest.fixture(scope="module")
def kitti_draws():
    """Seeds 0..7 at (1, 352, 1216), every pixel a candidate: n = 20000, and all of them with noise on a tenth."""
    z = np.full((1, 352, 1216), 5.0, dtype=F32)
    res = []
    for seed in range(8):
        _, kept, km, nm = SC.sparsify_ref(z, 20000, seed=seed, draw=0, floor=None, noise_frac=0.1, detail=True)
        w0 = SC.philox4x32_10(np.arange(352 * 1216, dtype=np.uint64), 0, 0, 0, seed, 0)[0]
        _, every, _, nall = SC.sparsify_ref(z, seed=seed, draw=0, floor=None, noise_frac=0.1, detail=True)
        assert every[0] == z.size and not (nm & ~nall).any()  # the words do not depend on n
        res.append((int(kept[0]), km[0], nall[0], w0.size - np.unique(w0).size))
    return res


def test_reference_uniformity(kitti_draws):
    """Pearson's statistic over the 8 x 16 grid of 44 x 76 tiles stays below the 99.9 % quantile of
    chi-squared with 127 degrees of freedom."""
    for seed, (kept, km, _, ties) in enumerate(kitti_draws):
        x2 = SC.chi2_tiles(km)
        print(f"seed {seed}: chi2 {x2:.1f}, tied 32-bit keys {ties}")
        assert kept == 20000 == int(km.sum())
        assert x2 < 181.99
        assert ties > 0  # the tie-break on the pixel number is live at this size


def test_reference_noise_share(kitti_draws):
    """Over all 352 x 1216 pixels kept (mode ALL): a standard deviation of 0.00046, so +-0.003 is wide of
    chance and narrow enough to catch a threshold that is off by a few per cent."""
    for seed, (_, _, nm, _) in enumerate(kitti_draws):
        share = nm.sum() / nm.size
        print(f"seed {seed}: noisy share {share:.4f}")
        assert abs(share - 0.1) <= 0.003


# ---- ABI -------------------------------------------------------------------------------------------
def test_entry_points_exported_and_abi_unchanged(nconv_amd):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", src, re.M))
    lib = nconv_amd._lib.lib()
    for name in NEW:
        assert name in declared and name in nconv_amd._lib.EXPORTED
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    v = int(re.search(r"#define NCONV_ABI_VERSION (\d+)", src).group(1))
    assert lib.nconv_abi_version() == v == nconv_amd._lib.ABI_VERSION == 27
    L = nconv_amd._lib
    assert (L.SPARSIFY_ALL, L.SPARSIFY_COUNT, L.SPARSIFY_COUNT_DEV, L.SPARSIFY_FRACTION) == (0, 1, 2, 3)
    assert lib.nconv_depth_sparsify_workspace_bytes(2, 4, 8) == 2 * 6 * (2048 * 4 + 16)
    for bad in ((0, 4, 8), (2, -1, 8), (2, 4, 0), (1 << 15, 1 << 8, 1 << 8)):
        assert lib.nconv_depth_sparsify_workspace_bytes(*bad) == 0


# ---- host validation -------------------------------------------------------------------------------
FAKE = {n: 0x100000 * (q + 1) for q, n in enumerate(("src", "dst", "mask", "state", "n_dev", "kept", "ws"))}


def _call(L, dst=FAKE["dst"], dbs=32, drs=8, kept=FAKE["kept"], ws=FAKE["ws"], ws_bytes=None, desc=True, **kw):
    """A valid B=2, 4 x 8 COUNT call (contiguous planes), then one defect."""
    lib = L.lib()
    d = L.NconvDepthSparsify()
    d.B, d.H, d.W, d.mode = 2, 4, 8, L.SPARSIFY_COUNT
    d.src, d.src_image_stride, d.src_row_stride = FAKE["src"], 32, 8
    d.state, d.n, d.keep, d.key_mask = FAKE["state"], 5, 0.5, 0xFFFFFFFF
    for k, v in kw.items():
        setattr(d, k, v)
    need = lib.nconv_depth_sparsify_workspace_bytes(2, 4, 8)
    rc = lib.nconv_depth_sparsify(ctypes.byref(d) if desc else None, dst, dbs, drs, kept, ws,
                                  need if ws_bytes is None else ws_bytes, None)
    return rc, lib.nconv_last_error().decode()


BAD_CALLS = [
    (dict(desc=False), "null descriptor"),
    (dict(src=None), "null src or dst"),
    (dict(dst=None), "null src or dst"),
    (dict(state=None), "null state"),
    (dict(B=0), "non-positive"),
    (dict(H=-1), "non-positive"),
    (dict(W=0), "non-positive"),
    (dict(src_row_stride=7), "src: row stride"),
    (dict(drs=7), "dst: row stride"),
    (dict(mask=FAKE["mask"], mask_row_stride=7, mask_image_stride=0), "mask: row stride"),
    (dict(src_image_stride=31), "src: image stride"),
    (dict(dbs=31), "dst: image stride"),
    (dict(mask=FAKE["mask"], mask_row_stride=8, mask_image_stride=31), "mask: image stride"),
    (dict(B=1 << 15, H=1 << 8, W=1 << 8, src_image_stride=1 << 16, src_row_stride=1 << 8), "below 2^31"),
    (dict(mode=4), "unknown mode"),
    (dict(mode=-1), "unknown mode"),
    (dict(mode=2), "COUNT_DEV without n_dev"),
    (dict(n=-1), "negative n"),
    (dict(keep=-0.25), "keep must be"),
    (dict(keep=1.5), "keep must be"),
    (dict(keep=float("nan")), "keep must be"),
    (dict(ws=None), "workspace too small"),
    (dict(ws_bytes=2 * 6 * (2048 * 4 + 16) - 1), "workspace too small"),
    (dict(ws=FAKE["ws"] + 4), "8-byte aligned"),
    (dict(src=FAKE["src"] + 2), "4-byte aligned"),
    (dict(dst=FAKE["dst"] + 1), "4-byte aligned"),
    (dict(state=FAKE["state"] + 2), "4-byte aligned"),
    (dict(kept=FAKE["kept"] + 2), "4-byte aligned"),
    (dict(mode=2, n_dev=FAKE["n_dev"] + 1), "4-byte aligned"),
    # dst inside src's extent without being src: one row down, the same pointer with other strides
    (dict(dst=FAKE["src"] + 32), "overlaps src"),
    (dict(dst=FAKE["src"], drs=16, dbs=64), "overlaps src"),
    (dict(dst=FAKE["src"] - 4 * 63), "overlaps src"),
]


@pytest.mark.parametrize("bad,msg", BAD_CALLS)
def test_call_rejects_malformed_arguments(nconv_amd, bad, msg):
    rc, err = _call(nconv_amd._lib, **bad)
    assert rc == -22 and msg in err and err.startswith("nconv_depth_sparsify: "), (rc, err)


# ---- Python argument checks ------------------------------------------------------------------------
def test_sparsify_refuses_cpu_tensors_and_bad_arguments(nconv_amd):
    S = nconv_amd.sparsify
    assert nconv_amd.Sparsifier.__module__ == nconv_amd.SparsifyBatch.__module__ == S.__module__
    z = torch.ones(2, 1, 4, 8)
    for n in (None, 3):
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            S(z, n)
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            S(z[0, 0], n)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.Sparsifier((4, 8), B=2, seed=1)(z, 3)
    with pytest.raises(ValueError, match="mutually exclusive"):
        S(z, 3, keep=0.5)
    with pytest.raises(TypeError, match="depth"):
        S(z.double(), 3)
    with pytest.raises(TypeError, match="depth"):
        S(z.numpy(), 3)
    with pytest.raises(ValueError, match="depth"):
        S(torch.ones(2, 3, 4, 8), 3)
    with pytest.raises(ValueError, match="depth"):
        S(torch.ones(2, 1, 4, 16)[..., ::2], 3)
    with pytest.raises(ValueError, match="negative"):
        S(z, -1)
    with pytest.raises(TypeError, match="n"):
        S(z, torch.tensor([1, 2]))  # int64
    with pytest.raises(ValueError, match="n must be"):
        S(z, torch.tensor([1, 2, 3], dtype=torch.int32))
    for keep in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="keep"):
            S(z, keep=keep)
    with pytest.raises(TypeError, match="mask"):
        S(z, 3, mask=torch.ones(4, 8))
    with pytest.raises(ValueError, match="mask"):
        S(z, 3, mask=torch.ones(4, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):
        S(z, 3, mask=torch.ones(3, 1, 4, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="noise_frac"):
        S(z, 3, noise_frac=1.5)
    with pytest.raises(ValueError, match="key_mask"):
        S(z, 3, key_mask=1 << 32)
    with pytest.raises(TypeError, match="state"):
        S(z, 3, state=torch.zeros(3))
    with pytest.raises(ValueError, match="state"):
        S(z, 3, state=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="Sparsifier takes no option"):
        nconv_amd.Sparsifier((4, 8), out={})
    mod = __import__("sys").modules[S.__module__]
    assert mod.noise_threshold(0.1) == SC.noise_threshold(0.1) and mod.noise_threshold(1.0) == 0xFFFFFFFF
    assert mod.state_words((0x89ABCDEF << 32) | 0x80000001, 0xFFFFFFFF) == [-0x7FFFFFFF, 0x89ABCDEF - (1 << 32), -1]


# ---- the loader ------------------------------------------------------------------------------------
def _nyu_tree(tmp_path):
    rng = np.random.default_rng(2)
    for d in ("train/gt", "train/depth", "train/img", "mask"):
        os.makedirs(tmp_path / d)
    gt = rng.random((480, 640)).astype(np.float32) * 10
    np.save(tmp_path / "train/gt/000.npy", gt)
    np.save(tmp_path / "train/depth/000.npy", rng.random((480, 640)).astype(np.float32))
    Image.fromarray(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)).save(tmp_path / "train/img/000.png")
    mask = (rng.random((240, 320)) < 0.1).astype(np.uint8)
    np.save(tmp_path / "mask/m0.npy", mask)
    return gt, np.array(Image.fromarray(mask).resize((640, 480), Image.NEAREST))


def _reference_preprocess(gt, mask, apply_mask, apply_noise):
    """nyuloader.py:79-119 restated (the random mask file is the tree's only one)."""
    raw_depth = torch.FloatTensor(np.expand_dims(gt.copy(), axis=0))
    if apply_noise:
        n = raw_depth.numel()
        nn_ = int(n * 0.1)
        idx = torch.randperm(n)[:nn_]
        noise = torch.FloatTensor(nn_).uniform_(-0.1, 0.1)
        flat = raw_depth.reshape(-1)
        flat[idx] += flat[idx] * noise
        depth = flat.view_as(raw_depth)
    else:
        depth = raw_depth
    if apply_mask:
        return depth * torch.FloatTensor(mask)
    zeros = np.count_nonzero(mask == 0)
    idx = torch.randperm(depth.numel())[:min(zeros, depth.numel())]
    flat = depth.reshape(-1)
    flat[idx] = 0
    return flat.view_as(depth)


def test_nyu_loader_host_mode_is_unchanged(tmp_path, nconv_amd):
    gt, big = _nyu_tree(tmp_path)
    D = nconv_amd.data.DataLoader_NYU
    for use_mask in (True, False):
        for add_noise in (True, False):
            for kw in ({}, {"sparse": "host"}):
                ds = D(str(tmp_path), "train", use_mask, add_noise, height=448, width=608, **kw)
                random.seed(3), torch.manual_seed(7)
                s = ds[0]
                assert set(s) == {"rgb", "depth", "gt", "k"}
                random.seed(3), torch.manual_seed(7)
                want = _reference_preprocess(gt, big, use_mask, add_noise)
                assert s["depth"].shape == (1, 480, 640) and torch.equal(s["depth"], want)
                assert int((s["depth"] == 0).sum()) >= int((big == 0).sum())
    with pytest.raises(ValueError, match="sparse"):
        D(str(tmp_path), "train", True, False, sparse="gpu")


def test_nyu_loader_device_mode_samples(tmp_path, nconv_amd, monkeypatch):
    gt, big = _nyu_tree(tmp_path)
    D = nconv_amd.data.DataLoader_NYU
    H, W = 448, 608
    tp, lp = 480 - H, (640 - W) // 2
    crop = (slice(tp, tp + H), slice(lp, lp + W))

    def no_randperm(*a, **kw):
        raise AssertionError("randperm on the host")
    monkeypatch.setattr(torch, "randperm", no_randperm)
    s = D(str(tmp_path), "train", True, True, height=H, width=W, sparse="device")[0]
    assert set(s) == {"rgb", "depth", "gt", "k", "mask"}
    assert s["mask"].dtype == torch.uint8 and s["mask"].shape == (1, H, W) and s["mask"].is_contiguous()
    assert np.array_equal(s["mask"][0].numpy(), (big[crop] != 0).astype(np.uint8))
    assert s["depth"].shape == (1, H, W) and np.array_equal(s["depth"][0].numpy(), gt[crop])
    assert torch.equal(s["depth"], s["gt"]) and s["depth"].data_ptr() != s["gt"].data_ptr()
    s = D(str(tmp_path), "train", False, False, height=H, width=W, sparse="device")[0]
    assert set(s) == {"rgb", "depth", "gt", "k", "n_keep"}
    assert s["n_keep"].dtype == torch.int32 and s["n_keep"].shape == ()
    assert int(s["n_keep"]) == H * W - int((big[crop] == 0).sum())
    assert np.array_equal(s["depth"][0].numpy(), gt[crop])
    # the default collate stacks them as the batch stage takes them
    from torch.utils.data import DataLoader
    b = next(iter(DataLoader(D(str(tmp_path), "train", False, False, height=H, width=W, sparse="device"), batch_size=1)))
    assert b["n_keep"].dtype == torch.int32 and b["n_keep"].shape == (1,) and b["depth"].shape == (1, 1, H, W)
