"""CPU: what csrc/augment_params.h draws on a C host equals the numpy reference exactly (gains bit for
bit); struct nconv_frame_augment's layout matches the ctypes binding under an unchanged ABI number; every
malformed call fails on the host with -22 and a telling message before any launch; the reference's own
invariants (window in range and reaching both ends, the flip share, copies, hand-applied params, the
rewritten intrinsics keep every pixel's ray); the Python function refuses CPU tensors and malformed
arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import augment_cases as AC
import host_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
F32, U32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "augment_host", csrc=True)


def _f(bits):
    return float(np.array([bits], dtype=U32).view(F32)[0])


# ---- the draw: host code == reference --------------------------------------------------------------
def test_host_draws_equal_the_reference(host_report):
    draws = host_report["draws"]
    assert len(draws) == 3 * 3 * 4 * 6
    flips, offsets = set(), set()
    for row in draws:
        seed, draw, b, H, W, h, w, my, mx, thr, bri, con, col, y0, x0, fl, *gains = row
        p = thr / 4294967296.0  # exact: the thresholds of the table are multiples of 2^-32
        assert AC.flip_threshold(p) == thr
        ry0, rx0, rfl, rg = AC.params_ref(seed, draw, b, H, W, h, w, (my, mx), p, _f(bri), _f(con), _f(col))
        assert (y0, x0, fl) == (ry0, rx0, rfl), row
        assert gains == [int(v) for v in rg.view(U32)], row
        assert 0 <= y0 <= H - h and 0 <= x0 <= W - w
        flips.add(fl), offsets.add((y0, x0))
    assert flips == {0, 1} and len(offsets) > 40


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    L = nconv_amd._lib
    want = {}
    for name, S in (("nconv_frame_augment", L.NconvFrameAugment), ("nconv_augment_plane", L.NconvAugmentPlane)):
        want.update(host_harness.ctypes_layout(S, name))
    c = {k: v for k, v in host_report.items() if k.startswith(("nconv_frame_augment", "nconv_augment_plane"))}
    assert len(c) == 1 + 28 + 1 + 4 and c == want
    assert host_report["modes"] == [L.AUGMENT_CROPS[m] for m in ("random", "center", "min", "max")] == [0, 1, 2, 3]
    assert AC.MODES == L.AUGMENT_CROPS


def test_entry_point_exported_and_abi_unchanged(nconv_amd, host_report):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", src, re.M))
    lib = nconv_amd._lib.lib()
    assert "nconv_frame_augment" in declared and "nconv_frame_augment" in nconv_amd._lib.EXPORTED
    assert ctypes.cast(lib.nconv_frame_augment, ctypes.c_void_p).value
    v = int(re.search(r"#define NCONV_ABI_VERSION (\d+)", src).group(1))
    assert lib.nconv_abi_version() == v == nconv_amd._lib.ABI_VERSION == 27
    assert host_report["abi"] == [27, 27]


BAD_CALLS = {
    "null_descriptor": "null descriptor",
    "null_state": "null state",
    "no_source": "no source",
    "rgb_without_out": "rgb and rgb_out go together",
    "out_without_rgb": "rgb and rgb_out go together",
    "plane_without_out": "plane's src and out go together",
    "out_without_plane": "plane's src and out go together",
    "mask_without_out": "mask and mask_out go together",
    "out_without_mask": "mask and mask_out go together",
    "k_without_k_out": "k and k_out go together",
    "k_out_without_k": "k and k_out go together",
    "B_zero": "non-positive",
    "H_zero": "non-positive",
    "W_negative": "non-positive",
    "h_zero": "non-positive",
    "w_negative": "non-positive",
    "h_above_H": "exceeds the source size",
    "w_above_W": "exceeds the source size",
    "too_large": "below 2^31",
    "rgb_row_stride": "rgb: row stride smaller than W",
    "plane_row_stride": "plane[0]: row stride smaller than W",
    "mask_row_stride": "mask: row stride smaller than W",
    "rgb_channel_overlap": "rgb: channel stride smaller",
    "rgb_image_overlap": "rgb: image stride too small",
    "plane_image_overlap": "plane[1]: image stride smaller",
    "mask_image_overlap": "mask: image stride smaller",
    "mode_y": "unknown mode",
    "mode_x": "unknown mode",
    "flip_threshold": "flip_threshold above 2^32",
    "brightness_negative": "must be in [0, 1]",
    "contrast_above_one": "must be in [0, 1]",
    "color_nan": "must be in [0, 1]",
    "pivot_nan": "pivot is NaN",
    "rgb_max_nan": "rgb_max is NaN or negative",
    "rgb_max_negative": "rgb_max is NaN or negative",
    "state_misaligned": "state not 4-byte aligned",
    "rgb_misaligned": "rgb / rgb_out not 4-byte aligned",
    "rgb_out_misaligned": "rgb / rgb_out not 4-byte aligned",
    "plane_misaligned": "plane's src / out not 4-byte aligned",
    "plane_out_misaligned": "plane's src / out not 4-byte aligned",
    "k_misaligned": "k / k_out not 4-byte aligned",
    "k_out_misaligned": "k / k_out not 4-byte aligned",
    "params_misaligned": "params / gains not 4-byte aligned",
    "gains_misaligned": "params / gains not 4-byte aligned",
    "rgb_out_in_rgb": "output rgb_out overlaps source rgb",
    "plane_out_in_mask": "output plane[0] overlaps source mask",
    "mask_out_on_rgb_end": "output mask_out overlaps source rgb",
    "gt_out_before_depth": "output plane[1] overlaps source plane[0]",
    "params_in_k": "output params overlaps source k",
    "k_out_on_state": "output k_out overlaps source state",
    "gains_in_plane": "output gains overlaps source plane[2]",
}


def test_every_malformed_call_is_refused_on_the_host(host_report):
    """Without a device a call that got past the validation would return -5 (launch error), not -22."""
    calls = {k: v for k, v in host_report.items() if isinstance(v, list) and len(v) == 2 and isinstance(v[1], str)}
    assert set(calls) == set(BAD_CALLS)
    for name, msg in BAD_CALLS.items():
        rc, err = calls[name]
        assert rc == -22 and msg in err and err.startswith("nconv_frame_augment: "), (name, rc, err)


def test_ctypes_call_is_refused_too(nconv_amd):
    L = nconv_amd._lib
    d = L.NconvFrameAugment()
    d.B, d.H, d.W, d.h, d.w = 1, 4, 8, 4, 9
    d.state, d.k, d.k_out = 0x1000, 0x2000, 0x3000
    assert L.lib().nconv_frame_augment(ctypes.byref(d), None) == -22
    assert "exceeds the source size" in L.lib().nconv_last_error().decode()
    assert L.lib().nconv_frame_augment(None, None) == -22


# ---- the reference's invariants --------------------------------------------------------------------
def test_window_stays_in_range_and_reaches_both_ends():
    H, h, W, w = 12, 7, 9, 4  # H - h = W - w = 5
    ys, xs = set(), set()
    for i in range(4096):
        y0, x0, _, _ = AC.params_ref(5, i // 8, i % 8, H, W, h, w)
        ys.add(y0), xs.add(x0)
    assert ys == set(range(6)) and xs == set(range(6))
    for b in range(16):
        y0, x0, _, _ = AC.params_ref(5, 3, b, H, W, H, W)
        assert (y0, x0) == (0, 0)  # h = H, w = W leaves no choice
        assert AC.params_ref(5, 3, b, H, W, h, w, (AC.CENTER, AC.MAX))[:2] == (2, 5)
        assert AC.params_ref(5, 3, b, H, W, h, w, (AC.MIN, AC.CENTER))[:2] == (0, 2)
        assert AC.params_ref(5, 3, b, 11, W, 4, w, (AC.CENTER, AC.MIN))[:2] == (3, 0)


def test_flip_share():
    """4096 (b, draw) pairs at p = 0.5: 2048 +- 160, five binomial standard deviations of 32."""
    n = sum(AC.params_ref(7, i // 16, i % 16, 8, 8, 4, 4, flip=0.5)[2] for i in range(4096))
    print("flipped", n, "of 4096")
    assert abs(n - 2048) <= 160
    for i in range(256):
        assert AC.params_ref(7, i // 16, i % 16, 8, 8, 4, 4, flip=0.0)[2] == 0
        assert AC.params_ref(7, i // 16, i % 16, 8, 8, 4, 4, flip=1.0)[2] == 1
    assert AC.flip_threshold(0.0) == 0 and AC.flip_threshold(1.0) == 1 << 32 and AC.flip_threshold(0.5) == 1 << 31


def test_gains_lie_in_their_band():
    for b in range(64):
        g = AC.params_ref(11, 0, b, 8, 8, 4, 4, brightness=0.2, contrast=0.1, color=0.05)[3]
        assert abs(float(g[0]) - 1) <= 0.2 and abs(float(g[1]) - 1) <= 0.1 and (np.abs(g[2:].astype(np.float64) - 1) <= 0.05).all()
        assert len({float(v) for v in g}) == 5
        assert (AC.params_ref(11, 0, b, 8, 8, 4, 4)[3] == 1).all()
        g = AC.params_ref(11, 0, b, 8, 8, 4, 4, color=0.3)[3]  # one amplitude is enough to switch the jitter on
        assert g[0] == 1 and g[1] == 1 and (g[2:] != 1).all()


def _batch(B, H, W, seed):
    return dict(rgb=AC.image(B, H, W, seed), planes={"depth": AC.plane(B, H, W, seed + 1), "gt": AC.plane(B, H, W, seed + 2)},
                mask=AC.mask_u8(B, H, W, seed + 3), k=AC.intrinsics(B, H, W, seed + 4))


def test_zero_amplitudes_copy_the_rgb_and_params_reproduce_every_output():
    B, H, W, h, w = 5, 9, 20, 6, 13
    src = _batch(B, H, W, 30)
    src["rgb"][0, 0, :2, :9] = AC.SPECIALS  # without jitter even a NaN's payload is copied
    for kw in (dict(), dict(brightness=0.2, contrast=0.2, color=0.2)):
        r = AC.augment_ref((h, w), **src, seed=3, draw=1, **kw)
        assert set(r["params"][:, 2].tolist()) == {0, 1} and (r["params"][:, 3] == 0).all()
        for b in range(B):
            y0, x0, fl, _ = r["params"][b]
            sl = (slice(y0, y0 + h), slice(x0, x0 + w))
            for name, s in (("depth", src["planes"]["depth"]), ("gt", src["planes"]["gt"]), ("mask", src["mask"])):
                want = s[b][sl]
                assert AC.same_bits(r[name][b], want[:, ::-1] if fl else want)
            want = src["rgb"][b][(slice(None), *sl)]
            want = want[..., ::-1] if fl else want
            if not kw:
                assert AC.same_bits(r["rgb"][b], want) and (r["gains"][b] == 1).all()
            else:
                ok = np.isfinite(want)
                assert (r["rgb"][b][ok] != want[ok]).any() and r["rgb"][b][ok].min() >= 0 and r["rgb"][b][ok].max() <= 255


def test_k_out_keeps_every_pixels_ray():
    B, H, W, h, w = 6, 37, 71, 20, 33
    k = AC.intrinsics(B, H, W, 5).astype(F32)
    k[:, 0, 1] = 0  # no skew: the mirror is exact only without it
    r = AC.augment_ref((h, w), k=k, src_size=(H, W), seed=9, draw=2)
    assert set(r["params"][:, 2].tolist()) == {0, 1}
    for b in range(B):
        y0, x0, fl, _ = (int(v) for v in r["params"][b])
        ko = r["k"][b].astype(np.float64)
        ks = k[b].astype(np.float64)
        assert AC.same_bits(np.delete(r["k"][b].reshape(-1), [2, 5]), np.delete(k[b].reshape(-1), [2, 5]))
        for i, j in ((0, 0), (h - 1, w - 1), (7, 11)):
            u = x0 + (w - 1 - j) if fl else x0 + j  # the source pixel the output pixel (i, j) shows
            v = y0 + i
            ray_src = ((u - ks[0, 2]) / ks[0, 0], (v - ks[1, 2]) / ks[1, 1])
            ray_out = ((j - ko[0, 2]) / ko[0, 0], (i - ko[1, 2]) / ko[1, 1])
            sign = -1.0 if fl else 1.0
            assert abs(ray_out[0] - sign * ray_src[0]) < 1e-6 and abs(ray_out[1] - ray_src[1]) < 1e-6


# ---- Python argument checks ------------------------------------------------------------------------
def test_augment_refuses_cpu_tensors_and_bad_arguments(nconv_amd):
    A = nconv_amd.augment
    assert nconv_amd.Augmenter.__module__ == nconv_amd.Augment.__module__ == A.__module__
    rgb, z, m, k = torch.ones(2, 3, 6, 16), torch.ones(2, 1, 6, 16), torch.ones(2, 1, 6, 16, dtype=torch.uint8), torch.ones(2, 3, 3)
    for kw in (dict(rgb=rgb), dict(depth=z), dict(mask=m), dict(k=k, src_size=(6, 16)), dict(rgb=rgb, depth=z, gt=z, mask=m, k=k)):
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            A(size=(4, 8), **kw)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.Augmenter((6, 16), (4, 8), B=2, seed=1)(rgb=rgb, depth=z)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.Augment((4, 8))({"rgb": rgb, "depth": z})
    with pytest.raises(ValueError, match="no source"):
        A(size=(4, 8))
    with pytest.raises(ValueError, match="src_size"):
        A(k=k, size=(4, 8))
    with pytest.raises(TypeError, match="rgb"):
        A(rgb=rgb.double(), size=(4, 8))
    with pytest.raises(TypeError, match="mask"):
        A(depth=z, mask=z, size=(4, 8))
    with pytest.raises(TypeError, match="depth"):
        A(depth=z.numpy(), size=(4, 8))
    with pytest.raises(ValueError, match="rgb"):
        A(rgb=torch.ones(2, 4, 6, 16), size=(4, 8))
    with pytest.raises(ValueError, match="rgb"):
        A(rgb=torch.ones(2, 3, 6, 32)[..., ::2], size=(4, 8))
    with pytest.raises(ValueError, match="gt"):
        A(depth=z, gt=torch.ones(2, 1, 6, 15), size=(4, 8))
    with pytest.raises(ValueError, match="depth"):
        A(rgb=rgb, depth=torch.ones(3, 1, 6, 16), size=(4, 8))
    with pytest.raises(ValueError, match="mask"):
        A(rgb=rgb, mask=torch.ones(3, 1, 6, 16, dtype=torch.uint8), size=(4, 8))
    with pytest.raises(ValueError, match="k "):
        A(rgb=rgb, k=torch.ones(3, 3, 3), size=(4, 8))
    with pytest.raises(ValueError, match="k must be"):
        A(rgb=rgb, k=torch.ones(2, 3, 4), size=(4, 8))
    for size in ((7, 8), (4, 17), (0, 8), (4, -1)):
        with pytest.raises(ValueError, match="size"):
            A(rgb=rgb, size=size)
    with pytest.raises(ValueError, match="size"):
        A(rgb=rgb, size=5)
    for crop in ("top", ("random", "bottom"), ("random",), 3):
        with pytest.raises(ValueError, match="crop"):
            A(rgb=rgb, size=(4, 8), crop=crop)
    for name in ("brightness", "contrast", "color"):
        for v in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match=name):
                A(rgb=rgb, size=(4, 8), **{name: v})
    for p in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="flip"):
            A(rgb=rgb, size=(4, 8), flip=p)
    with pytest.raises(ValueError, match="rgb_max"):
        A(rgb=rgb, size=(4, 8), rgb_max=-1.0)
    with pytest.raises(ValueError, match="pivot"):
        A(rgb=rgb, size=(4, 8), pivot=float("nan"))
    with pytest.raises(TypeError, match="state"):
        A(rgb=rgb, size=(4, 8), state=torch.zeros(3))
    with pytest.raises(ValueError, match="state"):
        A(rgb=rgb, size=(4, 8), state=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="Augmenter takes no option"):
        nconv_amd.Augmenter((6, 16), (4, 8), out={})
    with pytest.raises(ValueError, match="size"):
        nconv_amd.Augmenter((6, 16), (7, 8))
    with pytest.raises(TypeError, match="Augment takes no option"):
        nconv_amd.Augment((4, 8), state=None)
    with pytest.raises(ValueError, match="'mask' form"):
        nconv_amd.Augment((4, 8))({"rgb": rgb, "depth": z, "n_keep": torch.tensor([3, 4], dtype=torch.int32)})
    with pytest.raises(KeyError, match="none of"):
        nconv_amd.Augment((4, 8))({"name": "a"})
    mod = __import__("sys").modules[A.__module__]
    assert mod.flip_threshold(0.3) == AC.flip_threshold(0.3) and mod.flip_threshold(1.0) == 1 << 32
