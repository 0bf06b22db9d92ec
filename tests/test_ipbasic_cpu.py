"""CPU: the numpy reference of the IP-Basic baseline checks itself (an exact constant plane, a single
sample's footprints, the empty image, keep_samples, the special values, the median and the blur against
independent formulations); the entry point is exported, declared and bound with the C struct's layout
under an unchanged ABI number; every malformed call fails on the host with -22 before any launch; the
Python layer refuses CPU tensors and malformed arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import host_harness
import ipbasic_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
F32 = np.float32


# ---- the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("extrapolate", (False, True), ids=("plain", "extrapolate"))
def test_reference_exact_constant(extrapolate):
    """Samples of 36 m every fourth pixel: v = 64 everywhere after the closing, every later stage value
    is a small dyadic (the blur: 4 + 16 = 20, + 24 = 44, + 16 = 60, + 4 = 64), so the result is 36.0f
    exactly at every pixel."""
    z = np.zeros((1, 24, 40), dtype=F32)
    z[:, ::4, ::4] = 36.0
    s = IC.ipbasic_ref(z, max_depth=100.0, extrapolate=extrapolate, stages=True)
    assert (s["v0"][z > 0] == 64.0).all() and (s["v0"][z == 0] == 0.0).all()
    assert (s["v1"][0, 2, 2] == 0.0) and (s["v1"][0, 1, 1] == 64.0)  # the diamond does not reach (2, 2)
    for k in ("v2", "v3", "v4", "v5", "v6"):
        assert (s[k] == 64.0).all(), k
    assert IC.same_bits(s["out"], np.full_like(z, 36.0))


def test_reference_single_sample_footprints():
    z = np.zeros((1, 21, 23), dtype=F32)
    z[0, 10, 11] = 30.0
    yy, xx = np.mgrid[0:21, 0:23]
    dy, dx = np.abs(yy - 10), np.abs(xx - 11)
    for kernel, want in ((("diamond", 5), dy + dx <= 2), (("cross", 7), ((dy == 0) | (dx == 0)) & (dy <= 3) & (dx <= 3)),
                         (("full", 3), (dy <= 1) & (dx <= 1)), (("diamond", 7), dy + dx <= 3)):
        s = IC.ipbasic_ref(z, kernel=kernel, stages=True)
        assert ((s["v1"][0] == 70.0) == want).all() and (s["v1"][0][~want] == 0).all(), kernel
    s = IC.ipbasic_ref(z, stages=True)
    # The closing gives the diamond back: a pixel outside it has a 5 x 5 window around it that misses
    # the diamond, so the erosion cuts it away again. The fill then reaches every empty pixel that has
    # a pixel of the diamond in its 7 x 7 window: Chebyshev distance 3 of the diamond, built here tap by
    # tap. (Only a square first kernel leaves a square: the full 3 x 3 case below.)
    diamond = dy + dx <= 2
    pad = np.pad(diamond, 3)
    reach = np.zeros_like(diamond)
    for a in range(7):
        for b in range(7):
            reach |= pad[a:a + 21, b:b + 23]
    assert ((s["v2"][0] == 70.0) == diamond).all()
    assert ((s["v3"][0] == 70.0) == reach).all() and (s["v3"][0][~reach] == 0).all()
    # without median and blur the picture of v3 comes back as depth 30 exactly
    out = IC.ipbasic_ref(z, median=False, blur=None)
    assert ((out[0] == 30.0) == reach).all() and (out[0][~reach] == 0).all()
    # the full 3 x 3 kernel: the 3 x 3 square after stage 1, and the closing keeps a square a square
    s = IC.ipbasic_ref(z, kernel=("full", 3), stages=True)
    assert ((s["v2"][0] == 70.0) == ((dy <= 1) & (dx <= 1))).all()
    assert ((s["v3"][0] == 70.0) == ((dy <= 4) & (dx <= 4))).all()


def test_reference_empty_image_and_specials():
    for shape in ((1, 1, 1), (2, 5, 7), (1, 40, 75)):
        z = np.zeros(shape, dtype=F32)
        for o in IC.OPTION_SETS:
            assert IC.same_bits(IC.ipbasic_ref(z, **o), z), o
    # every special value alone is no sample, and among real samples the output stays finite
    sp = IC.specials()
    for v in sp:
        z = np.full((1, 9, 11), v, dtype=F32)
        for o in IC.OPTION_SETS:
            assert (IC.ipbasic_ref(z, **o).view(np.uint32) == 0).all(), (v, o)
    z = IC.plane(2, 40, 75, seed=3, density=0.3)
    assert np.isnan(z).any() and np.isinf(z).any()
    for o in IC.OPTION_SETS:
        out = IC.ipbasic_ref(z, **o)
        assert np.isfinite(out).all() and (out >= 0).all() and not np.signbit(out).any(), o
        assert (out <= F32(o["max_depth"])).all()


def test_reference_keep_samples_and_their_loss_without_it():
    z = IC.plane(2, 40, 75, seed=5, density=0.2)
    smp = IC.sample_of(z, 100.0)
    assert 100 < smp.sum() < z.size
    for extrapolate in (False, True):
        kept = IC.ipbasic_ref(z, keep_samples=True, extrapolate=extrapolate)
        plain = IC.ipbasic_ref(z, extrapolate=extrapolate)
        assert (kept.view(np.uint32)[smp] == z.view(np.uint32)[smp]).all()
        assert (kept.view(np.uint32)[~smp] == plain.view(np.uint32)[~smp]).all()
        assert (plain[smp] != z[smp]).mean() > 0.5  # IP-Basic moves its samples


def test_reference_median_and_blur_against_other_formulations():
    rng = np.random.default_rng(0)
    for shape in ((1, 1, 1), (1, 2, 1), (2, 1, 2), (1, 2, 3), (2, 5, 7), (1, 9, 12)):
        v = rng.uniform(0, 100, shape).astype(F32)
        v[rng.random(shape) < 0.3] = 0
        B, H, W = shape
        med = IC.median5(v)
        blur = IC.gauss5(v)
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    win = [v[b, min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]
                           for dy in range(-2, 3) for dx in range(-2, 3)]
                    assert med[b, y, x] == sorted(win)[12]
            # the blur with numpy's own reflect padding where that is defined (pad < size)
            if H > 2 and W > 2:
                p = np.pad(v[b], 2, mode="reflect")
                h = sum(IC.W5[k].astype(np.float64) * p[:, k:k + W] for k in range(5))
                full = sum(IC.W5[k].astype(np.float64) * h[k:k + H] for k in range(5))
                assert np.abs(blur[b] - full[:H]).max() <= 1e-4
    assert [IC.reflect101(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 3, 2]
    assert [IC.reflect101(i, 2) for i in (-2, -1, 2, 3)] == [0, 1, 0, 1] and IC.reflect101(-2, 1) == 0


def test_reference_blur_rounds_every_product():
    """0.375 a is not exact in float32 (3 a needs two more bits than a), so the blur's products are rounded
    before they are added, as include/nconv.h states: a fused multiply-add gives other bits."""
    a = np.array([[[0.0, 0.0, 64.0 * (1.0 + 2.0 ** -23), 0.0, 0.0]]], dtype=F32)  # 3 a ends in 1.5 ulp
    exact = 0.375 * float(a[0, 0, 2])
    assert float(F32(0.375) * a[0, 0, 2]) != exact
    assert IC._gauss_axis(a, 2)[0, 0, 2] == F32(0.375) * a[0, 0, 2]
    v = np.random.default_rng(1).uniform(1, 99, (1, 9, 12)).astype(F32)
    h64 = sum(float(IC.W5[k]) * np.pad(v[0], 2, mode="reflect")[2:-2, k:k + 12].astype(np.float64) for k in range(5))
    assert (IC._gauss_axis(v, 2)[0] != h64.astype(F32)).any()  # one rounding at the end is another rule


def test_reference_extrapolation():
    v = np.zeros((1, 6, 4), dtype=F32)
    v[0, 3, 0], v[0, 4, 0] = 7.0, 9.0   # top 3
    v[0, 5, 1] = 5.0                    # only the last row
    v[0, 0, 3], v[0, 2, 3] = 2.0, 4.0   # top 0; column 2 has none
    e, top = IC.extrapolate(v)
    assert top.tolist() == [[3, 5, 0, 0]]
    assert e[0, :, 0].tolist() == [7, 7, 7, 7, 9, 0] and e[0, :, 1].tolist() == [5] * 6
    assert e[0, :, 2].tolist() == [0] * 6 and e[0, :, 3].tolist() == [2, 0, 4, 0, 0, 0]


def test_generated_planes_are_as_the_tests_need_them():
    z = IC.plane(2, 71, 139, seed=1, density=0.6)
    assert (z[:, :20] == 0).sum() > 0.98 * z[:, :20].size
    cols = (IC.sample_of(z, 100.0).sum(axis=1) == 0)
    assert cols.sum(axis=1).min() >= 40
    assert sum(np.isnan(z).ravel()) and (z == IC.T).any() and (z == F32(100.0)).any()
    s = IC.ipbasic_ref(z, kernel=("full", 3), extrapolate=True, stages=True)
    assert (s["v4"] == 0).any() and (s["v3e"] != s["v3"]).any() and (s["v4"] != s["v3e"]).any()


# ---- symbols, layout, host calls -------------------------------------------------------------------
def test_entry_point_exported_and_declared(nconv_amd):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", src, re.M))
    assert "nconv_depth_ipbasic" in declared and "nconv_depth_ipbasic" in nconv_amd._lib.EXPORTED
    lib = nconv_amd._lib.lib()
    assert lib.nconv_depth_ipbasic.restype is ctypes.c_int and len(lib.nconv_depth_ipbasic.argtypes) == 7
    assert lib.nconv_abi_version() == 27 == nconv_amd._lib.ABI_VERSION
    assert int(re.search(r"#define\s+NCONV_ABI_VERSION\s+(\d+)", src).group(1)) == 27
    # the header states the rule
    for text in ("v0 = max_depth - d_p", "erode(dilate(v1, full 5), full 5)", "empty(v2) ? dilate(v2, full 7) : v2",
                 "the 13th smallest of the 25 values", "(((w0*a0 + w1*a1) + w2*a2) + w3*a3) + w4*a4",
                 "no contraction", "reflect-101", "does not\n *               preserve"):
        assert text in src, text


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "ipbasic_host")


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    S = nconv_amd._lib.NconvDepthIpbasic
    want = host_harness.ctypes_layout(S, "nconv_depth_ipbasic")
    c = {k: v for k, v in host_report.items() if k.startswith("nconv_depth_ipbasic")}
    assert len(c) == 14 and c == want
    assert host_report["desc_typedef"] == ctypes.sizeof(S)
    L = nconv_amd._lib
    assert host_report["enums"] == [L.IPBASIC_KERNELS["full"], L.IPBASIC_KERNELS["cross"], L.IPBASIC_KERNELS["diamond"],
                                    L.IPBASIC_BLURS[None], L.IPBASIC_BLURS["gaussian"]]
    assert L.IPBASIC_BLURS["none"] == L.IPBASIC_BLURS[None]


HOST_REJECTS = {
    "null_descriptor": "null descriptor", "null_src": "null src or dst", "null_dst": "null src or dst",
    "B_zero": "non-positive", "H_zero": "non-positive", "W_negative": "non-positive",
    "too_many_pixels": "below 2^31", "shape_negative": "kernel_shape", "shape_3": "kernel_shape",
    "size_4": "kernel_size", "size_9": "kernel_size", "size_1": "kernel_size", "blur_2": "unknown blur",
    "blur_negative": "unknown blur", "max_depth_nan": "max_depth", "max_depth_inf": "max_depth",
    "max_depth_2T": "max_depth", "max_depth_negative": "max_depth",
    "src_misaligned": "4-byte aligned", "dst_misaligned": "4-byte aligned", "work_misaligned": "4-byte aligned",
    "top_misaligned": "4-byte aligned",
    "src_row_stride_short": "src: row stride smaller than W", "src_image_stride_short": "src: image stride smaller",
    "dst_row_stride_short": "dst: row stride smaller than W", "dst_image_stride_short": "dst: image stride smaller",
    "src_image_2_31_bytes": "src: plane too large", "dst_image_2_31_bytes": "dst: plane too large",
    "overlap_inside": "overlaps src", "overlap_tail": "overlaps src", "overlap_same": "overlaps src",
    "work_missing": "extrapolate without", "top_missing": "extrapolate without",
    "work_is_src": "workspace overlaps", "top_in_dst": "workspace overlaps", "top_in_work": "workspace overlaps",
}


def test_host_calls(host_report):
    assert host_report["abi"] == [27, 27]
    got = {k[3:]: v for k, v in host_report.items() if k.startswith("rc_")}
    assert set(got) == set(HOST_REJECTS)
    for name, msg in HOST_REJECTS.items():
        rc, err = got[name]
        assert rc == -22 and err.startswith("nconv_depth_ipbasic") and msg in err, (name, rc, err)


# ---- the Python layer ------------------------------------------------------------------------------
def test_python_refuses_cpu_tensors_and_bad_arguments(nconv_amd):
    M = nconv_amd.ipbasic
    assert nconv_amd.ipbasic_fill is M.ipbasic_fill and nconv_amd.IPBasicFiller is M.IPBasicFiller
    assert nconv_amd.IPBasic is M.IPBasic and nconv_amd.IPBasicFill is M.IPBasicFill
    z = torch.ones(2, 1, 6, 8)
    with pytest.raises(RuntimeError, match="ipbasic: S is on cpu; .*no PyTorch fallback"):
        nconv_amd.ipbasic_fill(z)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        nconv_amd.IPBasicFiller((6, 8), B=2, extrapolate=True)(z)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        nconv_amd.IPBasic(extrapolate=True)(z)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        nconv_amd.IPBasicFill()({"depth": z})
    for bad, exc, text in ((dict(kernel="diamond"), TypeError, "kernel must be \\(shape, size\\)"),
                           (dict(kernel=(5, "diamond")), TypeError, "kernel must be \\(shape, size\\)"),
                           (dict(kernel=("diamond", 5.0)), TypeError, "kernel must be \\(shape, size\\)"),
                           (dict(kernel=("star", 5)), ValueError, "kernel shape 'star' is not one of"),
                           (dict(kernel=("full", 4)), ValueError, "kernel size 4 is not 3, 5 or 7"),
                           (dict(kernel=("full", 9)), ValueError, "kernel size 9 is not 3, 5 or 7"),
                           (dict(blur="bilateral"), ValueError, "blur 'bilateral' is not offered"),
                           (dict(blur="box"), ValueError, "blur 'box' is not"),
                           (dict(blur=5), TypeError, "blur must be"),
                           (dict(max_depth=float("nan")), ValueError, "max_depth"),
                           (dict(max_depth=float("inf")), ValueError, "max_depth"),
                           (dict(max_depth=0.2), ValueError, "max_depth = 0.2 must be finite and above 0.2")):
        with pytest.raises(exc, match="ipbasic: " + text):
            nconv_amd.ipbasic_fill(z, **bad)
    with pytest.raises(TypeError, match="ipbasic: S: expected torch.float32"):
        nconv_amd.ipbasic_fill(z.double())
    with pytest.raises(TypeError, match="ipbasic: S must be a tensor"):
        nconv_amd.ipbasic_fill(z.numpy())
    with pytest.raises(ValueError, match="ipbasic: S of shape"):
        nconv_amd.ipbasic_fill(torch.ones(2, 3, 6, 8))
    with pytest.raises(ValueError, match="ipbasic: S of shape"):
        nconv_amd.ipbasic_fill(torch.ones(8, 6).t())
    for cls in (nconv_amd.IPBasicFiller, nconv_amd.IPBasic, nconv_amd.IPBasicFill):
        args = ((6, 8),) if cls is nconv_amd.IPBasicFiller else ()
        with pytest.raises(TypeError, match="takes no option 'out'"):
            cls(*args, out={})
        with pytest.raises(TypeError, match="takes no option 'window'"):
            cls(*args, window=3)
    m = nconv_amd.IPBasic(extrapolate=True, kernel=("full", 3))
    assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and "extrapolate=True" in repr(m)
    assert m.eval() is m and m.to("cpu") is m
    st = nconv_amd.IPBasicFill(key="depth", out_key="filled")
    assert (st.key, st.out_key) == ("depth", "filled") and nconv_amd.IPBasicFill().out_key == "depth"
