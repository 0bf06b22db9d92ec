"""CPU: the dense convolutions' host-side layout, pinned.

nconv_dense_packed_floats and nconv_dense_wgrad_workspace_bytes are host-only (the weight-gradient
plan sizes its split-K by a fixed 512 workgroups, not by the device). The counts size the buffers
the packing and weight-gradient kernels write: a plan that drifts from the launch code is an
out-of-bounds write, not a failed parity test, so the values below are the ones the library
returned before dense_conv.hip was split into one file per kernel family (generated from that
build, not from the code under test)."""
import ctypes

import pytest

from dense_cases import CASES, case_id

KINDS = {"3x3": 0, "1x1": 1, "tr4x4": 2, "4x4s2": 3}
# the 32- and 64-wide tiles, the tie rule of dense_cout_tile, ragged chunks
PACK_CHANNELS = ((1, 32), (3, 32), (32, 64), (33, 64), (64, 64), (128, 64), (65, 64), (32, 1), (40, 96))
# tests/test_gpu_dense_train.py::test_transposed_wgrad_row_split
ROW_SPLIT = ((1, 32, 32, 9, 19), (1, 64, 64, 7, 20), (32, 1, 32, 12, 33), (64, 1, 64, 5, 17), (2, 32, 32, 20, 41),
             (1, 32, 32, 44, 152))
# layers of the guided model on a 352 x 1216 frame: (kind, stride, C0, C1, Cout, H, W)
GUIDED = {"rgb_encoder0": (0, 1, 3, 0, 32, 352, 1216), "rgb_encoder1-s2": (0, 2, 32, 0, 64, 352, 1216),
          "fuse_conv1": (0, 1, 32, 32, 32, 352, 1216), "upcat-trans": (2, 2, 1, 64, 64, 176, 608)}


def _wgrad(nconv_amd, B, kind, stride, c0, c1, cout, H, W, math):
    d = nconv_amd._lib.NconvDenseWgrad()
    d.B, d.kind, d.stride = B, kind, stride
    d.x0 = d.gy = d.gw = 0x1000  # never dereferenced: the query reads the geometry only
    d.C0, d.C1 = c0, c1
    d.x1 = 0x1000 if c1 else None
    d.H, d.W, d.Cout = H, W, cout
    if kind == 2:
        d.Ho, d.Wo = 2 * H, 2 * W
    else:
        k = 3 if kind == 0 else 1
        d.Ho, d.Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    d.math = nconv_amd._lib.DENSE_MATHS[math]
    return d


def wgrad_cases(nconv_amd):
    """(name, descriptor, NCONV_WGD_TR_ROWS or None)"""
    out = []
    for case in CASES:
        for math in ("fp32", "bf16x9"):
            out.append((f"{case_id(case)}-{math}", _wgrad(nconv_amd, 2, *case[:7], math), None))
    for c0, c1, cout, H, W in ROW_SPLIT:
        for env in (None, "0"):
            out.append((f"rowsplit-{c0}+{c1}to{cout}_{H}x{W}-env{env}",
                        _wgrad(nconv_amd, 2, 2, 2, c0, c1, cout, H, W, "bf16x9"), env))
    for name, layer in GUIDED.items():  # (split-K not capped by the tile count: the bf16x9 plan differs)
        for math in ("fp32", "bf16x9"):
            out.append((f"guided-{name}-{math}", _wgrad(nconv_amd, 1, *layer, math), None))
    return out


PACKED = {
    "3x3-1to32": 6144,
    "3x3-3to32": 6144,
    "3x3-32to64": 49152,
    "3x3-33to64": 61440,
    "3x3-64to64": 98304,
    "3x3-128to64": 196608,
    "3x3-65to64": 110592,
    "3x3-32to1": 24576,
    "3x3-40to96": 92160,
    "1x1-1to32": 1024,
    "1x1-3to32": 1024,
    "1x1-32to64": 8192,
    "1x1-33to64": 10240,
    "1x1-64to64": 16384,
    "1x1-128to64": 32768,
    "1x1-65to64": 18432,
    "1x1-32to1": 4096,
    "1x1-40to96": 15360,
    "tr4x4-1to32": 10240,
    "tr4x4-3to32": 10240,
    "tr4x4-32to64": 81920,
    "tr4x4-33to64": 102400,
    "tr4x4-64to64": 163840,
    "tr4x4-128to64": 327680,
    "tr4x4-65to64": 184320,
    "tr4x4-32to1": 40960,
    "tr4x4-40to96": 153600,
    "4x4s2-1to32": 10240,
    "4x4s2-3to32": 10240,
    "4x4s2-32to64": 81920,
    "4x4s2-33to64": 102400,
    "4x4s2-64to64": 163840,
    "4x4s2-128to64": 327680,
    "4x4s2-65to64": 184320,
    "4x4s2-32to1": 40960,
    "4x4s2-40to96": 153600,
}

WGRAD_WS = {
    "k0s1_32+32to32_19x45_relu_bias-fp32": 1474560,
    "k0s1_32+32to32_19x45_relu_bias-bf16x9": 1474560,
    "k0s1_64+64to64_12x40-fp32": 3538944,
    "k0s1_64+64to64_12x40-bf16x9": 3538944,
    "k0s1_1+0to32_13x33_relu_bias-fp32": 18432,
    "k0s1_1+0to32_13x33_relu_bias-bf16x9": 18432,
    "k0s1_64+0to64_9x70_relu_bias-fp32": 2654208,
    "k0s1_64+0to64_9x70_relu_bias-bf16x9": 2654208,
    "k0s2_32+0to64_17x43_bias-fp32": 737280,
    "k0s2_32+0to64_17x43_bias-bf16x9": 737280,
    "k0s2_64+0to64_16x40_bias-fp32": 1179648,
    "k0s2_64+0to64_16x40_bias-bf16x9": 1179648,
    "k0s1_3+0to32_16x40_bias-fp32": 55296,
    "k0s1_3+0to32_16x40_bias-bf16x9": 55296,
    "k1s1_3+0to32_11x35-fp32": 4608,
    "k1s1_3+0to32_11x35-bf16x9": 4608,
    "k1s2_64+0to64_15x41-fp32": 65536,
    "k1s2_64+0to64_15x41-bf16x9": 65536,
    "k2s2_1+64to64_7x20-fp32": 2113536,
    "k2s2_1+64to64_7x20-bf16x9": 2113536,
    "k2s2_1+32to32_9x19_bias-fp32": 671744,
    "k2s2_1+32to32_9x19_bias-bf16x9": 671744,
    "k0s1_32+0to1_14x37-fp32": 18432,
    "k0s1_32+0to1_14x37-bf16x9": 18432,
    "k0s1_1+32to32_11x37_relu_bias-fp32": 456192,
    "k0s1_1+32to32_11x37_relu_bias-bf16x9": 456192,
    "k0s2_33+0to64_13x29_bias-fp32": 608256,
    "k0s2_33+0to64_13x29_bias-bf16x9": 608256,
    "rowsplit-1+32to32_9x19-envNone": 671744,
    "rowsplit-1+32to32_9x19-env0": 675840,
    "rowsplit-1+64to64_7x20-envNone": 2113536,
    "rowsplit-1+64to64_7x20-env0": 2129920,
    "rowsplit-32+1to32_12x33-envNone": 1589248,
    "rowsplit-32+1to32_12x33-env0": 1622016,
    "rowsplit-64+1to64_5x17-envNone": 1589248,
    "rowsplit-64+1to64_5x17-env0": 1597440,
    "rowsplit-2+32to32_20x41-envNone": 2670592,
    "rowsplit-2+32to32_20x41-env0": 2785280,
    "rowsplit-1+32to32_44x152-envNone": 14516224,
    "rowsplit-1+32to32_44x152-env0": 14868480,
    "guided-rgb_encoder0-fp32": 1769472,
    "guided-rgb_encoder0-bf16x9": 1769472,
    "guided-rgb_encoder1-s2-fp32": 37748736,
    "guided-rgb_encoder1-s2-bf16x9": 18874368,
    "guided-fuse_conv1-fp32": 18874368,
    "guided-fuse_conv1-bf16x9": 18874368,
    "guided-upcat-trans-fp32": 34455552,
    "guided-upcat-trans-bf16x9": 34455552,
}


def test_every_case_is_pinned(nconv_amd):
    assert sorted(PACKED) == sorted(f"{k}-{ci}to{co}" for k in KINDS for ci, co in PACK_CHANNELS)
    assert sorted(WGRAD_WS) == sorted(name for name, *_ in wgrad_cases(nconv_amd))
    assert (len(PACKED), len(WGRAD_WS)) == (36, 2 * len(CASES) + 2 * len(ROW_SPLIT) + 2 * len(GUIDED))


@pytest.mark.parametrize("name", sorted(PACKED))
def test_packed_floats_match_the_pinned_values(nconv_amd, name):
    kind, chans = name.split("-")
    ci, co = map(int, chans.split("to"))
    assert nconv_amd._lib.lib().nconv_dense_packed_floats(KINDS[kind], ci, co) == PACKED[name]


@pytest.mark.parametrize("name", sorted(WGRAD_WS))
def test_wgrad_workspace_bytes_match_the_pinned_values(nconv_amd, name, monkeypatch):
    d, env = next(c[1:] for c in wgrad_cases(nconv_amd) if c[0] == name)
    if env is None:
        monkeypatch.delenv("NCONV_WGD_TR_ROWS", raising=False)
    else:
        monkeypatch.setenv("NCONV_WGD_TR_ROWS", env)
    assert nconv_amd._lib.lib().nconv_dense_wgrad_workspace_bytes(ctypes.byref(d)) == WGRAD_WS[name]
