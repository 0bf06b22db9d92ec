"""CPU: the backward's workspace layout and kernel choice, pinned.

nconv_bwd_workspace_bytes, the fused head / tail workspace queries and nconv_plan are host-only
(without a device the CU count falls back to 256, so the numbers are deterministic). The byte counts
size the partial rows every weight-gradient kernel writes: a layout that drifts from the launch
code is an out-of-bounds row, not a failed parity test, so the values below are the ones the
library returned before the backward was split into one file per kernel family (generated from
that build, not from the code under test)."""
import ctypes

import pytest


def _src(s, C, H, W):
    s.x = s.c = 0x1000  # never dereferenced: the queries read the geometry only
    s.C, s.H, s.W = C, H, W


def _desc(nconv_amd, B, cin, cout, k, pad, mode, H, W, a, b=None, stride=1):
    L = nconv_amd._lib.NconvLayer()
    L.B, L.Cin, L.H, L.W, L.Cout = B, cin, H, W, cout
    L.KH = L.KW = k
    L.SH = L.SW = stride
    L.DH = L.DW = L.groups = 1
    L.PH = L.PW = pad
    L.Ho = (H + 2 * pad - k) // stride + 1
    L.Wo = (W + 2 * pad - k) // stride + 1
    L.eps, L.thresh = 1e-20, 0.01
    L.load_mode = mode
    _src(L.a, *a)
    if b:
        _src(L.b, *b)
    L.weight = L.bias = L.wsum = 0x1000
    return L


def dnet_layers(nconv_amd, B, H, W):
    """The nine DNET layers (dnet.py) on a B x 1 x H x W input: (name, descriptor)."""
    m = nconv_amd._lib
    h2, w2, h4, w4, h8, w8 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8
    d = lambda *a, **k: _desc(nconv_amd, B, *a, **k)
    return [
        ("nconv1", d(1, 8, 5, 2, m.THRESH, H, W, (1, H, W))),
        ("nconv2", d(8, 8, 5, 2, m.PLAIN, H, W, (8, H, W))),
        ("down1", d(8, 8, 5, 2, m.POOL2, h2, w2, (8, H, W))),
        ("down2", d(8, 8, 5, 2, m.POOL2, h4, w4, (8, h2, w2))),
        ("down3", d(8, 8, 5, 2, m.POOL2, h8, w8, (8, h4, w4))),
        ("nconv4", d(16, 8, 3, 1, m.UPCAT_SKIP_FIRST, h4, w4, (8, h4, w4), (8, h8, w8))),
        ("nconv5", d(16, 8, 3, 1, m.UPCAT_SKIP_FIRST, h2, w2, (8, h2, w2), (8, h4, w4))),
        ("nconv6", d(16, 8, 3, 0, m.UPCAT_UP_FIRST, H, W, (8, H, W), (8, h2, w2))),
        ("nconv7", d(8, 1, 1, 2, m.PLAIN, H - 2, W - 2, (8, H - 2, W - 2))),
    ]


def cases(nconv_amd):
    """(name, descriptor, tail query too, head query too)"""
    out = []
    for B, H, W in ((1, 352, 1216), (2, 37, 71)):
        for name, L in dnet_layers(nconv_amd, B, H, W):
            out.append((f"{name}-B{B}-{H}x{W}", L, name == "nconv6", name == "nconv2"))
    # any stride but 1: the generic kernels
    out.append(("stride2-B2-37x71", _desc(nconv_amd, 2, 8, 8, 5, 2, nconv_amd._lib.PLAIN, 37, 71, (8, 37, 71), stride=2),
                False, False))
    return out


def query(nconv_amd, L, tail, head):
    lib = nconv_amd._lib.lib()
    f, d, w = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.nconv_plan(ctypes.byref(L), ctypes.byref(f), ctypes.byref(d), ctypes.byref(w))
    assert rc == 0, lib.nconv_last_error().decode()
    r = {"ws": lib.nconv_bwd_workspace_bytes(ctypes.byref(L)),
         "dgrad": nconv_amd._lib.KERNEL_NAMES[d.value], "wgrad": nconv_amd._lib.KERNEL_NAMES[w.value]}
    if tail:
        r["tail_ws"] = lib.nconv_bwd_tail_workspace_bytes(ctypes.byref(L))
    if head:
        r["head_ws"] = lib.nconv_bwd_head_workspace_bytes(ctypes.byref(L))
    return r


PINNED = {
    "nconv1-B1-352x1216": {'ws': 1458432, 'dgrad': 'tiled_fp32', 'wgrad': 'tiled_fp32'},
    "nconv2-B1-352x1216": {'ws': 11480064, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32', 'head_ws': 736128},
    "down1-B1-352x1216": {'ws': 11480064, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "down2-B1-352x1216": {'ws': 2947584, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "down3-B1-352x1216": {'ws': 956672, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "nconv4-B1-352x1216": {'ws': 3842560, 'dgrad': 'tiled_fp32_phase', 'wgrad': 'mfma_fp32'},
    "nconv5-B1-352x1216": {'ws': 15145984, 'dgrad': 'tiled_fp32_phase', 'wgrad': 'mfma_fp32'},
    "nconv6-B1-352x1216": {'ws': 35280384, 'dgrad': 'tiled_fp32_phase', 'wgrad': 'mfma_fp32', 'tail_ws': 67520},
    "nconv7-B1-352x1216": {'ws': 71936, 'dgrad': 'tiled_fp32', 'wgrad': 'tiled_fp32'},
    "nconv1-B2-37x71": {'ws': 48384, 'dgrad': 'tiled_fp32', 'wgrad': 'tiled_fp32'},
    "nconv2-B2-37x71": {'ws': 1060096, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32', 'head_ws': 29376},
    "down1-B2-37x71": {'ws': 336128, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "down2-B2-37x71": {'ws': 219904, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "down3-B2-37x71": {'ws': 155136, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "nconv4-B2-37x71": {'ws': 178560, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "nconv5-B2-37x71": {'ws': 323584, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32'},
    "nconv6-B2-37x71": {'ws': 1065088, 'dgrad': 'tiled_fp32', 'wgrad': 'mfma_fp32', 'tail_ws': 6240},
    "nconv7-B2-37x71": {'ws': 2304, 'dgrad': 'tiled_fp32', 'wgrad': 'tiled_fp32'},
    "stride2-B2-37x71": {'ws': 110080, 'dgrad': 'generic', 'wgrad': 'generic'},
}


def test_every_case_is_pinned(nconv_amd):
    assert sorted(PINNED) == sorted(name for name, *_ in cases(nconv_amd))
    assert len(PINNED) == 19


@pytest.mark.parametrize("name", sorted(PINNED))
def test_layout_and_plan_match_the_pinned_values(nconv_amd, name):
    L, tail, head = next(c[1:] for c in cases(nconv_amd) if c[0] == name)
    assert query(nconv_amd, L, tail, head) == PINNED[name]
