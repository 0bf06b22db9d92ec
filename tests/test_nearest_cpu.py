"""CPU: the brute-force numpy reference of the nearest-sample transform checks itself (hand-written 3 x 3 and
5 x 5 answers with ties, the closed form of a single sample, scipy's Euclidean distance transform where
scipy is importable, the forced ties); the entry point is exported, declared and bound with the C struct's
layout under an unchanged ABI number; every malformed call fails on the host with -22 before any launch; the
Python layer refuses CPU tensors and malformed arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import host_harness
import nearest_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
F32 = np.float32
INF, NO = np.inf, NC.NO_DIST2


# ---- the reference ---------------------------------------------------------------------------------
def test_reference_by_hand_3x3():
    z = np.array([[[0, 0, 5], [0, 0, 0], [7, 0, 0]]], dtype=F32)  # samples: pixel 2 (0, 2) and pixel 6 (2, 0)
    r = NC.nearest_ref(z)
    # (0, 0), (1, 1) and (2, 2) are equally far from both: the smaller pixel number, 2, wins
    assert r["index"].tolist() == [[[2, 2, 2], [6, 2, 2], [6, 6, 2]]]
    assert r["dist2"].tolist() == [[[4, 1, 0], [1, 2, 1], [0, 1, 4]]]
    assert r["dst"].tolist() == [[[5, 5, 5], [7, 5, 5], [7, 7, 5]]]
    assert NC.same_bits(r["dist"], np.sqrt(np.array(r["dist2"], dtype=F32)))
    assert r["dist"][0, 1, 1] == F32(np.sqrt(F32(2)))
    lim = NC.nearest_ref(z, max_distance=1.5)  # max_dist2 = floor(2.25) = 2
    assert lim["index"].tolist() == [[[-1, 2, 2], [6, 2, 2], [6, 6, -1]]]
    assert lim["dist2"].tolist() == [[[NO, 1, 0], [1, 2, 1], [0, 1, NO]]]
    assert lim["dst"].tolist() == [[[0, 5, 5], [7, 5, 5], [7, 7, 0]]] and not np.signbit(lim["dst"]).any()
    assert lim["dist"][0, 0, 0] == INF and lim["dist"][0, 2, 2] == INF
    zero = NC.nearest_ref(z, max_distance=0)
    assert zero["index"].tolist() == [[[-1, -1, 2], [-1, -1, -1], [6, -1, -1]]] and NC.same_bits(zero["dst"], z)


def test_reference_by_hand_5x5():
    z = np.zeros((1, 5, 5), dtype=F32)
    z[0, 0, 4], z[0, 2, 1], z[0, 4, 3] = 1.5, 2.5, 3.5  # pixels 4, 11 and 23
    r = NC.nearest_ref(z)
    assert r["index"].tolist() == [[[11, 11, 4, 4, 4],      # (0, 2): 4 and 11 at d2 = 4 and 5
                                    [11, 11, 11, 4, 4],     # (1, 3): 4 at 2, 11 at 5
                                    [11, 11, 11, 11, 4],    # (2, 3): 4, 11 and 23 all at d2 = 4 and 5: 11 at 4
                                    [11, 11, 11, 23, 23],   # (3, 2): 11 and 23 at d2 = 2: the smaller number
                                    [11, 11, 23, 23, 23]]]  # (4, 1): 11 at 4, 23 at 4: the smaller number
    assert r["dist2"].tolist() == [[[5, 4, 4, 1, 0], [2, 1, 2, 2, 1], [1, 0, 1, 4, 4], [2, 1, 2, 1, 2], [5, 4, 1, 0, 1]]]
    # floor 2.5: the sample 2.5 is not above it; floor None: the zeros are samples, everything is its own
    r = NC.nearest_ref(z, floor=2.5)
    assert (r["index"] == 23).all() and r["dist2"][0, 0, 0] == 25 and r["dist"][0, 0, 0] == 5.0
    r = NC.nearest_ref(z, floor=None)
    assert (r["index"].reshape(-1) == np.arange(25)).all() and (r["dist2"] == 0).all() and NC.same_bits(r["dst"], z)


def test_reference_specials_empty_and_single():
    for v in NC.specials():
        z = np.full((2, 4, 6), v, dtype=F32)
        floors = (0.0, 2.5) if np.isfinite(v) else NC.FLOORS
        for floor in floors:
            r = NC.nearest_ref(z, floor=floor)
            if NC.sample_of(z, floor).any():
                assert 0 < v <= F32(2.5) and floor == 0.0  # the positive ones: samples above 0, none above 2.5
                continue
            assert (r["index"] == -1).all() and (r["dist2"] == NO).all() and (r["dist"] == INF).all()
            assert (r["dst"].view(np.uint32) == 0).all()
    for shape, at in (((2, 7, 9), (6, 0)), ((1, 1, 1), (0, 0)), ((1, 9, 1), (3, 0)), ((1, 33, 70), (0, 69))):
        for md in (None, 0, 1.5, 5):
            z, want = NC.single_ref(shape, at, 41.5, NC.max_dist2_of(md))
            got = NC.nearest_ref(z, max_distance=md)
            for k in want:
                assert NC.same_bits(got[k].view(np.uint32), want[k].view(np.uint32)), (shape, md, k)
    assert [NC.max_dist2_of(m) for m in (None, 0, 1.5, 5, 1e30, np.inf)] == [-1, 0, 2, 25, NO, NO]


def test_reference_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for seed, density in ((1, 0.02), (2, 0.4)):
        z = NC.plane(1, 33, 70, seed=seed, density=density)
        for floor in (0.0, 2.5):
            valid = NC.sample_of(z, floor)[0]
            d = ndimage.distance_transform_edt(~valid, return_distances=True)
            got = NC.nearest_ref(z, floor=floor)["dist2"][0]
            assert (got == np.rint(d * d).astype(np.int64)).all()


def test_reference_forced_ties_and_generated_planes():
    cases = NC.forced_planes()
    assert len(cases) > 150
    z = np.concatenate([c[1] for c in cases])
    r = NC.nearest_ref(z)
    for n, (name, _, centre, want) in enumerate(cases):
        assert r["index"][n, centre[0], centre[1]] == want, name
    B, H, W = 3, 33, 70
    z = NC.plane(B, H, W, seed=4, density=0.4)
    assert np.isnan(z[0]).any() and np.isinf(z[0]).any() and np.signbit(z[0][z[0] == 0]).any() and (z[0] < 0).any()
    for floor in (0.0, 2.5):
        v = NC.sample_of(z, floor)
        assert v[0].sum() > 100 and v[1].sum() == 0 and v[2].sum() == 1 and v[2, H - 1, 0]
    assert NC.sample_of(z, 0.0)[0].sum() > NC.sample_of(z, 2.5)[0].sum()
    zn = NC.plane(B, H, W, seed=4, density=0.4, background=np.nan)
    v = NC.sample_of(zn, None)
    assert v[1].sum() == 0 and v[2].sum() == 1 and (zn[0][v[0]] < 0).any() and 100 < v[0].sum() < H * W
    r = NC.nearest_ref(zn, floor=None)
    assert (r["dst"] < 0).any()  # with floor=None negatives are samples


# ---- symbols, layout, host calls -------------------------------------------------------------------
def test_entry_point_exported_and_declared(nconv_amd):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", src, re.M))
    assert "nconv_depth_nearest" in declared and "nconv_depth_nearest" in nconv_amd._lib.EXPORTED
    lib = nconv_amd._lib.lib()
    assert lib.nconv_depth_nearest.restype is ctypes.c_int and len(lib.nconv_depth_nearest.argtypes) == 9
    assert lib.nconv_abi_version() == 27 == nconv_amd._lib.ABI_VERSION
    assert int(re.search(r"#define\s+NCONV_ABI_VERSION\s+(\d+)", src).group(1)) == 27
    # the header states the rule
    for text in ("iff its value is finite and > floor", "(r - r')^2 + (c - c')^2", "ties to the smallest pixel\n *               number",
                 "0x7FFFFFFF", "correctly rounded sqrtf((float)d2)", "H^2 + W^2 >= 2^31", "max_dist2 < 0: no limit"):
        assert text in src, text


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "nearest_host")


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    S = nconv_amd._lib.NconvDepthNearest
    want = host_harness.ctypes_layout(S, "nconv_depth_nearest")
    c = {k: v for k, v in host_report.items() if k.startswith("nconv_depth_nearest")}
    assert len(c) == 9 and c == want
    assert host_report["desc_typedef"] == ctypes.sizeof(S)


HOST_REJECTS = {
    "null_descriptor": "null descriptor", "null_src": "null src or work", "null_work": "null src or work",
    "no_output": "no output at all", "B_zero": "non-positive", "H_zero": "non-positive", "W_negative": "non-positive",
    "too_many_pixels": "B * H * W must be below 2^31", "diagonal_too_long_W": "H^2 + W^2 must be below 2^31",
    "diagonal_too_long_HW": "H^2 + W^2 must be below 2^31", "floor_nan": "floor is NaN",
    "src_misaligned": "4-byte aligned", "dst_misaligned": "4-byte aligned", "index_misaligned": "4-byte aligned",
    "dist2_misaligned": "4-byte aligned", "dist_misaligned": "4-byte aligned", "work_misaligned": "4-byte aligned",
    "src_row_stride_short": "src: row stride smaller than W", "src_image_stride_short": "src: image stride smaller",
    "dst_row_stride_short": "dst: row stride smaller than W", "dst_image_stride_short": "dst: image stride smaller",
    "src_image_2_31_bytes": "src: plane too large", "dst_image_2_31_bytes": "dst: plane too large",
    "dst_overlap_inside": "dst overlaps src", "dst_overlap_tail": "dst overlaps src", "dst_overlap_same": "dst overlaps src",
    "work_is_src": "work overlaps src", "work_in_dst": "dst overlaps work", "index_in_src": "index overlaps src",
    "index_in_work": "index overlaps work", "dist2_in_work": "dist2 overlaps work", "dist2_is_index": "dist2 overlaps index",
    "dist_in_dst": "dist overlaps dst", "dist_in_dist2": "dist overlaps dist2", "dist_in_src": "dist overlaps src",
}


def test_host_calls(host_report):
    assert host_report["abi"] == [27, 27]
    got = {k[3:]: v for k, v in host_report.items() if k.startswith("rc_")}
    assert set(got) == set(HOST_REJECTS)
    for name, msg in HOST_REJECTS.items():
        rc, err = got[name]
        assert rc == -22 and err.startswith("nconv_depth_nearest") and msg in err, (name, rc, err)


# ---- the Python layer ------------------------------------------------------------------------------
def test_python_refuses_cpu_tensors_and_bad_arguments(nconv_amd):
    M = nconv_amd.nearest
    assert nconv_amd.nearest_sample is M.nearest_sample and nconv_amd.NearestFiller is M.NearestFiller
    assert nconv_amd.NearestFill is M.NearestFill and nconv_amd.NearestSample is M.NearestSample
    for name in ("nearest_sample", "NearestFiller", "NearestFill", "NearestSample"):
        assert name in nconv_amd.__all__
    z = torch.ones(2, 1, 6, 8)
    with pytest.raises(RuntimeError, match="nearest: S is on cpu; .*no PyTorch fallback"):
        nconv_amd.nearest_sample(z)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        nconv_amd.NearestFiller((6, 8), B=2, return_dist=True)(z)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        nconv_amd.NearestFill(max_distance=3)(z)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        nconv_amd.NearestSample(dist_key="dist")({"depth": z})
    for bad in (-1, -0.5, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="nearest: max_distance = .* must be >= 0"):
            nconv_amd.nearest_sample(z, max_distance=bad)
    with pytest.raises(ValueError, match="nearest: floor is NaN"):
        nconv_amd.nearest_sample(z, floor=float("nan"))
    with pytest.raises(TypeError, match="nearest: S: expected torch.float32"):
        nconv_amd.nearest_sample(z.double())
    with pytest.raises(TypeError, match="nearest: S must be a tensor"):
        nconv_amd.nearest_sample(z.numpy())
    with pytest.raises(ValueError, match="nearest: S of shape"):
        nconv_amd.nearest_sample(torch.ones(2, 3, 6, 8))
    with pytest.raises(ValueError, match="nearest: S of shape"):
        nconv_amd.nearest_sample(torch.ones(8, 6).t())
    assert [M._max_dist2(m) for m in (None, 0, 1.5, 5, 1e30, float("inf"))] == [NC.max_dist2_of(m) for m in (None, 0, 1.5, 5, 1e30, np.inf)]
    for cls, args in ((nconv_amd.NearestFiller, ((6, 8),)), (nconv_amd.NearestFill, ()), (nconv_amd.NearestSample, ())):
        with pytest.raises(TypeError, match="takes no option 'out'"):
            cls(*args, out={})
        with pytest.raises(TypeError, match="takes no option 'window'"):
            cls(*args, window=3)
    for cls in (nconv_amd.NearestFill, nconv_amd.NearestSample):  # one plane out: no extra outputs
        with pytest.raises(TypeError, match="takes no option 'return_index'"):
            cls(return_index=True)
    m = nconv_amd.NearestFill(max_distance=8, floor=None)
    assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and "max_distance=8" in repr(m)
    assert m.eval() is m and m.to("cpu") is m
    st = nconv_amd.NearestSample(dist_key="dist")
    assert (st.key, st.out_key, st.dist_key) == ("depth", "filled", "dist") and nconv_amd.NearestSample().dist_key is None


@pytest.mark.parametrize("key, bad", (("depth", torch.ones(2, 1, 6, 7)), ("depth", torch.ones(2, 1, 6, 8).double()),
                                      ("index", torch.ones(2, 6, 8)), ("index", torch.ones(2, 1, 6, 8).int()),
                                      ("dist2", torch.ones(2, 6, 9).int()), ("dist", torch.ones(2, 6, 8).int()),
                                      ("dist", torch.ones(2, 8, 6).transpose(1, 2)), ("work", torch.ones(2, 6, 8)),
                                      ("work", torch.ones(1, 6, 8).int())),
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v.shape)) + str(v.dtype)[6:])
def test_python_refuses_bad_out_shapes(nconv_amd, key, bad):
    """The out buffers are checked before the device is asked for: shapes, dtypes and contiguity."""
    z = torch.ones(2, 1, 6, 8)
    with pytest.raises(TypeError, match=f"nearest: out\\[{key!r}\\]"):
        nconv_amd.nearest_sample(z, return_index=True, return_dist2=True, return_dist=True, out={key: bad})
