"""CPU: the numpy reference of the sparsification curves checks itself (a hand-computed example with ties,
oracle <= confidence, conf = -a, raster order under equal confidence, NaN first, uncertainty, k_j); the two
entry points are exported, declared and bound with the C struct's layout under an unchanged ABI number; every
malformed call fails on the host with -22 and its message before any launch; the Python function refuses CPU
tensors and bad arguments; the shapes of the GPU tests are sized from the kernel file's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import host_harness
import sparsification_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
NEW = ("nconv_depth_sparsification_workspace_bytes", "nconv_depth_sparsification")
F32 = np.float32


# ---- the reference ---------------------------------------------------------------------------------
def test_hand_computed_example_with_ties():
    """3 x 4, gt 0 at pixels 2 and 9. Errors a (valid pixels 0 1 3 4 5 6 7 8 10 11):
         1 2 . 4 / 2 1 8 1 / 0.5 . 2 4
    conf 0.5 everywhere but 0.25 at pixels 3, 6 and 1.0 at pixel 0."""
    gt = np.full((1, 3, 4), 10, dtype=F32)
    gt.reshape(-1)[[2, 9]] = 0
    a = np.array([1, 2, 7, 4, 2, 1, 8, 1, 0.5, 7, 2, 4], dtype=F32)
    pred = (gt + a.reshape(1, 3, 4)).astype(F32)
    conf = np.full((1, 3, 4), 0.5, dtype=F32)
    conf.reshape(-1)[[3, 6]] = 0.25
    conf.reshape(-1)[0] = 1.0
    curves, order, n = SC.sparsification_ref(pred, gt, conf, steps=5)
    assert n.tolist() == [10]
    # confidence: 0.25 first (3, 6), the 0.5 ties in raster order, 1.0 last
    assert order[0, 0].tolist() == [3, 6, 1, 4, 5, 7, 8, 10, 11, 0, -1, -1]
    # oracle: 8 (6), the 4s (3, 11), the 2s (1, 4, 10), the 1s (0, 5, 7), 0.5 (8)
    assert order[0, 1].tolist() == [6, 3, 11, 1, 4, 10, 0, 5, 7, 8, -1, -1]
    assert curves[0, :, :, 0].tolist() == [[10, 8, 6, 4, 2]] * 2  # k = 0 2 4 6 8
    assert curves[0, 0, :, 1].tolist() == [25.5, 13.5, 9.5, 7.5, 5.0]
    assert curves[0, 1, :, 1].tolist() == [25.5, 13.5, 7.5, 3.5, 1.5]
    assert curves[0, 0, :, 2].tolist() == [111.25, 31.25, 23.25, 21.25, 17.0]
    assert curves[0, 1, :, 2].tolist() == [111.25, 31.25, 11.25, 3.25, 1.25]


def test_oracle_is_below_confidence_per_kept_pixel():
    _, _, _, curves, _, n = SC.case(SC.SMALL, "random", seed=3, steps=7)
    pred, gt, conf, curves2, _, n2 = SC.case((2, 9, 13), "four", seed=4, steps=7)
    for c in (curves, curves2):
        kept = c[..., :1]
        mean = c[..., 1:] / np.where(kept > 0, kept, 1)
        assert (mean[:, 1] <= mean[:, 0]).all()


def test_conf_minus_a_follows_the_oracle():
    rng = np.random.default_rng(5)
    gt = np.full((1, 9, 13), 5, dtype=F32)
    a = rng.permutation(117).astype(F32).reshape(1, 9, 13) * F32(0.25)  # tie-free, exact
    pred = gt + a
    curves, order, n = SC.sparsification_ref(pred, gt, -a, steps=11)
    assert n[0] == 117 and np.array_equal(order[0, 0], order[0, 1])
    assert np.array_equal(curves[0, 0], curves[0, 1])  # AUSE exactly 0
    norm = SC.normalised_ref(curves)
    assert ((norm[:, :, 0] - norm[:, :, 1]) == 0).all()
    # with ties in a the two orders agree wherever a has none
    a2 = a.copy()
    a2.reshape(-1)[[3, 50, 77]] = a2.reshape(-1)[10]
    _, o2, _ = SC.sparsification_ref(gt + a2, gt, -a2, steps=11)
    vals = a2.reshape(-1)
    untied = np.array([np.count_nonzero(vals == vals[p]) == 1 for p in o2[0, 1]])
    assert untied.sum() == 113 and np.array_equal(o2[0, 0][untied], o2[0, 1][untied])
    # -a breaks its ties by ascending pixel number, and so does the oracle
    assert np.array_equal(o2[0, 0], o2[0, 1])


def test_equal_confidence_gives_raster_order():
    pred, gt, conf, _, order, n = SC.case((2, 9, 13), "equal", seed=6, steps=3)
    for b in range(2):
        pix = np.flatnonzero(gt[b].reshape(-1) > 0)
        assert np.array_equal(order[b, 0, :n[b]], pix) and (order[b, 0, n[b]:] == -1).all()


def test_nan_confidence_first_and_uncertainty_flips():
    gt = np.full((1, 2, 4), 3, dtype=F32)
    pred = gt + F32(1)
    conf = np.array([0.5, np.nan, -np.inf, 0.0, -0.0, np.inf, 2.0, -np.nan], dtype=F32).reshape(1, 2, 4)
    _, order, _ = SC.sparsification_ref(pred, gt, conf, steps=2)
    assert order[0, 0].tolist() == [1, 7, 2, 4, 3, 0, 6, 5]  # NaNs in raster order, -inf, -0.0 before +0.0
    _, order, _ = SC.sparsification_ref(pred, gt, conf, steps=2, uncertainty=True)
    assert order[0, 0].tolist() == [1, 7, 5, 6, 0, 3, 4, 2]  # NaNs still first, then the largest
    # a NaN error sorts before +inf in the oracle
    pred2 = pred.copy()
    pred2.reshape(-1)[[2, 5]] = [np.inf, np.nan]
    _, order, _ = SC.sparsification_ref(pred2, gt, conf, steps=2, sums=False)
    assert order[0, 1].tolist()[:2] == [5, 2]


def test_steps_k():
    assert SC.steps_k(10, 4) == [0, 2, 5, 7]
    assert SC.steps_k(3, 7) == [0, 0, 0, 1, 1, 2, 2]  # n < J
    assert SC.steps_k(0, 3) == [0, 0, 0] and SC.steps_k(1, 3) == [0, 0, 0]
    big = SC.steps_k(2 ** 31 - 1, 1024)
    assert big[1023] == 1023 * (2 ** 31 - 1) // 1024 and big[1023] > 2 ** 31 - 2 ** 22
    curves, _, n = SC.sparsification_ref(*[np.ones((1, 1, 3), dtype=F32) * v for v in (2, 1, 0.5)], steps=7)
    assert curves[0, 0, :, 0].tolist() == [3, 3, 3, 2, 2, 1, 1]


def test_validity_window_and_clamp():
    gt = np.array([0, 0.5, 1, 50, 80, 81], dtype=F32).reshape(1, 1, 6)
    assert SC.valid_mask(gt).tolist() == [[[False, True, True, True, True, True]]]
    assert SC.valid_mask(gt, 1.0, 80.0).tolist() == [[[False, False, True, True, True, False]]]
    a, q = SC.terms(np.array([0.1, 100, np.nan], dtype=F32), np.array([1, 1, 1], dtype=F32), clamp=(0.9, 80.0))
    assert a[0] == F32(1) - F32(0.9) and a[1] == 79 and np.isnan(a[2]) and q[1] == 79 * 79


def test_shapes_follow_the_kernel_constants():
    k = SC.source_constants()
    assert (k["kT"], k["kTile"], k["kMaxBlocks"], k["kPrepTile"], k["kChunk"]) == (
        SC.THREADS, SC.SORT_TILE, SC.MAX_BLOCKS, SC.PREP_TILE, SC.CHUNK)
    assert k["kDigitBits"] * k["kPasses"] == 32


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
    assert int(re.search(r"#define NCONV_SPARSIFICATION_MAX_STEPS (\d+)", src).group(1)) == 1024
    assert nconv_amd._lib.SPARSIFICATION_MAX_STEPS == 1024
    assert lib.nconv_depth_sparsification_workspace_bytes(2, 4, 8, 10) >= 2 * 4 * 8 * 40
    for bad in ((0, 4, 8, 10), (2, -1, 8, 10), (2, 4, 0, 10), (2, 4, 8, 0), (2, 4, 8, 1025),
                (1 << 15, 1 << 8, 1 << 8, 10)):
        assert lib.nconv_depth_sparsification_workspace_bytes(*bad) == 0


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "sparsification_host")


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    S = nconv_amd._lib.NconvDepthSparsification
    want = host_harness.ctypes_layout(S, "nconv_depth_sparsification")
    c = {k: v for k, v in host_report.items() if k.startswith("nconv_depth_sparsification")}
    assert len(c) == 21 and c == want


HOST_CALLS = (
    ("rc_null_descriptor", "null descriptor"), ("rc_null_pred", "null plane"), ("rc_null_gt", "null plane"),
    ("rc_null_conf", "null plane"), ("rc_null_curves", "null curves"), ("rc_B", "non-positive"),
    ("rc_H", "non-positive"), ("rc_W", "non-positive"), ("rc_steps_low", "steps must be in [1, 1024]"),
    ("rc_steps_high", "steps must be in [1, 1024]"), ("rc_pred_row_stride", "pred: row stride smaller than W"),
    ("rc_gt_row_stride", "gt: row stride smaller than W"), ("rc_conf_row_stride", "conf: row stride smaller than W"),
    ("rc_workspace_small", "workspace too small"), ("rc_workspace_null", "workspace too small"),
    ("rc_workspace_misaligned", "workspace not 8-byte aligned"), ("rc_plane_too_large", "conf: plane too large"),
    ("rc_pixel_numbers", "H * W must be below 2^31"), ("rc_image_stride", "conf: image stride smaller"),
    ("rc_bound", "negative or NaN bound"), ("rc_curves_misaligned", "curves not 8-byte aligned"),
    ("rc_order_misaligned", "4-byte aligned"),
)


def test_host_calls(host_report):
    assert host_report["abi"] == [27, 27]
    need, *none = host_report["workspace_bytes"]
    assert need >= 352 * 1216 * 40 and need % 8 == 0 and none == [0, 0, 0, 0]
    for key, msg in HOST_CALLS:
        rc, err = host_report[key]
        assert rc == -22 and msg in err and err.startswith("nconv_depth_sparsification: "), (key, rc, err)


# ---- Python argument checks ------------------------------------------------------------------------
def test_sparsification_refuses_cpu_tensors_and_bad_arguments(nconv_amd):
    S = nconv_amd.sparsification
    assert nconv_amd.SparsificationCurves.__module__ == S.__module__
    z = torch.ones(2, 1, 4, 8)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        S(z, z, z)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        S(z[0, 0], z[0, 0], z[0, 0], return_order=True)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.SparsificationCurves(steps=10, device="cpu").update(z, z, z)
    with pytest.raises(TypeError, match="pred"):
        S(z.numpy(), z, z)
    for steps in (0, 1025, -3):
        with pytest.raises(ValueError, match="steps"):
            S(z, z, z, steps=steps)
        with pytest.raises(ValueError, match="steps"):
            nconv_amd.SparsificationCurves(steps=steps, device="cpu")
    with pytest.raises(TypeError, match="steps"):
        S(z, z, z, steps=2.5)
    with pytest.raises(ValueError, match="gt_min"):
        S(z, z, z, gt_min=-1.0)
    with pytest.raises(ValueError, match="clamp"):
        S(z, z, z, clamp=(5.0, 1.0))
    c = nconv_amd.SparsificationCurves(steps=4, device="cpu")
    assert c.bounds == (0.0, 80.0, 0.0, 0.0) and tuple(c.state.shape) == (2, 2, 4)
    out = c.compute()
    assert out["images"] == 0 and out["fraction"].tolist() == [0.0, 0.25, 0.5, 0.75] and out["ause_mae"] != out["ause_mae"]
    # the device-side normalisation is the reference's
    curves = SC.case((2, 9, 13), "four", seed=4, steps=7)[3]
    got = nconv_amd.SparsificationCurves.normalised(torch.from_numpy(curves.copy())).numpy()
    assert np.array_equal(got, SC.normalised_ref(curves))
