"""The confidence loss without a GPU: the fp32 rule of include/nconv.h (confloss_cases.rule_fp32, what the
kernels reproduce bit for bit) against float64 autograd of the published formula, and the host-side
argument checks of nconv_conf_loss_* / nconv_bwd_tail_conf from a plain C program."""
import numpy as np
import pytest
import torch

import confloss_cases as CC
from host_harness import host_report

U = 2.0 ** -24  # the unit round-off of fp32


@pytest.mark.parametrize("lam", [1.0, 0.25])
@pytest.mark.parametrize("err,beta", [("smooth_l1", 1.0), ("smooth_l1", 0.5), ("l2", 1.0)])
def test_fp32_rule_matches_published_formula(err, beta, lam):
    """L, g_r, g_c of the fp32 rule against float64 autograd of the published loss. Per element: g_r =
    (k de)(1 + lam c) is a product of factors each a few roundings from exact (d = r - t is rounded
    once, relative to d itself), so within 8 ulps of itself; g_c = -(k lam)(1 - e) loses relative
    accuracy where e is near 1, its error being that of e: within 8 u k lam (1 + e). The values are
    identical (zero) where t == 0, and g_r is exactly 0 where d == 0."""
    g = torch.Generator().manual_seed(3)
    r, c, t = CC.loss_inputs(g, (2, 1, 45, 67), beta)
    terms, g_r, g_c = CC.rule_fp32(r.numpy(), c.numpy(), t.numpy(), lam, err, beta, gloss=1.0)
    n = r.numel()
    r64 = r.double().requires_grad_(True)
    c64 = c.double().requires_grad_(True)
    L64 = CC.published_loss(r64, c64, t.double(), lam, err, beta)
    L64.backward()
    L32 = terms.astype(np.float64).sum() / n
    assert abs(L32 - L64.item()) <= CC.loss_bound(r, c, t, lam, err, beta)
    ref_r, ref_c = r64.grad.numpy(), c64.grad.numpy()
    assert (np.abs(g_r - ref_r) <= 8 * U * np.abs(ref_r)).all()
    d = (r.double() - t.double())
    a = d.abs()
    e = (torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta) if err == "smooth_l1" else d * d).numpy()
    assert (np.abs(g_c - ref_c) <= 8 * U * (lam / n) * (1 + e)).all()
    invalid = (t == 0).numpy()
    assert invalid.any() and (g_r[invalid] == 0).all() and (g_c[invalid] == 0).all() and (terms[invalid] == 0).all()
    assert (ref_r[invalid] == 0).all() and (ref_c[invalid] == 0).all()
    same = ((r == t) & (t != 0)).numpy()
    assert same.any() and (g_r[same] == 0).all() and (ref_r[same] == 0).all()
    # e == 0 there: the term is -lam c and g_c is -k lam, both exact up to one product's rounding
    assert (terms[same] == -(np.float32(lam) * c.numpy()[same])).all()
    if err == "smooth_l1":  # |d| == beta takes the linear branch in both statements
        edge = ((r - t).abs() == beta).numpy() & ~invalid
        assert edge.any() and (np.abs(g_r[edge]) > 0).all()


def test_gloss_scales_the_gradients():
    g = torch.Generator().manual_seed(4)
    r, c, t = CC.loss_inputs(g, (1, 1, 8, 16))
    _, a_r, a_c = CC.rule_fp32(r.numpy(), c.numpy(), t.numpy(), 1.0, gloss=1.0)
    _, b_r, b_c = CC.rule_fp32(r.numpy(), c.numpy(), t.numpy(), 1.0, gloss=2.0)
    assert (b_r == 2 * a_r).all() and (b_c == 2 * a_c).all()  # a power of two: exact


@pytest.fixture(scope="module")
def report(nconv_amd, tmp_path_factory):
    return host_report(nconv_amd, tmp_path_factory, "confloss_host")


def test_host_workspace_sizes(report):
    small, full, zero_b, neg_w = report["ws"]
    tiles = lambda B, H, W: B * ((H + 15) // 16) * ((W + 63) // 64)  # noqa: E731
    assert small == 2 * 8 + tiles(2, 4, 8) * 4
    assert full == 8 * 8 + tiles(8, 352, 1216) * 4
    assert zero_b == 0 and neg_w == 0
    assert report["abi"] == [27, 27]


@pytest.mark.parametrize("case,why", [
    ("null_r", "null plane"), ("null_c", "null plane"), ("null_t", "null plane"), ("null_lam", "null lam"),
    ("B_zero", "non-positive"), ("H_negative", "non-positive"),
    ("beta_zero", "beta must be positive"), ("beta_negative", "beta must be positive"),
    ("beta_nan", "beta must be positive"), ("kind_2", "unknown err_kind"), ("kind_negative", "unknown err_kind"),
    ("r_row_stride_short", "row stride smaller than W"), ("c_image_stride_short", "image stride smaller"),
    ("r_plane_too_large", "plane too large"), ("c_plane_too_large", "plane too large"),
    ("t_plane_too_large", "plane too large")])
def test_host_refuses_bad_arguments(report, case, why):
    for side in ("fwd", "bwd"):
        rc, text = report[f"{side}_{case}"]
        assert rc == -22 and why in text and f"nconv_conf_loss_{side}" in text, (side, rc, text)


def test_host_forward_and_backward_only_checks(report):
    assert report["fwd_null_loss_or_outputs"][0] == -22 and "null loss" in report["fwd_null_loss_or_outputs"][1]
    assert report["bwd_null_loss_or_outputs"][0] == -22 and "null g_r and g_c" in report["bwd_null_loss_or_outputs"][1]
    for case in ("workspace_small_fwd_only", "workspace_null_fwd_only"):
        assert report[f"fwd_{case}"][0] == -22 and "workspace too small" in report[f"fwd_{case}"][1]


def test_host_tail_conf_null_plane_is_bwd_ex(report):
    """nconv_bwd_tail_conf(tail_gcout = NULL) goes through nconv_bwd_ex's checks with its message (here a
    workspace one byte short); the plane without io->tail and a null io are refused."""
    assert report["need"][0] > 0
    assert report["tail_ex"][0] == -22 and "workspace too small" in report["tail_ex"][1]
    assert report["tail_conf_null"] == report["tail_ex"]
    assert report["tail_conf_no_tail"][0] == -22 and "tail_gcout without a tail" in report["tail_conf_no_tail"][1]
    assert report["tail_conf_null_io"][0] == -22 and "null io" in report["tail_conf_null_io"][1]
