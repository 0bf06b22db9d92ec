"""The cross-view consistency rules without a GPU: the fp32 restatements (consistency_cases.rule_fp32,
loss_rule_fp32: what the kernels reproduce bit for bit in test_gpu_consistency.py) against the float64 composition
within kappa x the derived majorants, kappa measured from torch's own float32 run of the composition
(tests/golden/consistency_bound_kappa.json); the decisions against float64 on the analytic scene; the Python
argument checks; and the C boundary through tests/host/consistency_host.c."""
import ctypes

import numpy as np
import pytest
import torch

import consistency_cases as CC
import host_harness


@pytest.fixture(scope="module")
def kappa():
    return CC.kappa_for(CC.load_kappa())


def test_kappa_file_is_complete_and_current():
    """The stored table has every case and output, kappa = 4 x kappa_ref, and measuring again gives the stored
    values (torch's float32 kernels may differ in the last digits between builds: 25 % of slack on kappa_ref,
    which is itself a factor 4 below what is applied)."""
    table = CC.load_kappa()
    assert set(table) == {c[0] for c in CC.CPU_CASES}
    now = CC.measure_kappa()
    for name, row in table.items():
        assert set(row) == set(CC.OUTPUTS), name
        for key, v in row.items():
            assert v["kappa"] == pytest.approx(4 * v["kappa_ref"], rel=2e-3) and v["kappa_ref"] > 0, (name, key)
            assert now[name][key]["kappa_ref"] == pytest.approx(v["kappa_ref"], rel=0.25), (name, key, now[name][key])


@pytest.mark.parametrize("name", [c[0] for c in CC.CPU_CASES])
def test_fp32_rule_within_the_float64_budget(name, kappa):
    """reproj, reldiff, fused, the loss and its gradient of the fp32 rule against the float64 composition of
    grid_sample, matrix products and autograd, in units of the majorants, on the pixels where the rule's decisions
    are the reference's and the blend has no kink."""
    x, ref, per = CC.case_budget(name)
    S = len(x["src_depths"])
    rule = CC.rule_fp32(*CC._args(x), mask=x["mask"])
    losses = [CC.loss_rule_fp32(x["depth"], x["k"], x["src_depths"][s], x["ms"][s], x["mask"], gloss=CC.GLOSS)
              for s in range(S)]
    seen = np.isfinite(rule["reproj"])
    same = (seen == ref["seen"]) & (rule["cons"] == ref["cons"])
    r = CC.ratios(rule, losses, ref, per, same)
    for s in range(S):
        assert losses[s]["n_g"] == ref[f"n_g_{s}"] or abs(losses[s]["n_g"] - ref[f"n_g_{s}"]) <= 2, s
        assert per[s]["keep"].sum() > 0.1 * ref["seen"][:, s].sum() > 0
    print(name, {key: f"{v:.3g} / {kappa[key]:.3g}" for key, v in r.items()}, f"decisions differ on "
          f"{int((~same).sum())} of {same.size}")
    assert (~same).mean() < 0.01
    for key in CC.OUTPUTS:
        assert r[key] <= kappa[key], (key, r[key], kappa[key])
    # where the round trip is not defined both say +inf, and off the counted pixels the gradient is +0
    assert np.array_equal(np.isinf(rule["reproj"]), np.isinf(rule["reldiff"]))
    for s in range(S):
        assert (losses[s]["g_depth"][~losses[s]["counted"]] == 0).all()


def test_decisions_against_float64_on_the_analytic_scene():
    """count and views of the fp32 rule are float64's on every pixel of the wall-and-rectangle scene that is at
    least 2 px from a silhouette edge in either view (the margins are large there by construction), and they are
    the expected ones."""
    x = CC.analytic_scene()
    rule = CC.rule_fp32(*CC._args(x))
    ref = CC.composition(*CC._args(x))
    stated = x["expect"] >= 0
    assert stated.mean() > 0.8
    assert np.array_equal(rule["count"][stated], ref["count"][stated])
    assert np.array_equal(rule["views"][stated], ref["views"][stated])
    assert np.array_equal(rule["count"][stated], x["expect"][stated].astype(np.uint8))
    for kind in ("seen", "hidden", "left", "rect"):
        assert (x["kind"] == kind).sum() > 20, kind
    f = rule["fused"]
    assert (f[rule["count"] < 1] == 0).all() and np.isfinite(f).all() and (f[rule["count"] >= 1] > 0).all()


def test_min_views_and_tolerances_of_the_rule():
    x = CC.scene(7, 2, (17, 65), (19, 70), S=2, sparse=True)  # holes: pixels with one or no consistent source
    a = CC._args(x)
    r1, r0, r2 = (CC.rule_fp32(*a, min_views=mv) for mv in (1, 0, 2))
    assert np.array_equal(r1["count"], r0["count"]) and np.array_equal(r1["count"], r2["count"])
    lone = r0["pvalid"] & (r0["count"] == 0)
    assert lone.any() and np.array_equal(r0["fused"][lone], x["depth"][lone]) and (r1["fused"][lone] == 0).all()
    assert (r2["fused"][r2["count"] < 2] == 0).all() and (r2["fused"][r2["count"] == 2] > 0).all()
    tight = CC.rule_fp32(*a, px_tol=0.5, rel_tol=0.002)
    assert (r1["cons"] >= tight["cons"]).all() and r1["cons"].sum() > tight["cons"].sum() > 0
    assert np.array_equal(tight["reproj"], r1["reproj"])  # the errors do not depend on the thresholds


def test_inverse_pose(nconv_amd):
    p = torch.tensor(np.stack([CC.W.rigid(0.1, -0.2, 0.3, (0.5, -1.0, 2.0)), CC.W.rigid(t=(1.0, 2.0, 3.0))]))
    inv = nconv_amd.inverse_pose(p)
    assert inv.shape == (2, 3, 4) and inv.dtype == torch.float64
    for b in range(2):
        assert np.allclose(inv[b].numpy(), CC.inverse_rigid(p[b].numpy()), atol=1e-15)
    assert nconv_amd.inverse_pose(p[0].float()).shape == (1, 3, 4)
    full = torch.eye(4, dtype=torch.float64)
    full[:3] = p[0]
    assert torch.equal(nconv_amd.inverse_pose(full)[0], inv[0])
    with pytest.raises(ValueError, match="pose must be"):
        nconv_amd.inverse_pose(torch.zeros(3, 3))
    with pytest.raises(TypeError, match="pose"):
        nconv_amd.inverse_pose(np.zeros((3, 4)))


def test_python_argument_checks(nconv_amd):
    """Shapes, dtypes, counts and gradients are refused before any device is asked for (CPU tensors)."""
    d = torch.ones(2, 1, 8, 16)
    k = torch.eye(3)
    pose = torch.tensor(CC.W.rigid(), dtype=torch.float32)
    dc, geo = nconv_amd.depth_consistency, nconv_amd.geometry_consistency_loss
    with pytest.raises(TypeError, match="sequence"):
        dc(d, k, d, [k], [pose])
    with pytest.raises(ValueError, match="1..4"):
        dc(d, k, [d] * 5, [k] * 5, [pose] * 5)
    with pytest.raises(ValueError, match="one per source"):
        dc(d, k, [d, d], [k], [pose, pose])
    with pytest.raises(ValueError, match="min_views"):
        dc(d, k, [d], [k], [pose], min_views=2)
    with pytest.raises(ValueError, match="min_views"):
        dc(d, k, [d], [k], [pose], min_views=-1)
    with pytest.raises(ValueError, match="rel_tol"):
        dc(d, k, [d], [k], [pose], rel_tol=float("nan"))
    with pytest.raises(TypeError, match="Python numbers"):
        dc(d, k, [d], [k], [pose], px_tol=torch.tensor(1.0))
    with pytest.raises(ValueError, match=r"\(H, W\), \(1, H, W\) or \(B, 1, H, W\)"):
        dc(torch.ones(2, 3, 8, 16), k, [d], [k], [pose])
    with pytest.raises(TypeError, match="float32"):
        dc(d.double(), k, [d], [k], [pose])
    with pytest.raises(ValueError, match=r"src_depth must be \(H, W\)"):
        geo(d, k, torch.ones(2, 2, 8, 16), k, pose)
    with pytest.raises(ValueError, match="scatter"):
        geo(d, k, d.clone().requires_grad_(True), k, pose)
    with pytest.raises(ValueError, match="requires a gradient"):
        geo(d, k.clone().requires_grad_(True), d, k, pose)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        geo(d, k, d, k, pose)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        dc(d[0, 0], k, [d[0, 0]], [k], [pose])
    with pytest.raises(ValueError, match="z_min"):
        nconv_amd.GeometryConsistencyLoss(z_min=-1.0)
    with pytest.raises(ValueError, match="S in 1..4"):
        nconv_amd.DepthFuser((8, 16), S=5, device="cpu")
    with pytest.raises(ValueError, match="empty or too large"):
        nconv_amd.consistency.workspace_bytes(0, 8, 16)
    assert nconv_amd.consistency.workspace_bytes(3, 17, 65) == nconv_amd.warp.workspace_bytes(3, 17, 65)


def test_ctypes_layout_matches_the_header(nconv_amd):
    s = nconv_amd._lib.NconvConsistencySource
    assert ctypes.sizeof(s) == 32 and [f for f, _ in s._fields_] == ["k_src", "k_src_image_stride", "m_back",
                                                                     "m_back_image_stride"]
    for name in ("nconv_depth_consistency", "nconv_geo_consistency_workspace_bytes",
                 "nconv_geo_consistency_loss_fwd", "nconv_geo_consistency_loss_bwd"):
        assert name in nconv_amd._lib.EXPORTED and hasattr(nconv_amd._lib.lib(), name)


@pytest.fixture(scope="module")
def host(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "consistency_host")


# what the reason must name, for the cases where another check could have refused the call first
REASON = {"C_3": "C must be 1", "C_2": "C must be 1 or 3", "null_k_src": "null k_src or m_back",
          "null_m_back": "null k_src or m_back", "k_src_stride_negative": "negative k_src or m_back image stride",
          "m_back_stride_negative": "negative k_src or m_back image stride", "S_five": "S must be in 1..4",
          "S_zero": "S must be in 1..4", "px_tol_negative": "px_tol and rel_tol", "px_tol_nan": "px_tol and rel_tol",
          "rel_tol_negative": "px_tol and rel_tol", "rel_tol_nan": "px_tol and rel_tol",
          "min_views_negative": "min_views must be in 0..S", "min_views_above_S": "min_views must be in 0..S",
          "no_output": "nothing to write", "fused_misaligned": "not 4-byte aligned",
          "differ_depth": "differs from view 0 in the depth view", "differ_k": "differs from view 0 in k",
          "differ_in_third_view": "view 2 differs from view 0 in z_min or z_max",
          "workspace_small": "workspace too small", "workspace_null": "workspace too small",
          "workspace_misaligned": "workspace not 8-byte aligned", "src_plane_too_large": "plane too large",
          "null_depth": "null depth, src, k or m", "z_min_nan": "z_min must be >= 0",
          "depth_row_stride_short": "depth: row stride smaller than W", "W_above_2_24": "at most 2^24"}


def test_c_boundary_refuses_every_invalid_call(host, nconv_amd):
    assert host["abi"] == [27, 27]
    ws = host["ws"]
    assert ws[0] > 0 and ws[1] > ws[0] and ws[2] == 0 and ws[3] == 0 and ws[4] == ws[5] > 0
    assert ws[0] == nconv_amd.consistency.workspace_bytes(2, 4, 8)
    calls = {key: v for key, v in host.items() if key not in ("abi", "ws")}
    assert len(calls) > 150
    sides = {key.split("_", 1)[0] for key in calls}
    assert sides == {"check", "fwd", "bwd"}
    fn = {"check": "nconv_depth_consistency", "fwd": "nconv_geo_consistency_loss_fwd",
          "bwd": "nconv_geo_consistency_loss_bwd"}
    for key, (rc, text) in calls.items():
        side, name = key.split("_", 1)
        assert rc == -22, (key, rc, text)
        assert text.startswith(fn[side] + ": "), (key, text)
        view = None
        if name[:3] in ("v0_", "v1_"):
            view, name = int(name[1]), name[3:]
        if side == "check" and view is not None:
            assert f"view {view}: " in text, (key, text)
        if name in REASON:
            assert REASON[name] in text, (key, text)
    for name in ("null_output", "output_misaligned"):
        assert "null loss" in host["fwd_" + name][1] or "aligned" in host["fwd_" + name][1]
        assert "null g_depth" in host["bwd_" + name][1] or "aligned" in host["bwd_" + name][1]
