"""The pose rule's numpy restatement (pose_cases.py) held to what it must do, on the CPU: its Jacobian against
central differences, the Cayley retraction's orthogonality, convergence on the analytic scene within the bound
of tests/golden/pose_bound.json (MARGIN x the restatement's own final error), the degenerate cases, the Huber
weight, the pyramid's sparse pool and the three-level run; and the Python argument checks of pose.py."""
import numpy as np
import pytest
import torch

import pose_cases as pc
import warp_cases

f32 = np.float32


def _levels(nconv_amd, sc, levels):
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    lvs = nconv_amd.pose.pyramid(T(sc["depth"])[:, None], T(sc["k"]), T(sc["tgt"]), T(sc["src"]), T(sc["k_src"]),
                                 levels, T(sc["mask"]), 1e-3, None)
    return [dict(depth=l["depth"][:, 0].numpy(), k=l["k"].numpy(), tgt=l["tgt"].numpy(), src=l["src"].numpy(),
                 k_src=l["k_src"].numpy(), mask=None if l["mask"] is None else l["mask"].numpy()) for l in lvs]


@pytest.fixture(scope="module")
def runs():
    """The restatement's 8 iterations on the two 48 x 64 scenes, with the errors after every update."""
    out = {}
    for name, motion in (("small", pc.SMALL), ("large", pc.LARGE)):
        sc = pc.scene(motion=motion)
        errs = []
        r = pc.align([sc], iters=8, trace=lambda l, it, st: errs.append(pc.pose_error(st[0], sc["true"])))
        out[name] = (sc, r, errs)
    return out


def test_bound_json_is_current():
    assert pc.load_bound() == pc.measure_bound()


def test_jacobian_matches_central_differences():
    sc = pc.scene(motion=pc.LARGE)
    T = pc.true_pose((0.03, 0.01, -0.05), (0.002, 0.004, -0.003)).tolist()
    ii, jj = np.nonzero(sc["depth"][0] > 0)
    pix, z = np.stack((ii, jj), axis=1), sc["z_dense"][0][ii, jj].astype(np.float64)
    tgt = sc["tgt"][0, 0][ii, jj].astype(np.float64)
    _, uvQ = pc.residual64(pc.image, z, sc["k"], sc["k_src"], tgt, T, pix)
    J = pc.jacobian64(pc.image_grad, sc["k_src"], uvQ)
    h = 1e-6
    for n in range(6):
        d = np.zeros(6)
        d[n] = h
        rp, _ = pc.residual64(pc.image, z, sc["k"], sc["k_src"], tgt, pc.retract(T, list(d)), pix)
        rm, _ = pc.residual64(pc.image, z, sc["k"], sc["k_src"], tgt, pc.retract(T, list(-d)), pix)
        num = (rp - rm) / (2 * h)
        # central differences of a smooth function: O(h^2) truncation plus rounding eps |r| / h
        assert np.abs(num - J[:, n]).max() <= 1e-5 * max(1.0, np.abs(J[:, n]).max()), n


def test_fp32_jacobian_terms_follow_the_float64_jacobian():
    """The fp32 rule's sum J r against the float64 Jacobian on the bilinear image: the same formulas."""
    sc = pc.scene(motion=pc.SMALL)
    eye = np.eye(3, 4)
    m = pc.project(sc["k_src"], eye.tolist())[None]
    terms, valid, aux = pc.terms_fp32(sc["depth"], sc["k"], sc["tgt"], sc["src"], sc["k_src"], m, eye.astype(f32)[None])
    ii, jj = np.nonzero(valid[0])
    pix, z = np.stack((ii, jj), axis=1), sc["depth"][0][ii, jj].astype(np.float64)
    _, uvQ = pc.residual64(pc.image, z, sc["k"], sc["k_src"], 0.0, eye, pix)
    g = lambda u, v: (aux["dIu"][0][0][ii, jj].astype(np.float64), aux["dIv"][0][0][ii, jj].astype(np.float64))  # noqa: E731
    J = pc.jacobian64(g, sc["k_src"], uvQ)
    r = (aux["s"][0][0] - sc["tgt"][0, 0])[ii, jj].astype(np.float64)
    b64 = J.T @ r
    b32 = terms[0, 21:27].astype(np.float64).sum(axis=(1, 2))
    assert np.abs(b32 - b64).max() <= 1e-4 * np.abs(J * r[:, None]).sum(axis=0).max()


def test_shares_the_warp_rule_bit_for_bit():
    x = warp_cases.warp_inputs(5, 2, 3, (17, 65), (19, 70), True, True)
    pose = np.stack([warp_cases.rigid(0.004, -0.006, 0.003, (0.1, 0.0, 0.3))] * 2).astype(f32)
    _, valid, aux = pc.terms_fp32(x["depth"], x["k"], x["tgt"], x["src"], x["k"], x["m"], pose, x["mask"], 0.0, 0.0)
    ref = warp_cases.rule_fp32(x["depth"], x["k"], x["src"], x["m"], x["mask"], x["tgt"])
    assert np.array_equal(valid, ref["valid"])
    assert aux["u"].tobytes() == ref["u"].tobytes() and aux["v"].tobytes() == ref["v"].tobytes()
    for ch in range(3):
        assert np.array_equal(np.where(valid, aux["s"][ch], f32(0)), ref["warped"][:, ch])


def test_cayley_is_orthogonal():
    for omega in ((0.004, -0.006, 0.003), (0.3, -0.2, 0.5), (2.0, 1.0, -3.0), (0.0, 0.0, 0.0)):
        R = np.array(pc.cayley(omega))
        assert np.abs(R @ R.T - np.eye(3)).max() <= 8 * np.finfo(np.float64).eps
        assert abs(np.linalg.det(R) - 1.0) <= 8 * np.finfo(np.float64).eps
    state = np.eye(3, 4).tolist()
    for _ in range(200):   # the double state: orthogonality does not drift over many retractions
        state = pc.retract(state, [0.01, -0.02, 0.03, 0.02, -0.01, 0.015])
    R = np.array(state)[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 200 * 8 * np.finfo(np.float64).eps


@pytest.mark.parametrize("name", ["small", "large"])
def test_converges_on_the_analytic_scene(runs, name):
    sc, r, errs = runs[name]
    bound = pc.load_bound()[name]
    init = pc.pose_error(np.eye(3, 4), sc["true"])[0]
    print(name, "t err", [f"{e[0]:.4g}" for e in errs], "cost", r["cost"][0, 0].tolist())
    assert errs[-1][0] <= bound["t_err_bound"] and errs[-1][1] <= bound["r_err_bound"]
    assert errs[-1][0] < init / 10
    assert (r["status"] == 0).all()
    # the cost does not rise after iteration 1, up to what fp32 can tell: a residual of 255-valued frames
    # carries the blend's 8 roundings, dr = 8 * 2^-24 * 255, and d(r^2) <= 2 |r| dr + dr^2 with |r| ~ sqrt(cost)
    cost = r["cost"][0, 0].astype(np.float64)
    dr = 8 * 2.0 ** -24 * 255
    for it in range(1, len(cost) - 1):
        assert cost[it + 1] <= cost[it] + 2 * np.sqrt(cost[it]) * dr + dr * dr, (it, cost)


def test_degenerate_images_keep_their_pose():
    sc = pc.scene(motion=pc.SMALL, B=3, seed=3)
    depth = sc["depth"].copy()
    depth[0] = 0.0                                     # no sample
    pix = np.argwhere(depth[1] > 0)
    far = pix[np.argsort(np.abs(pix - np.array([24, 32])).sum(axis=1))[5:]]
    depth[1][far[:, 0], far[:, 1]] = 0.0               # five samples, the ones nearest the centre
    src = sc["src"].copy()
    src[2] = 100.0                                     # a constant source: H = 0
    lv = dict(sc, depth=depth, src=src)
    init = pc.true_pose((0.01, 0.02, -0.03), (0.001, 0.002, 0.003))
    r = pc.align([lv], init=init, iters=2, min_points=6)
    assert r["n"][0, :, 0].tolist()[:2] == [0, 5]
    assert r["status"][0].tolist() == [1, 1, 2]
    for b in range(3):
        assert np.array(r["state"][b]).tobytes() == init.tobytes()
        assert r["pose"][b].tobytes() == init.astype(f32).tobytes()


@pytest.mark.parametrize("name", ["small", "large"])
def test_huber_weight_resists_outliers(runs, name):
    sc = pc.with_outliers(runs[name][0])
    bound = pc.load_bound()[name]
    with_w = pc.pose_error(pc.align([sc], iters=8, huber=pc.OUTLIER_HUBER)["state"][0], sc["true"])[0]
    without = pc.pose_error(pc.align([sc], iters=8, huber=0.0)["state"][0], sc["true"])[0]
    print(name, "with", with_w, "without", without)
    assert with_w <= bound["t_err_bound"] < without


def test_pool_sparse_matches_the_loop(nconv_amd):
    g = torch.Generator().manual_seed(0)
    z = (torch.rand(2, 1, 10, 14, generator=g) * 20 + 1) * (torch.rand(2, 1, 10, 14, generator=g) < 0.3)
    z[0, 0, 0, 0], z[0, 0, 0, 1] = float("nan"), 3.0
    z[0, 0, 2, 2:4], z[0, 0, 3, 2:4] = float("nan"), float("inf")
    z[1, 0, 4, 4], z[1, 0, 5, 5] = -2.0, 1e-4
    z[:, :, 6:8, 6:10] = 0.0                                         # all-empty cells
    mask = torch.rand(2, 1, 10, 14, generator=g) > 0.2
    for mk, zmax in ((None, None), (mask, None), (mask, 15.0)):
        got = nconv_amd.pool_sparse(z, mk, 1e-3, zmax)[:, 0].numpy()
        want = pc.pool_loop(z[:, 0].numpy(), None if mk is None else mk[:, 0].numpy(), 1e-3, 0.0 if zmax is None else zmax)
        assert got.tobytes() == want.tobytes()
    assert nconv_amd.pool_sparse(z)[0, 0, 0, 0] == 3.0 and nconv_amd.pool_sparse(z)[0, 0, 1, 1] == 0.0


def test_three_levels_converge_where_one_does_not(nconv_amd):
    sc = pc.scene(**pc.PYRAMID_SCENE)
    init = pc.pose_error(np.eye(3, 4), sc["true"])[0]
    one = pc.pose_error(pc.align(_levels(nconv_amd, sc, 1), iters=8)["state"][0], sc["true"])[0]
    three = pc.pose_error(pc.align(_levels(nconv_amd, sc, 3), iters=8)["state"][0], sc["true"])[0]
    print("flow", pc.max_flow(sc), "one level", one, "three levels", three)
    assert three < init / 10 and three <= max(b["t_err_bound"] for b in pc.load_bound().values() if isinstance(b, dict))
    assert one > init / 10


def test_python_argument_checks(nconv_amd):
    z = torch.zeros(1, 1, 6, 8)
    k = torch.eye(3)
    img = torch.zeros(1, 1, 6, 8)
    with pytest.raises(ValueError, match="levels"):
        nconv_amd.pose.pyramid(z, k, img, img, k, 3)             # 6 x 8 -> 3 x 4: odd at level 1
    with pytest.raises(ValueError, match="levels"):
        nconv_amd.pose.pyramid(z, k, img, img, k, 0)
    with pytest.raises(ValueError, match="min_points"):
        nconv_amd.estimate_pose(z, k, img, img, min_points=5)
    with pytest.raises(ValueError, match="huber"):
        nconv_amd.estimate_pose(z, k, img, img, huber=-1.0)
    with pytest.raises(ValueError, match="damping"):
        nconv_amd.estimate_pose(z, k, img, img, damping=float("nan"))
    with pytest.raises(TypeError, match="huber"):
        nconv_amd.estimate_pose(z, k, img, img, huber=torch.tensor(1.0))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        nconv_amd.estimate_pose(z, k, img, img, levels=1)
    with pytest.raises(TypeError, match="no option"):
        nconv_amd.EstimatePose(lvls=2)
    batch = {"rgb": img, "depth": z, "k": k}
    assert nconv_amd.EstimatePose()(batch) is batch              # no neighbouring frame: untouched
    for name in ("EstimatePose", "PoseEstimator", "estimate_pose", "pose_step", "pool_sparse", "pose_projection"):
        assert name in nconv_amd.__all__


def test_pose_projection_matches_the_restatement(nconv_amd):
    T = pc.true_pose((0.3, -0.2, 0.7), (0.02, 0.05, -0.03))
    k = warp_cases.intrinsics(48, 64, 57.6).astype(f32)
    got = nconv_amd.pose_projection(torch.from_numpy(k), torch.from_numpy(T)[None])[0].numpy()
    assert got.tobytes() == pc.project(k, T.tolist()).tobytes()
    ref = nconv_amd.warp_projection(torch.from_numpy(k), torch.from_numpy(T))[0].numpy()
    assert np.abs(got - ref).max() <= np.spacing(np.abs(ref).max())
