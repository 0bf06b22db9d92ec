"""nconv_pose_normal_eq / nconv_pose_update on the device against the numpy restatement of their rule
(pose_cases.py), bit for bit: the sums, the counts, the cost, the updated pose and m of one step over tile edges,
strides, masks and per-image cameras; eight iterations of estimate_pose; run-to-run determinism; hipGraph
capture; the estimated m inside the photometric loss; the prefetch stage."""
import numpy as np
import pytest
import torch

import pose_cases as pc
import warp_cases

pytestmark = pytest.mark.gpu
f32 = np.float32


def _inputs(seed, B, C, size, src_size, per_image_k, with_mask):
    """warp_cases' smooth depth, random frames and a forward motion, thinned to a sparse plane: image 0 full,
    the last image of a batch of three empty, the middle one with 7 samples."""
    x = warp_cases.warp_inputs(seed, B, C, size, src_size, True, with_mask)
    H, W = size
    Hs, Ws = src_size or size
    rng = np.random.RandomState(seed)
    depth = np.where(rng.rand(B, H, W) < 0.3, x["depth"], f32(0)).astype(f32)
    if B == 3:
        pix = np.argwhere(np.isfinite(depth[1]) & (depth[1] > 0))
        far = pix[np.argsort(np.abs(pix - np.array([H // 2, W // 2])).sum(axis=1))[7:]]
        depth[1][far[:, 0], far[:, 1]] = 0.0
        depth[2] = 0.0
    f = 0.9 * max(W, 2)
    k, ks = warp_cases.intrinsics(H, W, f), warp_cases.intrinsics(Hs, Ws, f * Ws / W)
    if per_image_k:
        k = np.stack([k * np.array([[1 + 0.01 * b], [1 - 0.01 * b], [1]]) for b in range(B)])
        ks = np.stack([ks * np.array([[1 - 0.01 * b], [1 + 0.01 * b], [1]]) for b in range(B)])
    pose = np.stack([warp_cases.rigid(0.004 * (b + 1), -0.006, 0.003, (0.12 + 0.05 * b, -0.04, 0.45 - 0.1 * b))
                     for b in range(B)])
    return dict(depth=depth, k=k.astype(f32), k_src=ks.astype(f32), tgt=x["tgt"] * 255, src=x["src"] * 255,
                mask=x["mask"], pose=pose)


def _dev(x, gpu):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


STEP_CASES = [  # name, seed, B, C, size, src_size, per-image k, mask, strided depth, huber
    ("17x65_b1_c1", 1, 1, 1, (17, 65), None, False, False, False, 0.0),
    ("17x65_b3_c3_from_19x70_huber", 2, 3, 3, (17, 65), (19, 70), True, False, False, 20.0),
    ("33x130_b3_c1_mask_crop", 3, 3, 1, (33, 130), None, False, True, True, 20.0),
    ("33x130_b1_c3_per_image_k", 4, 1, 3, (33, 130), (35, 128), True, True, False, 0.0),
    ("48x64_b3_c3_crop_huber", 5, 3, 3, (48, 64), None, True, False, True, 30.0),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_pose_step_bit_for_bit(nconv_amd, gpu, case):
    _, seed, B, C, size, src_size, per_k, with_mask, crop, huber = case
    x = _inputs(seed, B, C, size, src_size, per_k, with_mask)
    H, W = size
    depth = _dev(x["depth"], gpu)[:, None]
    if crop:                                              # a cropped view of larger planes
        big = torch.full((B, 1, H + 3, W + 5), 7.0, device=gpu)
        big[:, :, 2:2 + H, 4:4 + W] = depth
        depth = big[:, :, 2:2 + H, 4:4 + W]
    min_points = 8
    pose, m, info = nconv_amd.pose_step(depth, _dev(x["k"], gpu), _dev(x["tgt"], gpu), _dev(x["src"], gpu),
                                        _dev(x["k_src"], gpu), _dev(x["pose"], gpu), mask=_dev(x["mask"], gpu),
                                        huber=huber, min_points=min_points, z_min=1e-3)
    # the restatement: one normal_eq + update from the same start
    states = [x["pose"][b].tolist() for b in range(B)]
    ks = pc._batched(x["k_src"], B, (3, 3))
    p32 = x["pose"].astype(f32)
    m0 = np.stack([pc.project(ks[b], states[b]) for b in range(B)])
    sums, n = pc.normal_eq(x, m0, p32, huber, 1e-3, 0.0)
    want = [pc.update(sums[b], n[b], states[b], ks[b], C, 1e-4, min_points) for b in range(B)]
    got_sums = info["sums"].cpu().numpy()
    assert info["n"].cpu().numpy().tolist() == n.tolist()
    assert got_sums.tobytes() == sums.tobytes(), np.abs(got_sums - sums).max()
    assert info["status"].cpu().numpy().tolist() == [w[3] for w in want]
    assert info["cost"].cpu().numpy().tobytes() == np.array([w[4] for w in want], dtype=f32).tobytes()
    assert info["state"].cpu().numpy().tobytes() == np.array([w[0] for w in want]).tobytes()
    assert pose.cpu().numpy().tobytes() == np.stack([w[1] for w in want]).tobytes()
    assert m.cpu().numpy().tobytes() == np.stack([w[2] for w in want]).tobytes()
    if B == 3:                                            # few samples, none: status 1, the pose as it was
        assert n.tolist()[1:] == [7, 0] or n[1] < min_points
        assert [w[3] for w in want][1:] == [1, 1]
        assert pose.cpu().numpy()[1:].tobytes() == p32[1:].tobytes()
    # m is warp_projection's within one ulp per entry
    ref = nconv_amd.warp_projection(_dev(x["k_src"], gpu), info["state"]).cpu().numpy()
    assert (np.abs(m.cpu().numpy() - ref) <= np.spacing(np.abs(ref))).all()


@pytest.fixture(scope="module")
def scene_run(nconv_amd, gpu):
    """The 48 x 64 scene (B = 2: the small and the large motion), 8 iterations at one level, on both sides."""
    a, b = pc.scene(motion=pc.SMALL), pc.scene(motion=pc.LARGE, seed=1)
    sc = {key: np.concatenate((a[key], b[key])) for key in ("depth", "tgt", "src", "z_dense")}
    sc.update(k=a["k"], k_src=a["k_src"], mask=None)
    want = pc.align([sc], iters=8, huber=0.0, min_points=32)
    args = (_dev(sc["depth"], gpu)[:, None], _dev(sc["k"], gpu), _dev(sc["tgt"], gpu), _dev(sc["src"], gpu))
    got = nconv_amd.estimate_pose(*args, levels=1, iters=8, huber=0.0, return_info=True)
    torch.cuda.synchronize()
    return sc, (a["true"], b["true"]), want, args, got


def test_estimate_pose_bit_for_bit(scene_run):
    sc, _, want, _, (pose, m, info) = scene_run
    assert info["cost"].cpu().numpy().tobytes() == want["cost"].tobytes()
    assert info["n"].cpu().numpy().tolist() == want["n"].tolist()
    assert info["status"].cpu().numpy().tolist() == want["status"].tolist()
    assert info["state"].cpu().numpy().tobytes() == np.array(want["state"]).tobytes()
    assert pose.cpu().numpy().tobytes() == want["pose"].tobytes()
    assert m.cpu().numpy().tobytes() == want["m"].tobytes()


def test_same_bits_on_two_runs(nconv_amd, scene_run):
    _, _, _, args, (pose, m, info) = scene_run
    pose2, m2, info2 = nconv_amd.estimate_pose(*args, levels=1, iters=8, huber=0.0, return_info=True)
    assert torch.equal(pose, pose2) and torch.equal(m, m2) and torch.equal(info["cost"], info2["cost"])
    assert torch.equal(info["state"], info2["state"])


def test_three_levels_against_the_restatement(nconv_amd, gpu):
    """The pyramid built on the device, every level handed to the restatement: the same bits again."""
    sc = pc.scene(**pc.PYRAMID_SCENE)
    args = (_dev(sc["depth"], gpu)[:, None], _dev(sc["k"], gpu), _dev(sc["tgt"], gpu), _dev(sc["src"], gpu))
    pose, m, info = nconv_amd.estimate_pose(*args, levels=3, iters=8, huber=0.0, return_info=True)
    lvs = nconv_amd.pose.pyramid(*args, args[1], 3)
    host = [dict(depth=l["depth"][:, 0].cpu().numpy(), k=l["k"].cpu().numpy(), tgt=l["tgt"].cpu().numpy(),
                 src=l["src"].cpu().numpy(), k_src=l["k_src"].cpu().numpy(), mask=None) for l in lvs]
    want = pc.align(host, iters=8)
    assert info["cost"].cpu().numpy().tobytes() == want["cost"].tobytes()
    assert pose.cpu().numpy().tobytes() == want["pose"].tobytes() and m.cpu().numpy().tobytes() == want["m"].tobytes()
    err = pc.pose_error(info["state"][0].cpu().numpy(), sc["true"])[0]
    assert err < pc.pose_error(np.eye(3, 4), sc["true"])[0] / 10


def test_graph_capture_and_refill(nconv_amd, gpu, scene_run):
    sc, _, want, args, (pose, m, info) = scene_run
    est = nconv_amd.PoseEstimator((48, 64), B=2, C=1, levels=1, iters=8, huber=0.0, device=gpu)
    static = [a.clone() for a in args]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        est(*static)                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_pose, out_m = est(*static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_pose, pose) and torch.equal(out_m, m) and torch.equal(est.info["cost"], info["cost"])
    # refill in place: the two images swapped
    for t in (static[0], static[2], static[3]):
        t.copy_(t.flip(0).clone())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_pose, pose.flip(0)) and torch.equal(out_m, m.flip(0))
    assert torch.equal(est.info["cost"], info["cost"].flip(1))


def test_estimated_m_in_the_photometric_loss(nconv_amd, gpu, scene_run):
    sc, true, _, args, (pose, m, _) = scene_run
    bound = pc.load_bound()
    for b, name in enumerate(("small", "large")):
        z = _dev(sc["z_dense"][b:b + 1], gpu)[:, None]
        one = (z, args[1], args[2][b:b + 1], args[3][b:b + 1])
        loss = lambda mm: float(nconv_amd.photometric_loss(*one, mm))  # noqa: E731
        eye = torch.eye(3, 4, dtype=torch.float64, device=gpu)
        l_est = loss(m[b:b + 1].contiguous())
        l_eye = loss(nconv_amd.warp_projection(args[1], eye))
        l_true = loss(nconv_amd.warp_projection(args[1], _dev(true[b], gpu)))
        print(name, "estimated", l_est, "identity", l_eye, "true", l_true)
        assert l_est < l_eye
        assert l_est <= bound[name]["photo_factor"] * l_true


def test_prefetch_stage(nconv_amd, gpu, scene_run):
    sc, _, _, args, (pose, m, _) = scene_run
    stage = nconv_amd.EstimatePose(levels=1, iters=8, huber=0.0)
    batch = {"depth": args[0], "k": args[1], "rgb": args[2], "rgb_near": args[3], "gt": args[0]}
    out = stage(batch)
    assert tuple(out["pose"].shape) == (2, 3, 4) and tuple(out["m"].shape) == (2, 3, 4)
    assert torch.equal(out["pose"], pose) and torch.equal(out["m"], m)
    assert out["gt"] is batch["gt"] and "pose" not in batch
    plain = {"depth": args[0], "k": args[1], "rgb": args[2]}
    assert stage(plain) is plain
