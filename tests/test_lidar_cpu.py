"""CPU: the numpy reference of the LiDAR projection against float64 and its invariants (empty pixels,
depth = c[index], row permutations, duplicated rows); the round trip through the numpy back-projection;
kitti_projection against a hand-written product; read_velodyne_bin; the entry points of ABI 27 are
exported, declared and bound with the C struct's layout; every malformed call fails on the host with
-22 before any launch; lidar.* refuse malformed arguments and CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import host_harness
import lidar_cases as LC
import pointcloud_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
NEW = ("nconv_lidar_project_workspace_bytes", "nconv_lidar_project")


# ---- the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,rows", [(37, 71, 4000), (352, 1216, 120000)])
def test_reference_against_float64(H, W, rows):
    """The float32 reference against the same formulas in float64 on the float32 inputs, camera depth
    in [2, 80] m and gates at 5 and 60 m. A point takes part when its float64 u and v are farther than
    2^-6 from a half-integer (where rint switches pixel; the image edges -0.5, W - 0.5 are
    half-integers) and its c farther than 1e-5 c from a gate. The band takes 2 * 2^-6 of every unit
    interval of u and of v, about 6 % of uniformly placed points: the excluded share is capped at 10 %
    of the in-image points. Outside the band the pixel and the validity must be identical; u's fp32
    error is a few 2^-24 |u| < 1e-3 pixel, far inside 2^-6. Depths agree to 4 ulp."""
    rng = np.random.default_rng(H)
    B, z_min, z_max = 2, 5.0, 60.0
    pts, off, m, _ = LC.scan(rng, B, H, W, rows)
    img, _, _, c32, u32, v32 = LC.project_terms(pts, off, m, np.float32)
    _, _, _, c64, u64, v64 = LC.project_terms(pts, off, m, np.float64)
    ok32, pix32 = LC.valid_pixels(img, c32, u32, v32, B, H, W, z_min, z_max)
    ok64, pix64 = LC.valid_pixels(img, c64, u64, v64, B, H, W, z_min, z_max)
    in_image = (c64 > 0) & (np.rint(u64) >= 0) & (np.rint(u64) <= W - 1) & (np.rint(v64) >= 0) & (np.rint(v64) <= H - 1)
    assert in_image.sum() > 0.7 * len(pts)
    half = lambda t: np.abs(t - np.floor(t) - 0.5)  # distance to the nearest half-integer
    clear = (half(u64) > 2.0 ** -6) & (half(v64) > 2.0 ** -6)
    clear &= (np.abs(c64 - z_min) > 1e-5 * np.abs(c64)) & (np.abs(c64 - z_max) > 1e-5 * np.abs(c64))
    excluded = (in_image & ~clear).sum() / in_image.sum()
    print(f"excluded share of the in-image points: {excluded:.4f}")
    assert excluded <= 0.10
    assert np.array_equal(ok32[clear], ok64[clear]) and np.array_equal(pix32[clear], pix64[clear])
    assert ok64[clear].sum() > 0.3 * len(pts)
    both = ok32 & ok64
    ulps = np.abs(c32[both].astype(np.float64) - c64[both]) / np.spacing(c32[both]).astype(np.float64)
    print(f"largest depth error: {ulps.max():.3f} ulp")
    assert (ulps <= 4.0).all()


def _small(seed=1, B=3, H=9, W=13, rows=700, **kw):
    rng = np.random.default_rng(seed)
    pts, off, m, _ = LC.scan(rng, B, H, W, rows, **kw)
    return rng, pts, off, m, (H, W)


def test_reference_empty_pixels_and_winner():
    _, pts, off, m, size = _small(rows=60)
    r = LC.project_ref(pts, off, m, size)
    d, ix = r["depth"][:, 0], r["index"]
    assert (ix >= 0).any() and (ix < 0).any()
    assert (d[ix < 0].view(np.uint32) == 0).all() and (ix[ix < 0] == -1).all()
    hit = ix >= 0
    assert np.array_equal(d[hit].view(np.uint32), r["c"][ix[hit]].view(np.uint32))
    # the winner is a valid row of its own image and pixel, and no valid row of the pixel is nearer
    assert np.array_equal(r["pix"][ix[hit]], np.flatnonzero(hit.reshape(-1)))
    valid = r["pix"] >= 0
    assert (r["c"][valid] >= d.reshape(-1)[r["pix"][valid]]).all()


def test_reference_known_values():
    # [K | 0] with fx = fy = 2, cx = 1.5, cy = 0.5: u = 2 x / z + 1.5, v = 2 y / z + 0.5
    m = np.array([[2.0, 0.0, 1.5, 0.0], [0.0, 2.0, 0.5, 0.0], [0.0, 0.0, 1.0, 0.0]], dtype=np.float32)
    pts = np.array([[0.0, 0.0, 4.0],     # u = 1.5 -> 2 (ties to even), v = 0.5 -> 0
                    [0.0, 0.0, 2.0],     # the same pixel, nearer
                    [-2.0, 1.0, 4.0],    # u = 0.5 -> 0, v = 1.0
                    [0.0, 0.0, -1.0],    # behind
                    [np.nan, 0.0, 3.0],
                    [4.0, 0.0, 4.0]],    # u = 3.5 -> 4: outside W = 4
                   dtype=np.float32)
    r = LC.project_ref(pts, [0, 6], m, (2, 4))
    assert r["depth"][0, 0].tolist() == [[0.0, 0.0, 2.0, 0.0], [4.0, 0.0, 0.0, 0.0]]
    assert r["index"][0].tolist() == [[-1, -1, 1, -1], [2, -1, -1, -1]]
    # z_min excluded, z_max included
    r = LC.project_ref(pts, [0, 6], m, (2, 4), z_min=2.0, z_max=4.0)
    assert r["index"][0].tolist() == [[-1, -1, 0, -1], [2, -1, -1, -1]]
    # rows outside [offsets[0], offsets[B]) are ignored
    r = LC.project_ref(pts, [1, 1, 2], m, (2, 4))
    assert r["index"].tolist() == [[[-1] * 4] * 2, [[-1, -1, 1, -1], [-1] * 4]]


def test_reference_row_permutations():
    rng, pts, off, m, size = _small(seed=2)
    r = LC.project_ref(pts, off, m, size)
    # within an image: depth unchanged, indices map back to the same winners unless c ties bit for bit
    perm = np.concatenate([off[b] + rng.permutation(off[b + 1] - off[b]) for b in range(len(off) - 1)])
    p = LC.project_ref(pts[perm], off, m, size)
    assert np.array_equal(p["depth"].view(np.uint32), r["depth"].view(np.uint32))
    hit = r["index"] >= 0
    assert np.array_equal(p["index"] >= 0, hit)
    back = perm[p["index"][hit]]
    same_c = r["c"][back].view(np.uint32) == r["c"][r["index"][hit]].view(np.uint32)
    assert same_c.all() and (back == r["index"][hit]).mean() > 0.99
    # one image, an arbitrary permutation of all rows: the depth plane is unchanged
    one = [0, len(pts)]
    perm = rng.permutation(len(pts))
    assert np.array_equal(LC.project_ref(pts[perm], one, m[0], size)["depth"].view(np.uint32),
                          LC.project_ref(pts, one, m[0], size)["depth"].view(np.uint32))


def test_reference_duplicated_row_resolves_to_the_smaller_row():
    _, pts, off, m, size = _small(seed=3, B=1, rows=400)
    r = LC.project_ref(pts, off, m, size)
    winners = r["index"][r["index"] >= 0]
    w = int(winners[len(winners) // 2])
    for at in (0, w, len(pts)):  # a copy of the winner before, at and after it
        dup = np.insert(pts, at, pts[w], axis=0)
        d = LC.project_ref(dup, [0, len(dup)], m, size)
        first = min(at, w)  # the copy sits at `at`; the original at w, or w + 1 when the copy precedes it
        assert np.array_equal(d["depth"].view(np.uint32), r["depth"].view(np.uint32))
        assert d["index"].reshape(-1)[r["pix"][w]] == first


def test_round_trip_through_backproject():
    """The numpy back-projection, then the projection with [K | 0], reproduces the depth plane exactly
    at valid pixels and gives 0 elsewhere: u = (x fx + cx z) / z with x = (j - cx) z / fx lands within a
    few 2^-24 j of j, and the one point of a pixel has c = z exactly (z * 1 + 0)."""
    rng = np.random.default_rng(4)
    B, H, W = 2, 37, 71
    z = PC.depth_values(rng, B, H, W, "p50")
    k = np.zeros((B, 3, 3), dtype=np.float32)
    k[:, 0, 0], k[:, 1, 1] = rng.uniform(40, 60, B), rng.uniform(40, 60, B)
    k[:, 0, 2], k[:, 1, 2], k[:, 2, 2] = W / 2 + rng.uniform(0.05, 0.95, B), H / 2 + rng.uniform(0.05, 0.95, B), 1.0
    pc = PC.points_ref(z, k)
    m = np.concatenate([k, np.zeros((B, 3, 1), dtype=np.float32)], axis=2)
    r = LC.project_ref(pc["xyz"], pc["offsets"], m, (H, W))
    valid = PC.valid_ref(z)
    want = np.where(valid, z, np.float32(0))
    assert valid.sum() > 0.3 * z.size and np.array_equal(r["depth"][:, 0].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(r["index"].reshape(-1)[pc["index"]], np.arange(len(pc["index"])))


# ---- host helpers ----------------------------------------------------------------------------------
def _write_calib(tmp_path, rng):
    p = {n: rng.uniform(-1, 1, 12) * [700, 1, 600, 50, 1, 700, 200, 1, 0.01, 0.01, 1, 0.01] for n in range(4)}
    rect = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    T = rng.uniform(-0.5, 0.5, 3)
    fmt = lambda v: " ".join(f"{x:.12e}" for x in np.ravel(v))
    c2c, v2c = tmp_path / "calib_cam_to_cam.txt", tmp_path / "calib_velo_to_cam.txt"
    lines = ["calib_time: 09-Jan-2012 13:57:47", f"R_rect_00: {fmt(rect)}"] + [f"P_rect_0{n}: {fmt(p[n])}" for n in range(4)]
    c2c.write_text("\n".join(lines) + "\n")
    v2c.write_text(f"calib_time: 15-Mar-2012 11:37:16\nR: {fmt(R)}\nT: {fmt(T)}\ndelta_f: 0.0 0.0\n")
    rt = lambda s: np.array([float(x) for x in s.split()])  # the values as the files carry them
    return str(c2c), str(v2c), {n: rt(fmt(p[n])).reshape(3, 4) for n in p}, rt(fmt(rect)).reshape(3, 3), \
        rt(fmt(R)).reshape(3, 3), rt(fmt(T))


@pytest.mark.parametrize("cam,top,left", [(2, 0, 0), (3, 0, 0), (2, 23, 5), (0, 96, 0)])
def test_kitti_projection(nconv_amd, tmp_path, cam, top, left):
    c2c, v2c, P, rect, R, T = _write_calib(tmp_path, np.random.default_rng(5))
    want = np.zeros((3, 4))
    for i in range(3):          # P . [rect | 0; 0 1] . [R | T; 0 1], written out entry by entry
        for j in range(4):
            for a in range(3):
                pr = sum(P[cam][i, q] * rect[q, a] for q in range(3))
                want[i, j] += pr * (R[a, j] if j < 3 else T[a])
            if j == 3:
                want[i, j] += P[cam][i, 3]
    want[0], want[1] = want[0] - left * want[2], want[1] - top * want[2]
    kw = {} if (top, left) == (0, 0) else dict(crop_top=top, crop_left=left)
    got = nconv_amd.kitti_projection(c2c, v2c, cam=cam, **kw) if cam != 2 else nconv_amd.kitti_projection(c2c, v2c, **kw)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    # float64 products in another order: agreement to 1e-12 relative to the row's scale, then one fp32 rounding
    assert np.allclose(got, want.astype(np.float32), rtol=0, atol=float(np.abs(want).max()) * 2.0 ** -22)
    g64 = nconv_amd.lidar.kitti_projection(c2c, v2c, cam=cam, crop_top=top, crop_left=left)
    assert np.array_equal(g64, got)
    # a pixel of the full image is the crop's pixel shifted by the crop's corner
    x = np.array([1.0, 2.0, 3.0, 1.0])
    full = nconv_amd.kitti_projection(c2c, v2c, cam=cam).astype(np.float64) @ x
    crop = got.astype(np.float64) @ x
    assert np.allclose([crop[0] / crop[2], crop[1] / crop[2]], [full[0] / full[2] - left, full[1] / full[2] - top],
                       rtol=0, atol=1e-3)


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_read_velodyne_bin_round_trip(nconv_amd, tmp_path, n):
    a = np.random.default_rng(n).normal(size=(n, 4)).astype(np.float32)
    p = str(tmp_path / "0000000000.bin")
    a.astype("<f4").tofile(p)
    got = nconv_amd.read_velodyne_bin(p)
    assert got.dtype == np.float32 and got.shape == (n, 4) and np.array_equal(got.view(np.uint32), a.view(np.uint32))
    with open(p, "ab") as fh:
        fh.write(b"\0" * 4)
    with pytest.raises(ValueError, match="4-float"):
        nconv_amd.read_velodyne_bin(p)


def test_projection_from_k(nconv_amd):
    k = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    for q in (k, k[0]):
        got = nconv_amd.projection_from_k(q)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == q.shape[:-1] + (4,)
        assert np.array_equal(got[..., :3], q) and (got[..., 3] == 0).all()
        t = nconv_amd.projection_from_k(torch.from_numpy(q))
        assert torch.is_tensor(t) and t.is_contiguous() and np.array_equal(t.numpy(), got)
    with pytest.raises(ValueError, match="k must be"):
        nconv_amd.projection_from_k(np.zeros((3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="k must be"):
        nconv_amd.projection_from_k(torch.zeros(4, 3))


# ---- ABI -------------------------------------------------------------------------------------------
def test_entry_points_exported_and_declared(nconv_amd):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", src, re.M))
    lib = nconv_amd._lib.lib()
    for name in NEW:
        assert name in declared and name in nconv_amd._lib.EXPORTED
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    v = int(re.search(r"#define NCONV_ABI_VERSION (\d+)", src).group(1))
    assert lib.nconv_abi_version() == v == nconv_amd._lib.ABI_VERSION == 27


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "lidar_host")


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    S = nconv_amd._lib.NconvLidarProject
    want = host_harness.ctypes_layout(S, "nconv_lidar_project")
    c = {k: v for k, v in host_report.items() if k.startswith("nconv_lidar_project")}
    assert len(c) == 12 and c == want
    assert host_report["desc_typedef"] == ctypes.sizeof(S)


HOST_REJECTS = {
    "null_descriptor": "null descriptor", "null_points": "null points", "null_offsets": "null offsets or m",
    "null_m": "null offsets or m", "null_depth": "null depth", "B_zero": "non-positive", "H_zero": "non-positive",
    "W_negative": "non-positive", "too_many_pixels": "below 2^31", "n_rows_negative": "n_rows",
    "n_rows_2_31": "n_rows", "point_stride_2": "point_stride", "z_min_negative": "z_min", "z_min_nan": "z_min",
    "z_max_below_z_min": "z_max < z_min", "workspace_null": "workspace too small",
    "workspace_short": "workspace too small", "workspace_misaligned": "8-byte aligned",
    "points_misaligned": "4-byte aligned", "depth_misaligned": "4-byte aligned", "index_misaligned": "4-byte aligned",
}


def test_host_calls(host_report):
    assert host_report["abi"] == [27, 27]
    got = {k[3:]: v for k, v in host_report.items() if k.startswith("rc_")}
    assert set(got) == set(HOST_REJECTS)
    for key, msg in HOST_REJECTS.items():
        rc, err = got[key]
        assert rc == -22 and msg in err, (key, rc, err)
    assert host_report["workspace"] == [0, 8 * 8 * 352 * 1216, 0, 0, 0]


# ---- host validation through ctypes ----------------------------------------------------------------
FAKE = {n: 0x10000 * (q + 1) for q, n in enumerate(("points", "depth", "index", "ws", "offsets", "m"))}


def _desc(L, **kw):
    d = L.NconvLidarProject()
    d.B, d.H, d.W, d.point_stride = 2, 4, 8, 4
    d.points, d.n_rows, d.offsets, d.m, d.m_image_stride = FAKE["points"], 100, FAKE["offsets"], FAKE["m"], 12
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("bad,msg", [
    (dict(points=None), "null points"),
    (dict(offsets=None), "null offsets or m"),
    (dict(m=None), "null offsets or m"),
    (dict(B=0), "non-positive"), (dict(H=-3), "non-positive"), (dict(W=0), "non-positive"),
    (dict(B=1 << 15, H=1 << 8, W=1 << 8), "below 2^31"),
    (dict(n_rows=-1), "n_rows"), (dict(n_rows=1 << 31), "n_rows"),
    (dict(point_stride=2), "point_stride"), (dict(point_stride=0), "point_stride"),
    (dict(point_stride=(1 << 20) + 1), "point_stride"),
    (dict(m_image_stride=-12), "m image stride"),
    (dict(z_min=-0.5), "z_min"), (dict(z_min=float("nan")), "z_min"),
    (dict(z_min=2.0, z_max=1.0), "z_max < z_min"), (dict(z_max=float("nan")), "z_max < z_min"),
    (dict(z_max=-1.0), "z_max < z_min"),
    (dict(points=FAKE["points"] + 2), "4-byte aligned"), (dict(offsets=FAKE["offsets"] + 1), "4-byte aligned"),
    (dict(m=FAKE["m"] + 2), "4-byte aligned"),
])
def test_call_rejects_bad_descriptors(nconv_amd, bad, msg):
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L, **bad)
    for index, ws, n in ((None, None, 0), (FAKE["index"], FAKE["ws"], 1 << 20)):
        assert lib.nconv_lidar_project(ctypes.byref(d), FAKE["depth"], index, ws, n, None) == -22
        assert msg in lib.nconv_last_error().decode()


def test_call_rejects_bad_arguments(nconv_amd):
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L)
    need = lib.nconv_lidar_project_workspace_bytes(2, 4, 8, 1)
    assert need == 8 * 2 * 4 * 8 and lib.nconv_lidar_project_workspace_bytes(2, 4, 8, 0) == 0
    call = lambda depth=FAKE["depth"], index=FAKE["index"], ws=FAKE["ws"], n=need: \
        lib.nconv_lidar_project(ctypes.byref(d), depth, index, ws, n, None)
    assert lib.nconv_lidar_project(None, FAKE["depth"], None, None, 0, None) == -22
    assert "null descriptor" in lib.nconv_last_error().decode()
    for kw, msg in ((dict(depth=None), "null depth"), (dict(depth=None, index=None), "null depth"),
                    (dict(ws=None), "workspace too small"), (dict(n=need - 1), "workspace too small"),
                    (dict(n=0), "workspace too small"), (dict(ws=FAKE["ws"] + 4), "8-byte aligned"),
                    (dict(depth=FAKE["depth"] + 2), "4-byte aligned"), (dict(index=FAKE["index"] + 1), "4-byte aligned")):
        assert call(**kw) == -22, msg
        assert msg in lib.nconv_last_error().decode(), msg
    for B, H, W in ((0, 4, 8), (2, -1, 8), (2, 4, 0), (1 << 15, 1 << 8, 1 << 8)):
        assert lib.nconv_lidar_project_workspace_bytes(B, H, W, 1) == 0
        assert lib.nconv_lidar_project_workspace_bytes(B, H, W, 0) == 0


# ---- Python argument checks ------------------------------------------------------------------------
def test_lidar_refuses_cpu_tensors_and_bad_arguments(nconv_amd):
    Ld = nconv_amd.lidar
    assert nconv_amd.project_points is Ld.project_points and nconv_amd.LidarProjector is Ld.LidarProjector
    assert nconv_amd.kitti_projection is Ld.kitti_projection and nconv_amd.read_velodyne_bin is Ld.read_velodyne_bin
    assert nconv_amd.projection_from_k is Ld.projection_from_k
    pts, m, off = torch.ones(10, 4), torch.zeros(3, 4), torch.tensor([0, 4, 10], dtype=torch.int32)
    for fn in (Ld.project_points, lambda p, o, q, s, **kw: Ld.LidarProjector(s)(p, o, q, **kw)):
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            fn(pts, off, m, (4, 8))
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            fn(pts[:, :3], None, m, (4, 8))
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            fn(pts, [0, 3, 3, 10], torch.zeros(3, 3, 4), (4, 8))
        with pytest.raises(TypeError, match="points"):
            fn(pts.double(), off, m, (4, 8))
        with pytest.raises(TypeError, match="points must be a tensor"):
            fn(np.ones((10, 4), dtype=np.float32), off, m, (4, 8))
        with pytest.raises(ValueError, match="points must be"):
            fn(pts[:, :2], off, m, (4, 8))
        with pytest.raises(ValueError, match="points must be"):
            fn(pts[0], off, m, (4, 8))
        with pytest.raises(ValueError, match="unit inner stride"):
            fn(torch.ones(10, 8)[:, ::2], off, m, (4, 8))
        with pytest.raises(ValueError, match="rows overlap"):
            fn(torch.ones(1, 4).expand(10, 4), off, m, (4, 8))
        with pytest.raises(TypeError, match="offsets"):
            fn(pts, off.long(), m, (4, 8))
        with pytest.raises(ValueError, match="offsets"):
            fn(pts, off[:1], m, (4, 8))
        with pytest.raises(ValueError, match="non-decreasing"):
            fn(pts, [0, 5, 4], m, (4, 8))
        with pytest.raises(ValueError, match="non-decreasing"):
            fn(pts, [0, 11], m, (4, 8))
        with pytest.raises(TypeError, match="m"):
            fn(pts, off, m.double(), (4, 8))
        with pytest.raises(ValueError, match="m must be"):
            fn(pts, off, torch.zeros(3, 3), (4, 8))
        with pytest.raises(ValueError, match="m must be"):
            fn(pts, off, torch.zeros(3, 3, 4), (4, 8))
        with pytest.raises(ValueError, match="not contiguous"):
            fn(pts, off, torch.zeros(3, 8)[:, ::2], (4, 8))
        with pytest.raises(ValueError, match="z_min"):
            fn(pts, off, m, (4, 8), z_min=-1.0)
        with pytest.raises(ValueError, match="z_max"):
            fn(pts, off, m, (4, 8), z_min=2.0, z_max=1.0)
    with pytest.raises(TypeError, match="size"):
        Ld.project_points(pts, off, m, 8)
    with pytest.raises(ValueError, match="not positive"):
        Ld.project_points(pts, off, m, (0, 8))
    with pytest.raises(ValueError, match="not positive"):
        Ld.LidarProjector((4, -8))
    with pytest.raises(ValueError, match="too large"):
        Ld.workspace_bytes(1 << 15, 1 << 8, 1 << 8)
    assert Ld.workspace_bytes(2, 4, 8) == 8 * 64 and Ld.workspace_bytes(2, 4, 8, with_index=False) == 0
