"""GPU: lidar.project_points / LidarProjector (nconv_lidar_project, csrc/lidar_project.hip) against
the numpy reference of tests/lidar_cases.py, bit for bit in depth and index: the sweep over sizes, row
strides, base alignments and matrix forms; image boundaries inside a wave; the validity rules at their
edges; ties; stale state; hipGraph capture; the round trip through backproject; the plane fed to DNET;
the argument errors that need a device."""
import numpy as np
import pytest
import torch

import lidar_cases as LC
import pointcloud_cases as PC

pytestmark = pytest.mark.gpu

GUARD_F, GUARD_I = -7.0, -77


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _points_tensor(gpu, pts, shifted=False):
    """pts (N, C) on the device; shifted: at one float past an allocation's base, so never 16-byte
    aligned."""
    flat = torch.full((pts.size + 1,), float("nan"), device=gpu)
    v = flat[1:] if shifted else flat[:-1]
    v = v.view(pts.shape)
    v.copy_(torch.from_numpy(pts))
    assert (v.data_ptr() % 16 != 0) == shifted or pts.size == 0
    return v


def _guarded(gpu, shape, dtype, guard, lead):
    """A contiguous tensor of `shape` `lead` elements into a larger allocation filled with `guard`."""
    n = int(np.prod(shape))
    whole = torch.full((n + lead + 5,), guard, dtype=dtype, device=gpu)
    return whole, whole[lead:lead + n].view(shape)


def _run(nconv_amd, gpu, pts, off, m, size, *, index=True, shifted=False, **kw):
    """(depth (B, 1, H, W), index (B, H, W) or None) as numpy. shifted: points, depth and index one
    element past a 16-byte boundary and the workspace 8 bytes past one; guards around the outputs
    must survive."""
    Ld = nconv_amd.lidar
    H, W = size
    B = len(off) - 1
    lead = 1 if shifted else 0
    wd, depth = _guarded(gpu, (B, 1, H, W), torch.float32, GUARD_F, lead)
    out = {"depth": depth}
    if index:
        wi, out["index"] = _guarded(gpu, (B, H, W), torch.int32, GUARD_I, lead)
        n = Ld.workspace_bytes(B, H, W)
        ww, out["workspace"] = _guarded(gpu, (n,), torch.uint8, 0x5A, 8 * lead)
    t_pts = _points_tensor(gpu, pts, shifted)
    t_off = torch.from_numpy(np.asarray(off, dtype=np.int32)).to(gpu)
    got = Ld.project_points(t_pts, t_off, torch.from_numpy(np.ascontiguousarray(m)).to(gpu), size,
                            return_index=index, out=out, **kw)
    torch.cuda.synchronize()
    npx = B * H * W
    assert (got[0] if index else got) is depth
    assert bool((wd[:lead] == GUARD_F).all()) and bool((wd[lead + npx:] == GUARD_F).all())
    if index:
        assert got[1] is out["index"]
        assert bool((wi[:lead] == GUARD_I).all()) and bool((wi[lead + npx:] == GUARD_I).all())
        assert bool((ww[:8 * lead] == 0x5A).all()) and bool((ww[8 * lead + 8 * npx:] == 0x5A).all())
    return depth.cpu().numpy(), (out["index"].cpu().numpy() if index else None)


def _check(nconv_amd, gpu, pts, off, m, size, ref=None, *, forms=((True, False), (False, False)), **kw):
    """Every (index, shifted) form in `forms` equals the reference bit for bit; returns the reference."""
    if ref is None:
        ref = LC.project_ref(pts, off, m, size, **kw)
    for index, shifted in forms:
        d, ix = _run(nconv_amd, gpu, pts, off, m, size, index=index, shifted=shifted, **kw)
        assert np.array_equal(_bits(d), _bits(ref["depth"])), (index, shifted)
        if index:
            assert np.array_equal(ix, ref["index"]), (index, shifted)
    return ref


ALL_FORMS = ((True, False), (False, False), (True, True), (False, True))


# ---- the sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 4, 5])
@pytest.mark.parametrize("B,H,W,rows", LC.SWEEP + ((1, 2, 3, 2000),))
def test_sweep(nconv_amd, gpu, B, H, W, rows, stride):
    """Sizes x row strides; per case the shared and the per-image matrix, with and without index, the
    aligned and the shifted bases (stride 4 aligned is the 128-bit row path, everything else the
    element path)."""
    rng = np.random.default_rng(1000 * H + 10 * W + stride)
    for shared in (False, True):
        pts, off, m, _ = LC.scan(rng, B, H, W, rows, stride=stride, shared_m=shared)
        ref = _check(nconv_amd, gpu, pts, off, m, (H, W), forms=ALL_FORMS)
        filled = (ref["index"] >= 0).mean()
        assert filled > 0.9 if H * W <= 35 else filled > 0.3
        if rows == 2000:  # hundreds of collisions per pixel
            assert (ref["pix"] >= 0).sum() > 200 * H * W


def test_many_images_search_offsets_in_global_memory(nconv_amd, gpu):
    """B + 1 above the 1024 entries staged in LDS: the binary search reads offsets from global
    memory. Random cut points, empty images among them; per-image matrices that differ by a power of
    two (the same pixels, depths scaled exactly)."""
    rng = np.random.default_rng(7)
    B, H, W, n = 1100, 2, 3, 6000
    cam = LC.camera(rng, H, W)
    pts = np.zeros((n, 4), dtype=np.float32)
    pts[:, :3] = LC.rows_for(rng, cam, H, W, n).astype(np.float32)
    off = np.sort(np.concatenate([[0, n], rng.integers(0, n - 500, B - 1)])).astype(np.int32)
    assert (np.diff(off) == 0).any() and (np.diff(off) > 64).any()
    scale = (2.0 ** rng.integers(-2, 3, B)).astype(np.float32)
    m = cam["m"][None] * scale[:, None, None]
    ref = _check(nconv_amd, gpu, pts, off, m, (H, W))
    assert (ref["index"] >= 0).mean() > 0.3
    _check(nconv_amd, gpu, pts, off, cam["m"], (H, W))


# ---- image boundaries inside a wave ------------------------------------------------------------------
@pytest.mark.parametrize("off,n_rows", [([0, 1, 1, 66, 300], 300), ([0, 1, 1, 66, 300], 310), ([2, 2, 70, 300], 321),
                                        ([0, 0, 0, 5], 5), ([0, 64, 128, 129], 200)])
def test_image_boundaries_inside_a_wave(nconv_amd, gpu, off, n_rows):
    """Images that begin and end inside a wave, an empty image in the middle, rows below offsets[0],
    and rows from offsets[B] on, which hold NaN or a point that would win its pixel: not read into the
    result."""
    rng = np.random.default_rng(n_rows + len(off))
    B, H, W = len(off) - 1, 5, 7
    cams = [LC.camera(rng, H, W) for _ in range(B)]
    img = LC.image_of_rows(off, n_rows)
    pts = np.zeros((n_rows, 4), dtype=np.float32)
    for b in range(B):
        rows = np.flatnonzero(img == b)
        pts[rows, :3] = LC.rows_for(rng, cams[b], H, W, len(rows)).astype(np.float32)
    outside = np.flatnonzero((img < 0) | (img >= B))
    # ignored rows: near points of the last / first camera (they would win), NaN at every other one
    near = cams[-1 if len(outside) and outside[0] >= off[-1] else 0]
    pts[outside, :3] = LC.rows_for(rng, near, H, W, len(outside), inside=1.0, c_lo=0.5, c_hi=1.0).astype(np.float32)
    pts[outside[::2]] = np.nan
    m = np.stack([c["m"] for c in cams])
    ref = _check(nconv_amd, gpu, pts, off, m, (H, W), forms=ALL_FORMS)
    won = ref["index"][ref["index"] >= 0]
    assert len(won) and not np.isin(won, outside).any()
    for b in range(B):
        if off[b + 1] == off[b]:
            assert not (ref["index"][b] >= 0).any()
        if off[b + 1] - off[b] >= 5:
            assert (ref["index"][b] >= 0).any()


def test_no_rows(nconv_amd, gpu):
    Ld = nconv_amd.lidar
    m = torch.from_numpy(LC.camera(np.random.default_rng(0), 5, 7)["m"]).to(gpu)
    for pts in (torch.empty(0, 4, device=gpu), torch.empty(0, 3, device=gpu)):
        out = {"depth": torch.full((2, 1, 5, 7), GUARD_F, device=gpu),
               "index": torch.full((2, 5, 7), GUARD_I, dtype=torch.int32, device=gpu)}
        d, ix = Ld.project_points(pts, [0, 0, 0], m, (5, 7), return_index=True, out=out)
        assert bool((_as_int(d) == 0).all()) and bool((ix == -1).all())
        d = Ld.project_points(pts, None, m, (5, 7))
        assert d.shape == (1, 1, 5, 7) and bool((_as_int(d) == 0).all())


def _as_int(t):
    return t.view(torch.int32)


# ---- validity ------------------------------------------------------------------------------------------
def test_validity_edges(nconv_amd, gpu):
    """m = diag(2, 4, 1) | 0: u = 2 x / z, v = 4 y / z, c = z, exact for the power-of-two inputs used.
    z_min = 2 (excluded), z_max = 8 (included). u exactly -0.5, 0.5, W - 1.5, W - 0.5 and the same for
    v: ties to even at the image edge (-0.5 -> -0 is column 0, W - 0.5 -> W is outside). Rows with NaN,
    +-inf and 1e30 coordinates, c <= 0."""
    H, W = 6, 8
    m = np.array([[2.0, 0, 0, 0], [0, 4.0, 0, 0], [0, 0, 1.0, 0]], dtype=np.float32)
    rows, expect = [], {}

    def add(u, v, c, pixel):
        """the point that projects to exactly (u, v) at depth c; pixel: (i, j) it must win, or None"""
        rows.append([u * c / 2.0, v * c / 4.0, c])
        if pixel is not None:
            expect[pixel] = len(rows) - 1

    # each expected winner on a pixel of its own, at depth 4
    add(-0.5, 1.0, 4.0, (1, 0))          # rint(-0.5) = -0: column 0
    add(0.5, 2.0, 4.0, (2, 0))           # ties to even: 0
    add(W - 1.5, 3.0, 4.0, (3, W - 2))   # 6.5 -> 6
    add(W - 0.5, 3.0, 4.0, None)         # 7.5 -> 8: outside
    add(1.0, -0.5, 4.0, (0, 1))
    add(2.0, 0.5, 4.0, (0, 2))
    add(3.0, H - 1.5, 4.0, (H - 2, 3))   # 4.5 -> 4
    add(3.0, H - 0.5, 4.0, None)         # 5.5 -> 6: outside
    add(-0.5, -0.5, 4.0, (0, 0))
    add(W - 1.0, H - 1.0, 4.0, (H - 1, W - 1))
    add(-0.75, 1.0, 4.0, None)           # -0.75 -> -1
    add(4.0, 1.0, 2.0, None)             # c == z_min: not valid
    add(4.0, 1.0, 8.0, (1, 4))           # c == z_max: valid
    add(4.0, 1.0, float(np.nextafter(np.float32(8.0), np.float32(9.0))), None)
    add(4.0, 2.0, float(np.nextafter(np.float32(2.0), np.float32(3.0))), (2, 4))
    add(4.0, 3.0, 0.0, None)
    add(4.0, 3.0, -4.0, None)
    pts = np.array(rows, dtype=np.float32)
    assert np.array_equal(pts.astype(np.float64), np.array(rows))  # every input is exact in fp32
    special = []
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for col in range(3):
            p = [2.0, 1.0, 4.0]  # u = 1, v = 1
            p[col] = bad
            special.append(p)
    special += [[1e30, 1e30, 1e30], [np.inf, np.inf, np.inf], [0.0, 0.0, 1e-40], [1e-40, 0.0, 4.0]]
    pts = np.concatenate([pts, np.array(special, dtype=np.float32)])
    off = [0, len(pts)]
    ref = _check(nconv_amd, gpu, pts, off, m, (H, W), forms=ALL_FORMS, z_min=2.0, z_max=8.0)
    want = np.full((H, W), -1, dtype=np.int32)
    for (i, j), r in expect.items():
        want[i, j] = r
    # [1e-40, 0, 4] is an ordinary point of column 0, row 0, behind the expected winner's equal depth
    assert np.array_equal(ref["index"][0], want)
    # without an upper gate the huge and the subnormal depths are valid where they land; +inf never is
    ref = _check(nconv_amd, gpu, pts, off, m, (H, W), forms=ALL_FORMS)
    c_won = ref["depth"][:, 0][ref["index"] >= 0]
    assert np.isfinite(c_won).all() and (c_won > 0).all() and (c_won == np.float32(1e30)).any()
    assert (c_won == np.float32(1e-40)).any()


# ---- ties ----------------------------------------------------------------------------------------------
def test_ties_resolve_to_the_smallest_row(nconv_amd, gpu):
    rng = np.random.default_rng(11)
    H, W = 5, 7
    cam = LC.camera(rng, H, W)
    pts = np.zeros((200, 4), dtype=np.float32)
    pts[:, :3] = LC.rows_for(rng, cam, H, W, 200, c_lo=20.0).astype(np.float32)
    # one row 64 times, rows 32 .. 95: across the first two waves; nearer than everything else
    near = LC.rows_for(rng, cam, H, W, 1, inside=1.0, c_lo=3.0, c_hi=4.0).astype(np.float32)
    pts[32:96, :3] = near
    ref = _check(nconv_amd, gpu, pts, [0, 200], cam["m"], (H, W), forms=ALL_FORMS)
    assert (ref["index"] == 32).sum() == 1 and not ((ref["index"] > 32) & (ref["index"] < 96)).any()
    # two different rows with bit-equal c on one pixel ([I | 0]: c = z; u = 3.25 and 2.75 -> column 3)
    m = np.eye(3, 4, dtype=np.float32)
    two = np.array([[100.0, 100.0, 1.0], [6.5, 2.0, 2.0], [5.5, 2.0, 2.0], [12.0, 4.0, 4.0]], dtype=np.float32)
    for order in ([0, 1, 2, 3], [0, 2, 1, 3], [3, 2, 0, 1]):
        p = two[order]
        ref = _check(nconv_amd, gpu, p, [0, 4], m, (H, W), forms=ALL_FORMS)
        first = min(order.index(1), order.index(2))
        assert ref["index"][0, 1, 3] == first and ref["depth"][0, 0, 1, 3] == 2.0
        assert (ref["index"] >= 0).sum() == 1


# ---- stale state ---------------------------------------------------------------------------------------
def test_second_call_carries_nothing_of_the_first(nconv_amd, gpu):
    Ld = nconv_amd.lidar
    rng = np.random.default_rng(12)
    B, H, W = 2, 9, 13
    out = {"depth": torch.empty(B, 1, H, W, device=gpu), "index": torch.empty(B, H, W, dtype=torch.int32, device=gpu),
           "workspace": torch.empty(Ld.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)}
    plain = {"depth": torch.empty(B, 1, H, W, device=gpu)}
    # a dense near scan first, then a sparse far one: every pixel of the first would win if it stayed
    for rows, c_lo, c_hi in ((3000, 2.0, 5.0), (40, 40.0, 80.0)):
        cams = [LC.camera(rng, H, W) for _ in range(B)]
        pts = np.zeros((B * rows, 4), dtype=np.float32)
        for b in range(B):
            pts[b * rows:(b + 1) * rows, :3] = LC.rows_for(rng, cams[b], H, W, rows, c_lo=c_lo, c_hi=c_hi)
        off, m = [0, rows, 2 * rows], np.stack([c["m"] for c in cams])
        ref = LC.project_ref(pts, off, m, (H, W))
        args = (torch.from_numpy(pts).to(gpu), off, torch.from_numpy(m).to(gpu), (H, W))
        d, ix = Ld.project_points(*args, return_index=True, out=out)
        d0 = Ld.project_points(*args, out=plain)
        assert d is out["depth"] and d0 is plain["depth"]
        for got in (d, d0):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref["depth"]))
        assert np.array_equal(ix.cpu().numpy(), ref["index"])
    assert (ref["index"] < 0).mean() > 0.5


# ---- hipGraph ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_index", [True, False])
def test_captured_in_a_graph(nconv_amd, gpu, with_index):
    """LidarProjector captured once and replayed on points, offsets and matrices refilled in place
    equals the reference each time: no allocation, no synchronisation, nothing kept between calls."""
    rng = np.random.default_rng(13)
    B, H, W, rows = 3, 9, 13, 500
    N = B * rows + 20

    def new():
        pts, _, m, _ = LC.scan(rng, B, H, W, rows + 20)
        pts = pts[:N]
        cuts = np.sort(rng.integers(0, B * rows, B - 1))
        off = np.concatenate([[0], cuts, [B * rows]]).astype(np.int32)  # the last 20 rows belong to no image
        return pts, off, m

    pts, off, m = new()
    s_pts, s_off, s_m = (torch.from_numpy(v).to(gpu) for v in (pts, off, m))
    proj = nconv_amd.LidarProjector((H, W), with_index=with_index)
    first = proj(s_pts, s_off, s_m)  # library loaded, outputs and workspace allocated before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = proj(s_pts, s_off, s_m)
    d, ix = res if with_index else (res, None)
    assert d is (first[0] if with_index else first)
    for _ in range(3):
        pts, off, m = new()
        s_pts.copy_(torch.from_numpy(pts))
        s_off.copy_(torch.from_numpy(off))
        s_m.copy_(torch.from_numpy(m))
        g.replay()
        torch.cuda.synchronize()
        ref = LC.project_ref(pts, off, m, (H, W))
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(ref["depth"]))
        if with_index:
            assert np.array_equal(ix.cpu().numpy(), ref["index"])


# ---- with the rest of the pipeline -------------------------------------------------------------------
def test_round_trip_through_backproject_on_the_device(nconv_amd, gpu):
    rng = np.random.default_rng(14)
    B, H, W = 2, 37, 71
    z = PC.depth_values(rng, B, H, W, "p50")
    k = np.zeros((B, 3, 3), dtype=np.float32)
    k[:, 0, 0], k[:, 1, 1] = rng.uniform(40, 60, B), rng.uniform(40, 60, B)
    k[:, 0, 2], k[:, 1, 2], k[:, 2, 2] = W / 2 + rng.uniform(0.05, 0.95, B), H / 2 + rng.uniform(0.05, 0.95, B), 1.0
    D, tk = torch.from_numpy(z).to(gpu)[:, None], torch.from_numpy(k).to(gpu)
    pc = nconv_amd.backproject(D, tk, with_index=True)
    depth, index = nconv_amd.project_points(pc.xyz, pc.offsets, nconv_amd.projection_from_k(tk), (H, W),
                                            return_index=True)
    want = np.where(PC.valid_ref(z), z, np.float32(0))
    assert np.array_equal(_bits(depth.cpu().numpy()[:, 0]), _bits(want))
    # the winner of a pixel is the point back-projected from it
    n = pc.count()
    back = pc.index[:n].cpu().numpy()
    assert np.array_equal(index.cpu().numpy().reshape(-1)[back], np.arange(n))
    assert (index.cpu().numpy() >= 0).sum() == n


def test_projected_plane_feeds_dnet(nconv_amd, gpu):
    """DNET on the projected plane is bitwise DNET on the reference plane uploaded: the planes are
    equal, so this only proves the layout is what the model takes."""
    rng = np.random.default_rng(15)
    B, H, W = 1, 16, 20
    pts, off, m, _ = LC.scan(rng, B, H, W, 60)
    ref = LC.project_ref(pts, off, m, (H, W))
    assert 0.05 < (ref["index"] >= 0).mean() < 0.9
    S = nconv_amd.project_points(torch.from_numpy(pts).to(gpu), torch.from_numpy(off).to(gpu),
                                 torch.from_numpy(m).to(gpu), (H, W))
    torch.manual_seed(0)
    net = nconv_amd.SETP1_NCONV(crop="generalized").to(gpu)
    net.train()  # one training-mode forward: EnforcePos makes the weights positive (what training produces)
    with torch.no_grad():
        net(torch.zeros(1, 1, 32, 32, device=gpu))
        net.eval()
        a = net(S)
        b = net(torch.from_numpy(ref["depth"]).to(gpu))
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ---- argument errors that need a device --------------------------------------------------------------
def test_argument_errors_on_the_device(nconv_amd, gpu):
    Ld = nconv_amd.lidar
    pts, m = torch.ones(10, 4, device=gpu), torch.zeros(3, 4, device=gpu)
    off = torch.tensor([0, 4, 10], dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        Ld.project_points(pts, off, m.cpu(), (4, 8))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        Ld.project_points(pts, off.cpu(), m, (4, 8))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        Ld.project_points(pts.cpu(), off, m, (4, 8))
    with pytest.raises(TypeError, match="out"):
        Ld.project_points(pts, off, m, (4, 8), out={"depth": torch.zeros(2, 1, 8, 4, device=gpu)})
    with pytest.raises(TypeError, match="out"):
        Ld.project_points(pts, off, m, (4, 8), out={"depth": torch.zeros(2, 1, 4, 8, dtype=torch.float64, device=gpu)})
    with pytest.raises(TypeError, match="out"):
        Ld.project_points(pts, off, m, (4, 8), return_index=True, out={"index": torch.zeros(2, 4, 8, device=gpu)})
    with pytest.raises(TypeError, match="out"):
        Ld.project_points(pts, off, m, (4, 8), return_index=True,
                          out={"workspace": torch.zeros(8, dtype=torch.uint8, device=gpu)})
    with pytest.raises(TypeError, match="out"):
        Ld.project_points(pts, off, m, (4, 8), out={"depth": torch.zeros(2, 1, 4, 16, device=gpu)[..., ::2]})
    with pytest.raises(RuntimeError, match="out"):
        Ld.project_points(pts, off, m, (4, 8), out={"depth": torch.zeros(2, 1, 4, 8)})
    if torch.cuda.device_count() > 1:
        other = torch.device("cuda:1")
        with pytest.raises(RuntimeError, match="m on"):
            Ld.project_points(pts, off, m.to(other), (4, 8))
        with pytest.raises(RuntimeError, match="offsets on"):
            Ld.project_points(pts, off.to(other), m, (4, 8))
