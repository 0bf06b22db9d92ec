"""CPU: the numpy reference of back-projection against float64 and its raster-order / offsets
invariants; write_ply round-trips through a parser written here; the entry points of ABI 26 are
exported, declared and bound with the C struct's layout; every malformed call fails on the host with
-22 before any launch; pointcloud.* refuse CPU tensors and malformed arguments;
DNET.forward_with_confidence refuses grad mode and CPU input."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import host_harness
import pointcloud_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
NEW = ("nconv_backproject_map", "nconv_backproject_workspace_bytes", "nconv_backproject_points")


# ---- the reference ---------------------------------------------------------------------------------
def test_reference_against_float64():
    """Three roundings of relative size 2^-24 give 3 * 2^-24 plus second-order terms; the bound is
    the next whole multiple, 4 * 2^-24 |x64|. cx, cy are non-integer, so j - cx is never 0."""
    rng = np.random.default_rng(0)
    B, H, W = 3, 37, 301
    z = rng.uniform(0.5, 80.0, (B, H, W)).astype(np.float32)
    k = PC.intrinsics(rng, B)
    xyz, valid = PC.map_ref(z, k)
    assert valid.all() and xyz.dtype == np.float32
    k64, z64 = k.astype(np.float64), z.astype(np.float64)
    j = np.arange(W, dtype=np.float64).reshape(1, 1, W)
    i = np.arange(H, dtype=np.float64).reshape(1, H, 1)
    x64 = (j - k64[:, 0, 2].reshape(B, 1, 1)) * z64 / k64[:, 0, 0].reshape(B, 1, 1)
    y64 = (i - k64[:, 1, 2].reshape(B, 1, 1)) * z64 / k64[:, 1, 1].reshape(B, 1, 1)
    bound = 4.0 * 2.0 ** -24
    for got, want in ((xyz[:, 0], x64), (xyz[:, 1], y64)):
        assert (np.abs(want) > 0).all()
        assert (np.abs(got.astype(np.float64) - want) <= bound * np.abs(want)).all()
    assert np.array_equal(xyz[:, 2], z)


def test_reference_known_values():
    k = np.array([[2.0, 9.0, 1.5], [9.0, 4.0, 0.5], [9.0, 9.0, 9.0]], dtype=np.float32)
    z = np.array([[[2.0, 0.0, 4.0], [np.nan, 8.0, -1.0]]], dtype=np.float32)
    r = PC.points_ref(z, k)
    assert r["offsets"].tolist() == [0, 3] and r["index"].tolist() == [0, 2, 4]
    assert r["xyz"].tolist() == [[-1.5, -0.25, 2.0], [1.0, -0.5, 4.0], [-2.0, 1.0, 8.0]]
    # z_min is excluded, z_max included; a confidence equal to conf_min passes, a NaN one does not
    c = np.array([[[0.5, 1.0, np.nan], [1.0, 0.25, 1.0]]], dtype=np.float32)
    assert PC.points_ref(z, k, z_min=2.0, z_max=8.0)["index"].tolist() == [2, 4]
    assert PC.points_ref(z, k, conf=c, conf_min=0.5)["index"].tolist() == [0]
    col = np.zeros((1, 3, 2, 3), dtype=np.float32)
    col[0, :, 0, 0] = (-3.0, 254.5, 255.5)
    col[0, :, 0, 2] = (300.0, np.nan, 2.5)
    got = PC.points_ref(z, k, color=col)["rgb"]
    assert got[:2].tolist() == [[0, 254, 255], [255, 0, 2]]
    assert PC.points_ref(z, k, color=col, reverse=True)["rgb"][:2].tolist() == [[255, 254, 0], [2, 0, 255]]


@pytest.mark.parametrize("pattern", PC.PATTERNS)
def test_reference_raster_order_and_offsets(pattern):
    rng = np.random.default_rng(len(pattern))
    B, H, W = 3, 5, 600
    zlim = dict(z_min=1.0, z_max=50.0) if pattern == "edges" else {}
    z = PC.depth_values(rng, B, H, W, pattern, **zlim)
    k = PC.intrinsics(rng, B)
    r = PC.points_ref(z, k, **zlim)
    xyz, valid = PC.map_ref(z, k, **zlim)
    off, idx = r["offsets"], r["index"]
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == valid.sum() == len(idx) == len(r["xyz"])
    assert (np.diff(idx) > 0).all()  # raster order inside an image, images in batch order
    assert np.array_equal(np.diff(off), valid.reshape(B, -1).sum(1))
    for b in range(B):
        seg = idx[off[b]:off[b + 1]]
        assert ((seg >= b * H * W) & (seg < (b + 1) * H * W)).all()
    b, rest = np.divmod(idx, H * W)
    i, j = np.divmod(rest, W)
    assert np.array_equal(r["xyz"].view(np.int32), xyz[b, :, i, j].view(np.int32))
    assert not np.isnan(r["xyz"]).any() and np.isnan(xyz.transpose(0, 2, 3, 1)[~valid]).all()
    if pattern == "none":
        assert off.tolist() == [0] * (B + 1)
    if pattern == "all":
        assert off.tolist() == [0, H * W, 2 * H * W, 3 * H * W]
    if pattern == "edges":
        assert not (z[valid] == 1.0).any() and (z[valid] == 50.0).any() and (z[~valid] == 1.0).any()


# ---- write_ply -------------------------------------------------------------------------------------
def _read_ply(path):
    """A small PLY parser: (property list [(type, name)], vertex count, payload bytes)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-2] == "end_header"
    m = re.fullmatch(r"element vertex (\d+)", lines[2])
    props = [tuple(l.split()[1:]) for l in lines[3:-2]]
    assert all(l.startswith("property ") for l in lines[3:-2])
    return props, int(m.group(1)), raw[end:]


@pytest.mark.parametrize("n", [0, 1, 257])
def test_write_ply_round_trip(tmp_path, nconv_amd, n):
    rng = np.random.default_rng(n)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.int64).astype(np.uint8)
    p = str(tmp_path / "a.ply")
    nconv_amd.write_ply(p, torch.from_numpy(xyz))
    props, count, body = _read_ply(p)
    assert props == [("float", "x"), ("float", "y"), ("float", "z")] and count == n and len(body) == 12 * n
    assert body == xyz.astype("<f4").tobytes()
    nconv_amd.write_ply(p, xyz, torch.from_numpy(rgb))
    props, count, body = _read_ply(p)
    assert props == [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"),
                     ("uchar", "blue")]
    assert count == n and len(body) == 15 * n
    for v in range(n):
        rec = struct.unpack_from("<fffBBB", body, 15 * v)
        assert rec[:3] == tuple(xyz[v].tolist()) and rec[3:] == tuple(rgb[v].tolist())
    with pytest.raises(TypeError):
        nconv_amd.write_ply(p, xyz.astype(np.float64))
    with pytest.raises(TypeError):
        nconv_amd.write_ply(p, xyz, rgb[:, :2])


# ---- ABI -------------------------------------------------------------------------------------------
def test_entry_points_exported_and_declared(nconv_amd):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", src, re.M))
    lib = nconv_amd._lib.lib()
    for name in NEW:
        assert name in declared and name in nconv_amd._lib.EXPORTED
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    v = int(re.search(r"#define NCONV_ABI_VERSION (\d+)", src).group(1))
    assert lib.nconv_abi_version() == v == nconv_amd._lib.ABI_VERSION and v >= 26
    # the header says which entries of K are read
    assert "NOT read" in src


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "pointcloud_host")


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    S = nconv_amd._lib.NconvBackproject
    want = host_harness.ctypes_layout(S, "nconv_backproject")
    c = {k: v for k, v in host_report.items() if k.startswith("nconv_backproject")}
    assert len(c) == 21 and c == want


def test_host_calls_and_enum(nconv_amd, host_report):
    L = nconv_amd._lib
    assert host_report["kinds"] == [L.COLOR_NONE, L.COLOR_F32_PLANAR, L.COLOR_U8_INTERLEAVED]
    assert host_report["abi"][0] == host_report["abi"][1] >= 26
    for key, msg in (("rc_row_stride", "row stride"), ("rc_workspace", "workspace too small")):
        rc, err = host_report[key]
        assert rc == -22 and msg in err, (key, rc, err)
    assert host_report["workspace"] == [8 * 352 * 5 * 4, 0]


# ---- host validation -------------------------------------------------------------------------------
FAKE = {n: 0x10000 * (q + 1) for q, n in enumerate(("depth", "conf", "color", "k", "xyz", "rgb", "index", "offsets", "ws"))}


def _desc(L, color=None, conf=False, color_ptr=None, **kw):
    """A valid B=2, 4 x 8 descriptor (contiguous sources), then one defect."""
    d = L.NconvBackproject()
    d.B, d.H, d.W = 2, 4, 8
    d.depth, d.depth_image_stride, d.depth_row_stride = FAKE["depth"], 32, 8
    d.k, d.k_image_stride = FAKE["k"], 9
    if conf:
        d.conf, d.conf_image_stride, d.conf_row_stride = FAKE["conf"], 32, 8
    if color == "f32":
        d.color, d.color_kind = FAKE["color"], L.COLOR_F32_PLANAR
        d.color_image_stride, d.color_channel_stride, d.color_row_stride = 96, 32, 8
    elif color == "u8":
        d.color, d.color_kind = FAKE["color"], L.COLOR_U8_INTERLEAVED
        d.color_image_stride, d.color_row_stride = 96, 24
    if color_ptr is not None:
        d.color = color_ptr
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# (descriptor defect, message) rejected by both entry points
BAD_DESC = [
    (dict(depth=None), "null depth or k"),
    (dict(k=None), "null depth or k"),
    (dict(B=0), "non-positive"),
    (dict(H=-1), "non-positive"),
    (dict(W=0), "non-positive"),
    (dict(depth_row_stride=7), "row stride"),
    (dict(conf=True, conf_row_stride=7), "row stride"),
    (dict(depth_image_stride=31), "image stride"),
    (dict(conf=True, conf_image_stride=31), "image stride"),
    (dict(depth_row_stride=(1 << 29) // 4, depth_image_stride=1 << 40), "2^31 bytes"),
    (dict(conf=True, conf_row_stride=(1 << 29) // 4, conf_image_stride=1 << 40), "2^31 bytes"),
    (dict(B=1 << 15, H=1 << 8, W=1 << 8, depth_image_stride=1 << 16, depth_row_stride=1 << 8), "below 2^31"),
    (dict(B=1, H=1 << 25, W=1, depth_row_stride=1), "2^24 segments"),
    (dict(z_min=2.0, z_max=1.0), "z_max < z_min"),
    (dict(z_min=-2.0, z_max=-3.0), "z_max < z_min"),
    (dict(z_max=float("nan")), "z_max < z_min"),
    (dict(z_min=float("nan")), "z_max < z_min"),
    (dict(conf_min=float("nan")), "conf_min"),
    (dict(color_kind=3), "unknown color kind"),
    (dict(color_kind=-1), "unknown color kind"),
    (dict(color="f32", color_kind=7), "unknown color kind"),
    (dict(color_kind=1), "both or neither"),
    (dict(color="u8", color_kind=0), "both or neither"),
    (dict(k_image_stride=-9), "k image stride"),
    (dict(depth=FAKE["depth"] + 2), "4-byte aligned"),
]
# defects of the colour view, looked at only when an rgb output asks for it
BAD_COLOR = [
    (dict(color="f32", color_row_stride=7), "row stride"),
    (dict(color="f32", color_channel_stride=31), "channel stride"),
    (dict(color="f32", color_image_stride=95), "image stride"),
    (dict(color="f32", color_ptr=FAKE["color"] + 1), "4-byte aligned"),
    (dict(color="u8", color_row_stride=23), "row stride"),
    (dict(color="u8", color_image_stride=95), "image stride"),
    (dict(color="u8", color_row_stride=(1 << 31) // 4, color_image_stride=1 << 40), "2^31 bytes"),
    (dict(), "without a color source"),
]


def _points(lib, d, xyz=FAKE["xyz"], rgb=None, index=None, capacity=64, offsets=FAKE["offsets"], ws=FAKE["ws"],
            ws_bytes=1 << 20):
    return lib.nconv_backproject_points(ctypes.byref(d), xyz, rgb, index, capacity, offsets, ws, ws_bytes, None)


@pytest.mark.parametrize("bad,msg", BAD_DESC)
def test_both_calls_reject_bad_descriptors(nconv_amd, bad, msg):
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L, **bad)
    assert lib.nconv_backproject_map(ctypes.byref(d), FAKE["xyz"], None) == -22
    assert msg in lib.nconv_last_error().decode()
    assert _points(lib, d) == -22
    assert msg in lib.nconv_last_error().decode()


@pytest.mark.parametrize("bad,msg", BAD_COLOR)
def test_points_reject_bad_colour_views(nconv_amd, bad, msg):
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L, **bad)
    assert _points(lib, d, rgb=FAKE["rgb"]) == -22
    assert msg in lib.nconv_last_error().decode()


def test_calls_reject_bad_arguments(nconv_amd):
    L = nconv_amd._lib
    lib = L.lib()
    assert lib.nconv_backproject_map(None, FAKE["xyz"], None) == -22
    assert "null descriptor" in lib.nconv_last_error().decode()
    assert lib.nconv_backproject_points(None, FAKE["xyz"], None, None, 4, FAKE["offsets"], FAKE["ws"], 64, None) == -22
    assert "null descriptor" in lib.nconv_last_error().decode()
    d = _desc(L)
    assert lib.nconv_backproject_map(ctypes.byref(d), None, None) == -22
    assert "null xyz" in lib.nconv_last_error().decode()
    need = lib.nconv_backproject_workspace_bytes(2, 4, 8)
    assert need == 2 * 4 * 1 * 4
    for kw, msg in ((dict(capacity=-1), "negative capacity"),
                    (dict(xyz=None), "null xyz"),
                    (dict(offsets=None), "null offsets"),
                    (dict(ws=None), "workspace too small"),
                    (dict(ws_bytes=need - 1), "workspace too small"),
                    (dict(ws_bytes=0), "workspace too small"),
                    (dict(ws=FAKE["ws"] + 2), "4-byte aligned"),
                    (dict(index=FAKE["index"] + 1), "4-byte aligned"),
                    (dict(xyz=FAKE["xyz"] + 2), "4-byte aligned")):
        assert _points(lib, d, **kw) == -22, msg
        assert msg in lib.nconv_last_error().decode(), msg
    # sizes without a workspace
    for B, H, W in ((0, 4, 8), (2, -1, 8), (2, 4, 0), (1 << 15, 1 << 8, 1 << 8), (1, 1 << 25, 1)):
        assert lib.nconv_backproject_workspace_bytes(B, H, W) == 0
    assert lib.nconv_backproject_workspace_bytes(8, 352, 1216) == 8 * 352 * 5 * 4


def test_single_image_ignores_image_strides(nconv_amd):
    """B == 1: the image strides are not looked at (the call then fails only at the next defect)."""
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L, conf=True, B=1, depth_image_stride=0, conf_image_stride=1)
    assert _points(lib, d, offsets=None) == -22
    assert "null offsets" in lib.nconv_last_error().decode()


# ---- Python argument checks ------------------------------------------------------------------------
def test_pointcloud_refuses_cpu_tensors_and_bad_arguments(nconv_amd):
    P = nconv_amd.pointcloud
    assert nconv_amd.backproject is P.backproject and nconv_amd.backproject_map is P.backproject_map
    assert nconv_amd.PointCloud is P.PointCloud and nconv_amd.write_ply is P.write_ply
    z, k = torch.ones(2, 1, 4, 8), torch.eye(3)
    for fn in (P.backproject, P.backproject_map):
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            fn(z, k)
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            fn(z[0, 0], k)
        with pytest.raises(TypeError, match="depth"):
            fn(z.double(), k)
        with pytest.raises(TypeError, match="k"):
            fn(z, k.double())
        with pytest.raises(ValueError, match="k must be"):
            fn(z, torch.eye(4))
        with pytest.raises(ValueError, match="k must be"):
            fn(z, torch.zeros(3, 3, 3))
        with pytest.raises(ValueError, match="depth"):
            fn(torch.ones(2, 1, 4, 16)[..., ::2], k)
        with pytest.raises(ValueError, match="depth"):
            fn(torch.ones(2, 3, 4, 8), k)
        with pytest.raises(ValueError, match="not contiguous"):
            fn(z, torch.zeros(3, 6)[:, ::2])
    # the checks that need a device source come after the device check, so only what precedes it is reachable here
    with pytest.raises(TypeError, match="tensor"):
        P.backproject(np.ones((4, 8), dtype=np.float32), k)


def test_dnet_confidence_refuses_grad_mode_and_cpu_input(nconv_amd):
    net = nconv_amd.SETP1_NCONV(crop="generalized")
    S = torch.zeros(1, 1, 16, 20)
    assert any(p.requires_grad for p in net.parameters())
    for m in (net, net.d_net):
        with pytest.raises(RuntimeError, match="inference only"):
            m.forward_with_confidence(S)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="ROCm devices only"):
                m.forward_with_confidence(S)
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="inference only"):
        net.forward_with_confidence(S.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        net.forward_with_confidence(S)
