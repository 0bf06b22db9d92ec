"""CPU: the numpy reference of the surface normals against the analytic plane (which sets
PLANE_ANGLE_TOL) and a sphere, its gate and one-sided differences; the two entry points are exported,
declared and bound with the C struct's layout under an unchanged ABI number; every malformed call
fails on the host with -22 before any launch; the Python functions refuse CPU tensors and malformed
arguments; write_ply with normals round-trips and is unchanged without them."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import host_harness
import normals_cases as NC
import pointcloud_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
NEW = ("nconv_depth_normals", "nconv_depth_normals_points")
F32 = np.float32


# ---- the reference ---------------------------------------------------------------------------------
def _unit_and_facing(ref, depth, k):
    """Every normal of ref is unit to 2 ulp of 1 and satisfies n . P <= 0."""
    xyz, _ = PC.map_ref(depth, k)
    has = ~np.isnan(ref[:, 0])
    n = ref.transpose(0, 2, 3, 1)[has].astype(np.float64)
    p = xyz.transpose(0, 2, 3, 1)[has].astype(np.float64)
    assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 2 * 2.0 ** -23).all()
    assert ((n * p).sum(1) <= 0).all()


def test_reference_against_analytic_plane():
    """The gate is off: along these planes the depth changes by more than a tenth of itself per pixel
    at the far end, which is what the gate is there to cut."""
    H, W = 9, 261
    worst = 0.0
    for z, n in NC.plane_cases(H, W):
        assert z.shape == (1, H, W) and z.min() >= 1.99 and z.max() <= 86.0 and z.max() >= 80.0
        assert PC.valid_ref(z).all()  # inside (z_min, z_max] = (0, FLT_MAX]
        ref = NC.normals_ref(z, NC.K_SMOOTH, jump_rel=0.0, jump_abs=0.0)
        assert not np.isnan(ref).any()  # every pixel has a normal
        a = NC.angle(ref, np.broadcast_to(n.reshape(1, 3, 1, 1), ref.shape)).max()
        print(f"plane normal {n}: worst angle {a:.4e} rad")
        worst = max(worst, a)
        _unit_and_facing(ref, z, NC.K_SMOOTH)
    print(f"worst angle {worst:.4e} rad, PLANE_ANGLE_TOL {NC.PLANE_ANGLE_TOL:.4e}")
    assert NC.PLANE_ANGLE_TOL == 2.0 * NC.PLANE_ANGLE_MEASURED
    assert worst <= NC.PLANE_ANGLE_TOL and worst >= 0.99 * NC.PLANE_ANGLE_MEASURED


def test_reference_against_analytic_sphere():
    """A chord between two points of a sphere is perpendicular to the radius through its midpoint,
    which is within theta of the centre pixel's radius, theta the largest angle between neighbouring
    pixels' radii. Two tangents each within theta of the tangent plane and about a right angle apart
    put the normal within theta_u + theta_v of the analytic one; the bound allows twice that, plus the
    rounding measured on the plane."""
    B, H, W = 2, 9, 261
    z, n = NC.sphere_cap((0.3, 0.0, 60.0), 50.0, NC.K_SMOOTH, B, H, W)
    assert PC.valid_ref(z).all()
    ref = NC.normals_ref(z, NC.K_SMOOTH)
    assert not np.isnan(ref).any()
    theta_u = NC.angle(n[..., 1:].transpose(0, 2, 3, 1).reshape(-1, 3), n[..., :-1].transpose(0, 2, 3, 1).reshape(-1, 3)).max()
    theta_v = NC.angle(n[:, :, 1:].transpose(0, 2, 3, 1).reshape(-1, 3), n[:, :, :-1].transpose(0, 2, 3, 1).reshape(-1, 3)).max()
    a = NC.angle(ref, n).max()
    print(f"sphere: worst angle {a:.4e} rad, theta_u {theta_u:.4e}, theta_v {theta_v:.4e}")
    assert a <= 2.0 * (theta_u + theta_v) + NC.PLANE_ANGLE_TOL
    _unit_and_facing(ref, z, NC.K_SMOOTH)


def test_reference_fronto_parallel_and_borders():
    k = np.array([[2.0, 0, 1.5], [0, 4.0, 0.5], [0, 0, 1]], dtype=F32)
    z = np.full((1, 3, 4), 8.0, dtype=F32)
    ref = NC.normals_ref(z, k)
    assert np.array_equal(ref[0, :, 1, 1], np.array([0.0, 0.0, -1.0], dtype=F32))
    assert (ref[:, 2] == -1.0).all()  # the borders take one-sided differences
    # a single row or column has no vertical or horizontal neighbour anywhere
    assert np.isnan(NC.normals_ref(z[:, :1], k)).all() and np.isnan(NC.normals_ref(z[:, :, :1], k)).all()


def test_reference_gate_and_isolated_pixels():
    k = NC.K_SMOOTH
    z = np.full((1, 3, 8), 10.0, dtype=F32)
    z[:, :, 4:] = 12.0  # a step of 2 m between columns 3 and 4
    xyz, _ = PC.map_ref(z, k)
    open_ = NC.normals_ref(z, k, jump_rel=0.0, jump_abs=0.0)
    gated = NC.normals_ref(z, k, jump_rel=0.1, jump_abs=0.0)  # tol = 1.0 / 1.2 < 2
    wide = NC.normals_ref(z, k, jump_rel=0.0, jump_abs=2.0)   # tol = 2: the step is within it
    assert np.array_equal(open_.view(np.int32), wide.view(np.int32))
    same = np.all(open_.view(np.int32) == gated.view(np.int32), axis=1)[0]
    assert same[:, [0, 1, 2, 5, 6, 7]].all() and not same[:, [3, 4]].any()
    # beside the step the horizontal tangent is the one-sided difference: the normal of a flat wall
    assert (gated[0, 2] == -1.0).all() and not (open_[0, 2, :, 3:5] == -1.0).any()
    tu = (xyz[0, :, 1, 3] - xyz[0, :, 1, 2]).astype(F32)
    assert tu[2] == 0.0 and tu[0] > 0
    # the gate compares with <=: a step exactly at the tolerance is usable
    edge = NC.normals_ref(z, k, jump_rel=0.0, jump_abs=2.0 - 2.0 ** -20)
    assert np.array_equal(edge.view(np.int32), gated.view(np.int32))
    # an isolated valid pixel, and one with neighbours on one axis only, have no normal
    z = np.zeros((1, 5, 5), dtype=F32)
    z[0, 2, 2] = 5.0
    assert np.isnan(NC.normals_ref(z, k)).all()
    z[0, 2, 1] = z[0, 2, 3] = 5.0
    assert np.isnan(NC.normals_ref(z, k)).all()
    z[0, 1, 2] = 5.0
    ref = NC.normals_ref(z, k)
    assert not np.isnan(ref[0, :, 2, 2]).any() and np.isnan(ref[0, 0]).sum() == 24
    # NaN and inf depths are not usable neighbours; a negative z_min does not make the outside valid
    z = np.full((1, 3, 3), 5.0, dtype=F32)
    z[0, 1, 0], z[0, 0, 1] = np.nan, np.inf
    ref = NC.normals_ref(z, k, z_min=-1.0, jump_rel=0.0)
    assert not np.isnan(ref[0, :, 1, 1]).any() and np.isnan(ref[0, :, 1, 0]).all() and np.isnan(ref[0, :, 0, 1]).all()
    one = NC.normals_ref(np.zeros((1, 1, 4), dtype=F32), k, z_min=-1.0, jump_rel=0.0)
    assert np.isnan(one).all()


def test_reference_picture_and_packed():
    n = np.full((1, 3, 1, 4), np.nan, dtype=F32)
    n[0, :, 0, 0] = (0.0, 0.0, -1.0)
    n[0, :, 0, 1] = (1.0, 0.0, 0.0)
    n[0, :, 0, 2] = (0.0, -1.0, 0.0)
    img = NC.picture_ref(n, empty=(1, 2, 3))
    # 127.5 rounds to the even 128
    assert img[0, 0].tolist() == [[128, 128, 255], [255, 128, 128], [128, 255, 128], [1, 2, 3]]
    rows = NC.packed_ref(n, [3, 0])
    assert rows.tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, -1.0]]


# ---- write_ply -------------------------------------------------------------------------------------
def _old_write_ply(path, xyz, rgb=None):
    """The file write_ply produced before it knew normals, restated."""
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}",
            "property float x", "property float y", "property float z"]
    if rgb is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        for v in range(len(xyz)):
            fh.write(struct.pack("<fff", *xyz[v].tolist()))
            if rgb is not None:
                fh.write(struct.pack("<BBB", *rgb[v].tolist()))


@pytest.mark.parametrize("n", [0, 1, 257])
def test_write_ply_with_normals(tmp_path, nconv_amd, n):
    rng = np.random.default_rng(n)
    xyz = rng.normal(size=(n, 3)).astype(F32)
    nrm = rng.normal(size=(n, 3)).astype(F32)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.int64).astype(np.uint8)
    p, q = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    for colours in (None, rgb):
        nconv_amd.write_ply(p, xyz, colours)
        _old_write_ply(q, xyz, colours)
        assert open(p, "rb").read() == open(q, "rb").read()
        nconv_amd.write_ply(p, xyz, colours, normals=None)
        assert open(p, "rb").read() == open(q, "rb").read()
    nconv_amd.write_ply(p, torch.from_numpy(xyz), rgb, torch.from_numpy(nrm))
    raw = open(p, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert raw[:end].decode("ascii").split("\n") == [
        "ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y",
        "property float z", "property float nx", "property float ny", "property float nz", "property uchar red",
        "property uchar green", "property uchar blue", "end_header", ""]
    body = raw[end:]
    assert len(body) == 27 * n
    for v in range(n):
        rec = struct.unpack_from("<ffffffBBB", body, 27 * v)
        assert rec[:3] == tuple(xyz[v].tolist()) and rec[3:6] == tuple(nrm[v].tolist())
        assert rec[6:] == tuple(rgb[v].tolist())
    nconv_amd.write_ply(p, xyz, normals=nrm)
    raw = open(p, "rb").read()
    assert b"property float nz\nend_header\n" in raw and len(raw[raw.index(b"end_header\n") + 11:]) == 24 * n
    with pytest.raises(TypeError):
        nconv_amd.write_ply(p, xyz, normals=nrm.astype(np.float64))
    with pytest.raises(TypeError):
        nconv_amd.write_ply(p, xyz, normals=nrm[:, :2])


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


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "normals_host")


def test_struct_layout_matches_ctypes(nconv_amd, host_report):
    S = nconv_amd._lib.NconvNormalsOpts
    want = host_harness.ctypes_layout(S, "nconv_normals_opts")
    c = {k: v for k, v in host_report.items() if k.startswith("nconv_normals_opts")}
    assert len(c) == 4 and c == want and want["nconv_normals_opts"] == [0, 12]


def test_host_calls(host_report):
    assert host_report["abi"] == [27, 27]
    for key, msg in (("rc_no_output", "nothing to write"), ("rc_jump", "must be >= 0"), ("rc_row_stride", "row stride"),
                     ("rc_capacity", "negative capacity")):
        rc, err = host_report[key]
        assert rc == -22 and msg in err, (key, rc, err)
    assert host_report["rc_empty"] == [0]


# ---- host validation -------------------------------------------------------------------------------
FAKE = {n: 0x10000 * (q + 1) for q, n in enumerate(("depth", "conf", "color", "k", "normals", "image", "index", "offsets"))}


def _desc(L, conf=False, **kw):
    """A valid B=2, 4 x 8 descriptor (contiguous sources), then one defect."""
    d = L.NconvBackproject()
    d.B, d.H, d.W = 2, 4, 8
    d.depth, d.depth_image_stride, d.depth_row_stride = FAKE["depth"], 32, 8
    d.k, d.k_image_stride = FAKE["k"], 9
    if conf:
        d.conf, d.conf_image_stride, d.conf_row_stride = FAKE["conf"], 32, 8
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _opts(L, jump_rel=0.1, jump_abs=0.0):
    o = L.NconvNormalsOpts()
    o.jump_rel, o.jump_abs = jump_rel, jump_abs
    return o


# what nconv_backproject_map refuses in the descriptor (tests/test_pointcloud_cpu.py: BAD_DESC)
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
    (dict(B=1 << 15, H=1 << 8, W=1 << 8, depth_image_stride=1 << 16, depth_row_stride=1 << 8), "below 2^31"),
    (dict(B=1, H=1 << 25, W=1, depth_row_stride=1), "2^24 segments"),
    (dict(z_min=2.0, z_max=1.0), "z_max < z_min"),
    (dict(z_max=float("nan")), "z_max < z_min"),
    (dict(conf_min=float("nan")), "conf_min"),
    (dict(color_kind=3), "unknown color kind"),
    (dict(color_kind=1), "both or neither"),
    (dict(k_image_stride=-9), "k image stride"),
    (dict(depth=FAKE["depth"] + 2), "4-byte aligned"),
]


def _map(lib, d, o, normals=FAKE["normals"], image=FAKE["image"]):
    return lib.nconv_depth_normals(None if d is None else ctypes.byref(d), None if o is None else ctypes.byref(o),
                                   normals, image, None)


def _points(lib, d, o, index=FAKE["index"], offsets=FAKE["offsets"], capacity=64, normals=FAKE["normals"]):
    return lib.nconv_depth_normals_points(None if d is None else ctypes.byref(d),
                                          None if o is None else ctypes.byref(o), index, offsets, capacity, normals,
                                          None)


@pytest.mark.parametrize("bad,msg", BAD_DESC)
def test_both_calls_reject_bad_descriptors(nconv_amd, bad, msg):
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L, **bad)
    for call in (_map, _points):
        assert call(lib, d, _opts(L)) == -22
        assert msg in lib.nconv_last_error().decode()
        assert call(lib, d, None) == -22
        assert msg in lib.nconv_last_error().decode()


def test_calls_reject_bad_arguments(nconv_amd):
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L)
    for call in (_map, _points):
        assert call(lib, None, _opts(L)) == -22
        assert "null descriptor" in lib.nconv_last_error().decode()
        for kw in (dict(jump_rel=-1.0), dict(jump_abs=-0.5), dict(jump_rel=float("nan")), dict(jump_abs=float("nan")),
                   dict(jump_rel=-float("inf"))):
            assert call(lib, d, _opts(L, **kw)) == -22, kw
            assert "must be >= 0" in lib.nconv_last_error().decode()
    assert _map(lib, d, _opts(L), normals=None, image=None) == -22
    assert "nothing to write" in lib.nconv_last_error().decode()
    assert _map(lib, d, None, normals=None, image=None) == -22
    assert _map(lib, d, _opts(L), normals=FAKE["normals"] + 2) == -22
    assert "4-byte aligned" in lib.nconv_last_error().decode()
    for kw, msg in ((dict(capacity=-1), "negative capacity"),
                    (dict(index=None), "null index"),
                    (dict(offsets=None), "null index"),
                    (dict(normals=None), "null index"),
                    (dict(index=FAKE["index"] + 1), "4-byte aligned"),
                    (dict(offsets=FAKE["offsets"] + 2), "4-byte aligned"),
                    (dict(normals=FAKE["normals"] + 3), "4-byte aligned")):
        assert _points(lib, d, _opts(L), **kw) == -22, msg
        assert msg in lib.nconv_last_error().decode(), msg
    # capacity 0 is legal, launches nothing and needs no pointer; a bad descriptor is still refused
    assert _points(lib, d, _opts(L), index=None, offsets=None, capacity=0, normals=None) == 0
    assert _points(lib, d, None, capacity=0) == 0
    assert _points(lib, _desc(L, W=0), None, capacity=0) == -22


# ---- Python argument checks ------------------------------------------------------------------------
def test_normals_refuse_cpu_tensors_and_bad_arguments(nconv_amd):
    P = nconv_amd.pointcloud
    assert nconv_amd.normals is P.normals and nconv_amd.normal_image is P.normal_image
    z, k = torch.ones(2, 1, 4, 8), torch.eye(3)
    for fn in (P.normals, P.normal_image, P.normals_and_image, lambda *a, **kw: P.backproject(*a, normals=True, **kw)):
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
        with pytest.raises(ValueError, match="depth"):
            fn(torch.ones(2, 1, 4, 16)[..., ::2], k)
        with pytest.raises(ValueError, match="depth"):
            fn(torch.ones(2, 3, 4, 8), k)
        for kw in (dict(jump_rel=-0.1), dict(jump_abs=-1.0), dict(jump_rel=float("nan"))):
            with pytest.raises(ValueError, match="must be >= 0"):
                fn(z, k, **kw)
    with pytest.raises(ValueError, match="empty"):
        P.normal_image(z, k, empty=(0, 256, 0))
    # the jumps and the empty colour are checked without a device
    for kw in (dict(jump_rel=-0.1), dict(jump_abs=-1.0), dict(jump_rel=float("nan"))):
        with pytest.raises(ValueError, match="must be >= 0"):
            P._normals_opts(**{"jump_rel": 0.1, "jump_abs": 0.0, **kw})
    with pytest.raises(ValueError, match="empty"):
        P._normals_opts(0.1, 0.0, (0, 256, 0))
    with pytest.raises(ValueError, match="empty"):
        P._normals_opts(0.1, 0.0, (0, 0))


def test_pointcloud_keeps_its_three_tuple(nconv_amd):
    xyz, off = torch.zeros(4, 3), torch.tensor([0, 1, 3], dtype=torch.int32)
    pc = nconv_amd.PointCloud(xyz, None, None, off)
    assert pc.normals is None and pc.image_normals(1) is None and len(pc.image(1)) == 3
    nrm = torch.arange(12.0).reshape(4, 3)
    pc = nconv_amd.PointCloud(xyz, None, None, off, nrm)
    assert len(pc.image(1)) == 3 and torch.equal(pc.image_normals(1), nrm[1:3])
    assert pc.image_normals(0).shape == (1, 3)
