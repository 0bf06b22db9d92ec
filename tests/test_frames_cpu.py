"""CPU: the frame entry points (nconv_frame_ingest, nconv_depth_export_u16) are exported, declared
and bound with the C struct's layout; every malformed call fails on the host with -22 before any
launch; frames.ingest refuses CPU tensors and non-unit inner strides; the loaders' raw=True samples
pushed through the numpy reference equal the raw=False samples bit for bit; the 16-bit PNG writer
round-trips; DevicePrefetcher keeps today's positional call."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

import frames_cases as FC
import host_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nconv.h")
NEW = ("nconv_frame_ingest", "nconv_depth_export_u16")


def test_entry_points_exported_and_declared(nconv_amd):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(nconv_\w+)\s*\(", src, re.M))
    lib = nconv_amd._lib.lib()
    for name in NEW:
        assert name in declared and name in nconv_amd._lib.EXPORTED
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    v = int(re.search(r"#define NCONV_ABI_VERSION (\d+)", src).group(1))
    assert lib.nconv_abi_version() == v == nconv_amd._lib.ABI_VERSION and v >= 25


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "frames_host")


@pytest.mark.parametrize("c_name,py_name", [("nconv_frame_plane", "NconvFramePlane"),
                                            ("nconv_frame_ingest_desc", "NconvFrameIngest")])
def test_struct_layout_matches_ctypes(nconv_amd, host_report, c_name, py_name):
    c = {k: v for k, v in host_report.items() if k == c_name or k.startswith(c_name + ".")}
    assert len(c) > 5 and c == host_harness.ctypes_layout(getattr(nconv_amd._lib, py_name), c_name)


def test_host_calls_and_enum(nconv_amd, host_report):
    L = nconv_amd._lib
    assert host_report["dtypes"] == [L.FRAME_U8, L.FRAME_U16, L.FRAME_F32]
    assert host_report["abi"][0] == host_report["abi"][1] >= 25
    for key, msg in (("rc_row_stride", "row stride"), ("rc_scale", "scale")):
        rc, err = host_report[key]
        assert rc == -22 and msg in err, (key, rc, err)


FAKE, FAKE_OUT = 0x10000, 0x20000  # never dereferenced: validation fails on the host first


def _desc(L, rgb=True, planes=(1,), **kw):
    """A valid B=2, 4 x 8 descriptor (contiguous sources), then one defect."""
    d = L.NconvFrameIngest()
    d.B, d.h, d.w, d.reverse = 2, 4, 8, 1
    if rgb:
        d.rgb, d.rgb_image_stride, d.rgb_row_stride, d.rgb_out = FAKE, 96, 24, FAKE_OUT
    for k, dt in enumerate(planes):
        e = {L.FRAME_U8: 1, L.FRAME_U16: 2, L.FRAME_F32: 4}[dt]
        p = d.plane[k]
        p.src, p.image_stride, p.row_stride, p.dtype, p.out = FAKE, 32 * e, 8 * e, dt, FAKE_OUT
        p.shift, p.scale = (8 if dt == L.FRAME_U16 else 0), 1.0 / 256.0
    for k, v in kw.items():
        obj, _, field = k.rpartition("__")
        setattr(d.plane[int(obj[-1])] if obj else d, field, v)
    return d


INGEST_BAD = [
    (dict(rgb=False, planes=()), "nothing to do"),
    (dict(B=0), "non-positive"),
    (dict(h=0), "non-positive"),
    (dict(w=-1), "non-positive"),
    (dict(rgb_row_stride=23), "row stride"),
    (dict(plane0__row_stride=15), "row stride"),
    (dict(rgb_image_stride=95), "image stride"),
    (dict(plane0__image_stride=62), "image stride"),
    (dict(plane0__dtype=3), "unknown dtype"),
    (dict(plane0__dtype=-1), "unknown dtype"),
    (dict(plane0__shift=16), "shift outside 0..15"),
    (dict(plane0__shift=-1), "shift outside 0..15"),
    (dict(planes=(2,), plane0__shift=1), "non-zero shift with F32"),
    (dict(plane0__src=FAKE + 1), "not aligned to its element size"),
    (dict(B=1, plane0__row_stride=17), "not aligned to its element size"),
    (dict(planes=(2,), plane0__src=FAKE + 2), "not aligned to its element size"),
    (dict(planes=(1, 2), plane1__image_stride=130), "not aligned to its element size"),
    (dict(rgb_out=None), "null rgb_out"),
    (dict(plane0__out=None), "null plane out"),
    (dict(planes=(1, 0), plane1__out=None), "null plane out"),
]


@pytest.mark.parametrize("bad,msg", INGEST_BAD)
def test_ingest_rejects_bad_descriptors(nconv_amd, bad, msg):
    L = nconv_amd._lib
    lib = L.lib()
    assert lib.nconv_frame_ingest(ctypes.byref(_desc(L, **bad)), None) == -22
    assert msg in lib.nconv_last_error().decode()


def test_ingest_rejects_null_descriptor(nconv_amd):
    lib = nconv_amd._lib.lib()
    assert lib.nconv_frame_ingest(None, None) == -22
    assert "null descriptor" in lib.nconv_last_error().decode()


def test_ingest_single_image_ignores_image_stride(nconv_amd):
    """B == 1: the image stride is not looked at (validation passes it; the call then fails only at
    the next defect)."""
    L = nconv_amd._lib
    lib = L.lib()
    d = _desc(L, B=1, rgb_image_stride=0, plane0__image_stride=1, plane0__out=None)
    assert lib.nconv_frame_ingest(ctypes.byref(d), None) == -22
    assert "null plane out" in lib.nconv_last_error().decode()


def test_export_rejects_bad_arguments(nconv_amd):
    lib = nconv_amd._lib.lib()
    p, o = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE_OUT)
    # (pred, image_stride, row_stride, B, H, W, scale, out, stream)
    cases = [
        ((None, 32, 8, 2, 4, 8, 256.0, o, None), "null pred or out"),
        ((p, 32, 8, 2, 4, 8, 256.0, None, None), "null pred or out"),
        ((p, 32, 8, 0, 4, 8, 256.0, o, None), "non-positive"),
        ((p, 32, 8, 2, 4, 0, 256.0, o, None), "non-positive"),
        ((p, 32, 7, 2, 4, 8, 256.0, o, None), "row stride"),
        ((p, 31, 8, 2, 4, 8, 256.0, o, None), "image stride"),
        ((p, 32, 8, 2, 4, 8, float("nan"), o, None), "scale must be positive"),
        ((p, 32, 8, 2, 4, 8, 0.0, o, None), "scale must be positive"),
        ((p, 32, 8, 2, 4, 8, -256.0, o, None), "scale must be positive"),
        ((ctypes.c_void_p(FAKE + 2), 32, 8, 2, 4, 8, 256.0, o, None), "aligned"),
        ((p, 32, 8, 2, 4, 8, 256.0, ctypes.c_void_p(FAKE_OUT + 1), None), "aligned"),
    ]
    for args, msg in cases:
        assert lib.nconv_depth_export_u16(*args) == -22, msg
        assert msg in lib.nconv_last_error().decode(), msg


def test_frames_refuse_cpu_tensors_and_inner_strides(nconv_amd):
    F = nconv_amd.frames
    assert nconv_amd.ingest is F.ingest and nconv_amd.export_depth16 is F.export_depth16
    rgb = torch.zeros(1, 4, 8, 3, dtype=torch.uint8)
    d16 = torch.zeros(1, 4, 8, dtype=torch.uint16)
    for kw in (dict(rgb=rgb), dict(depth=d16), dict(gt=d16), dict(rgb=rgb, depth=d16, gt=d16)):
        with pytest.raises(RuntimeError, match="ROCm devices only"):
            F.ingest(**kw)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        F.export_depth16(torch.zeros(1, 1, 4, 8))
    with pytest.raises(ValueError):
        F.ingest()
    # the stride checks come before the device check and name the argument
    with pytest.raises(ValueError, match="depth"):
        F.ingest(depth=torch.zeros(1, 4, 16, dtype=torch.uint16)[:, :, ::2])
    with pytest.raises(ValueError, match="gt"):
        F.ingest(gt=torch.zeros(1, 8, 4, dtype=torch.uint16).transpose(1, 2))
    with pytest.raises(ValueError, match="rgb"):
        F.ingest(rgb=torch.zeros(1, 4, 8, 4, dtype=torch.uint8)[..., :3])
    with pytest.raises(ValueError, match="rgb"):
        F.ingest(rgb=torch.zeros(1, 3, 4, 8, dtype=torch.uint8).permute(0, 2, 3, 1))
    # sliced views with a unit innermost stride are geometry the kernel takes (byte strides)
    assert F._plane_view(torch.zeros(2, 6, 12, dtype=torch.uint16)[:, 1:5, 2:10], "depth") == (2, 4, 8, 144, 24)
    assert F._plane_view(torch.zeros(2, 1, 6, 12)[:, :, 1:5, 2:10], "gt") == (2, 4, 8, 288, 48)
    assert F._rgb_view(torch.zeros(2, 6, 12, 3, dtype=torch.uint8)[:, 1:5, 2:10]) == (2, 4, 8, 216, 36)


# ---- raw loaders -------------------------------------------------------------------------------------
def _save(path, a):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(a).save(path)


def _kitti_trees(tmp, H=20, W=40):
    """train (16-bit lidar + gt), val_selection_cropped (16-bit) and the anonymous test split (8-bit
    lidar) with random images; returns nothing: the raw=False loaders are the expectation."""
    rng = np.random.default_rng(5)
    drive, date, f = "2011_09_26_drive_0001_sync", "2011_09_26", "0000000005.png"
    u16 = lambda p: (rng.integers(0, 65536, (H, W)) * (rng.random((H, W)) < p)).astype(np.uint16)
    rgb = lambda: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    _save(os.path.join(tmp, "data_depth_annotated", "train", drive, "proj_depth", "groundtruth", "image_02", f), u16(0.5))
    _save(os.path.join(tmp, "data_depth_velodyne", "train", drive, "proj_depth", "velodyne_raw", "image_02", f), u16(0.3))
    _save(os.path.join(tmp, "raw", date, drive, "image_02", "data", f), rgb())
    P2 = np.arange(12, dtype=np.float64) + 1.5
    with open(os.path.join(tmp, "raw", date, "calib_cam_to_cam.txt"), "w") as fh:
        fh.write("P_rect_02: " + " ".join(str(v) for v in P2) + "\n")
    for split, lidar in (("val_selection_cropped", u16(0.3)),
                         ("test_depth_completion_anonymous", rng.integers(0, 256, (H, W), dtype=np.uint8))):
        base = os.path.join(tmp, split)
        _save(os.path.join(base, "velodyne_raw", "a.png"), lidar)
        _save(os.path.join(base, "image", "a.png"), rgb())
        if split == "val_selection_cropped":
            _save(os.path.join(base, "groundtruth_depth", "a.png"), u16(0.5))
        os.makedirs(os.path.join(base, "intrinsics"))
        with open(os.path.join(base, "intrinsics", "a.txt"), "w") as fh:
            fh.write(" ".join(str(v) for v in np.arange(9) + 0.5))


@pytest.mark.parametrize("decode", ["reference", "kitti16"])
@pytest.mark.parametrize("loader", ["DataLoader_KITTI", "DataLoader_KITTI_seltest", "DataLoader_KITTI_test"])
def test_raw_kitti_samples_decode_to_the_fp32_samples(tmp_path, nconv_amd, loader, decode):
    _kitti_trees(str(tmp_path))
    cls = getattr(nconv_amd.data, loader)
    args = (str(tmp_path), "train") if loader == "DataLoader_KITTI" else (str(tmp_path),)
    kw = dict(height=16, width=32, depth_decode=decode)
    old, raw = cls(*args, **kw)[0], cls(*args, raw=True, **kw)[0]
    assert set(old) == set(raw) and len(cls(*args, raw=True, **kw)) == 1
    assert raw["rgb"].dtype == torch.uint8 and tuple(raw["rgb"].shape) == (16, 32, 3) and raw["rgb"].is_contiguous()
    want = torch.uint8 if loader == "DataLoader_KITTI_test" else torch.uint16
    planes = {k: np.asarray(raw[k])[None] for k in ("depth", "gt") if k in raw}
    for k, v in planes.items():
        assert raw[k].dtype == want and v.shape == (1, 16, 32) and raw[k].is_contiguous(), k
    ref = FC.ingest_ref(rgb=np.asarray(raw["rgb"])[None], depth_decode=decode, **planes)
    for k in ("rgb", "depth", "gt"):
        if k in old:
            assert torch.equal(torch.from_numpy(ref[k][0]), old[k]), k
    assert torch.equal(raw["k"], old["k"])
    # raw samples of one loader have one size: the default collate batches them
    b = torch.utils.data.default_collate([raw, raw])
    assert b["rgb"].shape == (2, 16, 32, 3) and b["depth"].shape == (2, 16, 32) and b["depth"].dtype == want


def test_raw_nyu_changes_rgb_only(tmp_path, nconv_amd):
    rng = np.random.default_rng(2)
    for d in ("train/gt", "train/depth", "train/img", "mask"):
        os.makedirs(tmp_path / d)
    np.save(tmp_path / "train/gt/000.npy", rng.random((480, 640)).astype(np.float32) * 10)
    np.save(tmp_path / "train/depth/000.npy", rng.random((480, 640)).astype(np.float32))
    Image.fromarray(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)).save(tmp_path / "train/img/000.png")
    np.save(tmp_path / "mask/m0.npy", (rng.random((480, 640)) < 0.1).astype(np.uint8))
    D = nconv_amd.data
    for kw in (dict(), dict(height=400, width=600)):
        random.seed(0)
        old = D.DataLoader_NYU(str(tmp_path), "train", use_mask=True, add_noise=False, **kw)[0]
        random.seed(0)
        raw = D.DataLoader_NYU(str(tmp_path), "train", use_mask=True, add_noise=False, raw=True, **kw)[0]
        assert raw["rgb"].dtype == torch.uint8 and raw["rgb"].shape[2] == 3 and raw["rgb"].is_contiguous()
        assert torch.equal(torch.from_numpy(FC.rgb_ref(np.asarray(raw["rgb"])[None])[0]), old["rgb"])
        for k in ("depth", "gt", "k"):
            assert torch.equal(raw[k], old[k]), k
    old = D.DataLoader_NYU_test(str(tmp_path), "train")[0]
    raw = D.DataLoader_NYU_test(str(tmp_path), "train", raw=True)[0]
    assert torch.equal(torch.from_numpy(FC.rgb_ref(np.asarray(raw["rgb"])[None])[0]), old["rgb"])
    assert torch.equal(raw["depth"], old["depth"]) and torch.equal(raw["k"], old["k"])


def test_reference_functions_on_known_values():
    """The numpy reference itself: decodes, channel order, rounding to even, clamps, NaN."""
    v = np.array([[[0, 255, 256, 65535]]], dtype=np.uint16)
    assert FC.plane_ref(v, 8, 1 / 256).reshape(-1).tolist() == [0.0, 0.0, 1 / 256, 255 / 256]
    assert FC.plane_ref(v, 0, 1 / 256).reshape(-1).tolist() == [0.0, 255 / 256, 1.0, 65535 / 256]
    rgb = np.arange(6, dtype=np.uint8).reshape(1, 1, 2, 3)
    assert FC.rgb_ref(rgb)[0, :, 0, :].tolist() == [[2.0, 5.0], [1.0, 4.0], [0.0, 3.0]]
    assert FC.rgb_ref(rgb, reverse=False)[0, :, 0, :].tolist() == [[0.0, 3.0], [1.0, 4.0], [2.0, 5.0]]
    d = np.array([0.5 / 256, 1.5 / 256, 2.5 / 256, -0.0, -1.0, 255.999, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert FC.export_ref(d).tolist() == [0, 2, 2, 0, 0, 65535, 65535, 0, 0]


def test_png16_round_trip(tmp_path, nconv_amd):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 65536, (7, 13), dtype=np.int64).astype(np.uint16)
    a[0, :4] = (0, 255, 256, 65535)
    for name, plane in (("t.png", torch.from_numpy(a)[None, None]), ("n.png", a)):
        path = str(tmp_path / name)
        nconv_amd.write_depth_png16(path, plane)
        with Image.open(path) as im:
            assert im.mode.startswith("I;16") and np.array_equal(np.asarray(im), a)
        # and it is what the loaders read back
        assert np.array_equal(nconv_amd.data.imread_gray_raw(path), a)
    with pytest.raises(TypeError):
        nconv_amd.write_depth_png16(str(tmp_path / "f.png"), a.astype(np.float32))


def test_prefetcher_signature_keeps_todays_call(nconv_amd):
    p = list(inspect.signature(nconv_amd.data.DevicePrefetcher.__init__).parameters.values())
    assert [q.name for q in p] == ["self", "loader", "device", "keys", "ingest"]
    assert p[3].default == ("rgb", "depth", "gt", "k") and p[4].default is None
    ing = nconv_amd.Ingest()
    assert (ing.depth_decode, ing.reverse_rgb) == ("reference", True)
    batch = {"k": torch.zeros(2, 3, 3), "name": ["a", "b"], "depth": torch.zeros(2, 1, 4, 8)}
    assert ing(batch) is batch  # nothing raw: passed through, no launch
