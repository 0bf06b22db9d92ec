"""The C boundary of nconv_pose_normal_eq / nconv_pose_update from a plain C host (tests/host/pose_host.c): the
descriptor's layout against the ctypes structure, the workspace sizes, and every -EINVAL path the header lists."""
import pytest

import host_harness


@pytest.fixture(scope="module")
def report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "pose_host")


def test_host_descriptor_layout_matches_ctypes(nconv_amd, report):
    want = host_harness.ctypes_layout(nconv_amd._lib.NconvPoseAlign, "nconv_pose_align")
    assert {key: report[key] for key in want} == want
    assert report["abi"] == [27, 27]
    # the leading fields are nconv_view_warp's, at its offsets
    warp = host_harness.ctypes_layout(nconv_amd._lib.NconvViewWarp, "nconv_view_warp")
    for key, val in warp.items():
        if "." in key:
            assert report["nconv_pose_align." + key.split(".")[1]] == val


def test_host_workspace_sizes(nconv_amd, report):
    small, full, zero_b, neg_w, odd = report["ws"]
    tiles = lambda B, H, W: B * ((H + 15) // 16) * ((W + 63) // 64)  # noqa: E731
    size = lambda B, H, W: 8 * B * (12 + 28) + 4 * 29 * tiles(B, H, W)  # noqa: E731
    assert (small, full, odd) == (size(2, 4, 8), size(8, 352, 1216), size(3, 17, 65))
    assert zero_b == 0 and neg_w == 0
    assert nconv_amd.pose.workspace_bytes(2, 4, 8) == small


BOTH = ("neq", "upd")
ENTRY = {"neq": "nconv_pose_normal_eq", "upd": "nconv_pose_update"}
NEW_NULL = "null k_src, pose, status, cost or n_hist"


@pytest.mark.parametrize("case,why,sides", [
    ("null_descriptor", "null descriptor", BOTH),
    ("null_depth", "null depth, src, k or m", BOTH), ("null_src", "null depth, src, k or m", BOTH),
    ("null_k", "null depth, src, k or m", BOTH), ("null_m", "null depth, src, k or m", BOTH),
    ("C_2", "C must be 1 or 3", BOTH),
    ("B_zero", "non-positive", BOTH), ("H_negative", "non-positive", BOTH), ("Ws_zero", "non-positive", BOTH),
    ("W_above_2_24", "at most 2^24", BOTH), ("batch_too_large", "batch too large", BOTH),
    ("k_stride_negative", "negative k or m image stride", BOTH),
    ("m_stride_negative", "negative k or m image stride", BOTH),
    ("z_min_negative", "z_min must be >= 0", BOTH), ("z_min_nan", "z_min must be >= 0", BOTH),
    ("z_max_below_z_min", "z_max < z_min", BOTH), ("z_max_nan", "z_max < z_min", BOTH),
    ("depth_misaligned", "not 4-byte aligned", BOTH),
    ("depth_row_stride_short", "depth: row stride smaller than W", BOTH),
    ("depth_image_stride_short", "depth: image stride smaller", BOTH),
    ("mask_row_stride_short", "mask: row stride smaller than W", BOTH),
    ("mask_image_stride_short", "mask: image stride smaller", BOTH),
    ("src_row_stride_short", "src: row stride smaller than W", BOTH),
    ("src_channel_stride_short", "src: channel stride smaller", BOTH),
    ("src_image_stride_short", "src: image stride too small", BOTH),
    ("depth_plane_too_large", "depth: plane too large", BOTH), ("src_plane_too_large", "src: plane too large", BOTH),
    ("null_tgt", "null tgt", BOTH), ("tgt_misaligned", "tgt not 4-byte aligned", BOTH),
    ("tgt_row_stride_short", "tgt: row stride smaller than W", BOTH),
    ("tgt_channel_stride_short", "tgt: channel stride smaller", BOTH),
    ("tgt_plane_too_large", "tgt: plane too large", BOTH),
    ("null_k_src", NEW_NULL, BOTH), ("null_pose", NEW_NULL, BOTH), ("null_status", NEW_NULL, BOTH),
    ("null_cost", NEW_NULL, BOTH), ("null_n_hist", NEW_NULL, BOTH),
    ("pose_misaligned", "not 4-byte aligned", BOTH),
    ("k_src_stride_negative", "negative k_src image stride", BOTH),
    ("m_stride_shared", "m_image_stride below 12", BOTH), ("m_stride_below_12", "m_image_stride below 12", BOTH),
    ("huber_negative", "huber must be >= 0", BOTH), ("huber_nan", "huber must be >= 0", BOTH),
    ("damping_negative", "damping must be >= 0", BOTH), ("damping_nan", "damping must be >= 0", BOTH),
    ("min_points_5", "min_points must be at least 6", BOTH),
    ("history_zero", "history must be positive", BOTH),
    ("workspace_small", "workspace too small", BOTH), ("workspace_null", "workspace too small", BOTH),
    ("workspace_misaligned", "workspace not 8-byte aligned", BOTH),
    ("it_negative", "it outside [0, history)", ("upd",)), ("it_past_history", "it outside [0, history)", ("upd",))])
def test_host_refuses_bad_arguments(report, case, why, sides):
    for side in sides:
        rc, text = report[f"{side}_{case}"]
        assert rc == -22 and why in text and text.startswith(ENTRY[side] + ":"), (side, rc, text)
