"""CPU: a non-Python host compiled against include/nconv.h agrees with the ctypes binding.

tests/host/capi_host.c is built with gcc against the public header and linked to libnconv.so. It
reports sizeof/offsetof of every ABI struct field, which must equal the ctypes structures of
realtime-depth-estimation-nconv_amd/_lib.py (so header, binding and INTEGRATION.md cannot drift
apart silently), and makes host-validated calls that must return -EINVAL with a message."""
import os
import re

import pytest

import host_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_report(nconv_amd, tmp_path_factory):
    return host_harness.host_report(nconv_amd, tmp_path_factory, "capi_host")


@pytest.mark.parametrize("c_name,py_name", [("nconv_src", "NconvSrc"), ("nconv_layer", "NconvLayer"),
                                            ("nconv_dense_conv", "NconvDenseConv"),
                                            ("nconv_dense_wgrad", "NconvDenseWgrad"),
                                            ("nconv_bwd_io", "NconvBwdIo"),
                                            ("nconv_bn_train", "NconvBnTrain")])
def test_struct_layout_matches_ctypes(nconv_amd, host_report, c_name, py_name):
    py = host_harness.ctypes_layout(getattr(nconv_amd._lib, py_name), c_name)
    c = {k: v for k, v in host_report.items() if k == c_name or k.startswith(c_name + ".")}
    assert c == py


def test_host_validation_and_abi(host_report):
    assert host_report["abi"][0] == host_report["abi"][1]
    for key, msg in (("rc_bad_ho", "Ho/Wo inconsistent"), ("rc_bad_math", "unknown math"),
                     ("rc_bad_mode", "unknown load mode")):
        rc, err = host_report[key]
        assert rc == -22 and msg in err, (key, rc, err)
    assert host_report["bwd_ws_ok"][0] > 0
    # zero-initialised math: NCONV_MATH_FP32, VALU forward / input gradient, fp32-MFMA weight gradient
    assert host_report["plan_zero"] == [0, 1, 1, 1, 2]


def test_integration_doc_binding_matches_ctypes(nconv_amd):
    """The ctypes NconvLayer / NconvSrc field lists shown in INTEGRATION.md §4 equal the binding's."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for cls in ("NconvSrc", "NconvLayer"):
        m = re.search(r"class %s\(ctypes\.Structure\):\s*_fields_ = \[(.*?)\]\n" % cls, doc, re.S)
        assert m, f"INTEGRATION.md has no {cls} binding"
        names = re.findall(r'\("(\w+)"', m.group(1))
        assert names == [n for n, _ in getattr(nconv_amd._lib, cls)._fields_], cls
