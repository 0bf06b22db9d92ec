"""The C host programs of tests/host/ for the *_cpu tests: built with gcc against include/nconv.h, linked to
libnconv.so, run, and their JSON report read; and the layout of a ctypes structure in the report's form."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_report(nconv_amd, tmp_path_factory, name, csrc=False):
    """The report of tests/host/<name>.c (csrc: the package's csrc/ is an include directory too). Skips
    without gcc or without the built library."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    lib = nconv_amd._lib.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("libnconv.so not built")
    exe = str(tmp_path_factory.mktemp("host") / name)
    inc = ["-I", os.path.join(ROOT, "include")]
    if csrc:
        inc += ["-I", os.path.join(os.path.dirname(nconv_amd.__file__), "csrc")]
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", *inc, os.path.join(ROOT, "tests", "host", name + ".c"),
                    "-o", exe, lib, f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
    return json.loads(r.stdout)


def ctypes_layout(struct, c_name):
    """{c_name: [0, size], c_name.field: [offset, size], ...} of a ctypes structure."""
    out = {c_name: [0, ctypes.sizeof(struct)]}
    for f, _ in struct._fields_:
        d = getattr(struct, f)
        out[f"{c_name}.{f}"] = [d.offset, d.size]
    return out
