#!/usr/bin/env python3
"""kappa_ref of the element-wise forward bounds (tests/test_gpu_layers.py): what the reference's
own float32 arithmetic costs, per element, relative to the forward majorant.

For every forward case of the layer tests (nconv_cases.LAYER_CASES, PHASE_CASES, FWD_SLICE_CASES)
this runs the reference's op sequence (nconv_cases.oracle_layer: glue + NConv2d.forward) in float32
on the CPU, compares both outputs with the float64 run of the same fp32-rounded operands, and records

    kappa_ref = max_i |out32_i - out64_i| / A_i,      A = nconv_cases.nconv2d_forward_majorant

per case and output (y, cout). The GPU tests hold the kernels to kappa = 4 x kappa_ref
(nconv_cases.kappa). Written to tests/golden/fwd_bound_kappa.json.

    python tools/fwd_kappa.py        # CPU, deterministic, ~1 min; test infrastructure
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import nconv_cases as NC  # noqa: E402

SECTIONS = {"layer": lambda: [c[0] for c in NC.LAYER_CASES], "phase": lambda: [c[0] for c in NC.PHASE_CASES],
            "slice": lambda: [e[2][0] for e in NC.FWD_SLICE_CASES]}


def compute(sections=("layer", "phase", "slice")):
    out = {s: {n: NC.fwd_problem(s, n).kappa_ref() for n in SECTIONS[s]()} for s in sections}
    return {s: {k: {t: float(f"{v:.4e}") for t, v in d.items()} for k, d in sec.items()} for s, sec in out.items()}


def main():
    import torch
    torch.set_num_threads(1)  # the float32 sums' order, and so the last digits, follow the thread count
    out = {"source": "max_i |out32_i - out64_i| / A_i of the reference's op sequence in float32 (CPU) against "
                     "float64 of the same fp32-rounded operands; written by tools/fwd_kappa.py"}
    out.update(compute())
    path = os.path.join(ROOT, "tests", "golden", "fwd_bound_kappa.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    vals = [v for s in out.values() if isinstance(s, dict) for d in s.values() for v in d.values()]
    print(f"wrote {path}: kappa_ref {min(vals):.2e} ... {max(vals):.2e}")


if __name__ == "__main__":
    main()
