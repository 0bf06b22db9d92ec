#!/usr/bin/env python3
"""kappa_ref of the element-wise gradient bounds (tests/test_gpu_layers.py,
tests/test_gpu_dense_train.py): what the reference's own float32 arithmetic costs, per element,
relative to the gradient majorant.

For every backward case of the layer tests (nconv_cases.LAYER_CASES, PHASE_CASES, the standalone
module's two sizes) this runs the reference's op sequence (nconv_cases.oracle_layer: glue +
NConv2d.forward) in float32 with torch autograd on the CPU, compares each of the six gradients with
the float64 run of the same fp32-rounded operands, and records

    kappa_ref = max_i |g32_i - g64_i| / A_i,      A = nconv_cases.nconv2d_backward_majorant

per case and tensor. The dense cases (dense_cases.CASES) record the same for the weight and bias
gradients of F.conv2d / F.conv_transpose2d, majorant wgrad(|x|, |g|) and sum |g|. The GPU tests hold
the kernels to kappa = 4 x kappa_ref (nconv_cases.kappa). Written to
tests/golden/bwd_bound_kappa.json.

    python tools/bwd_kappa.py        # CPU, deterministic, < 1 min; test infrastructure
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dense_cases as DC  # noqa: E402
import nconv_cases as NC  # noqa: E402


def compute(sections=("layer", "phase", "module", "dense")):
    out = {}
    if "layer" in sections:
        out["layer"] = {c[0]: NC.layer_bwd_problem(c).kappa_ref() for c in NC.LAYER_CASES}
    if "phase" in sections:
        out["phase"] = {c[0]: NC.phase_bwd_problem(c).kappa_ref() for c in NC.PHASE_CASES}
    if "module" in sections:
        w, b = NC.module_init_weights()
        out["module"] = {f"{H}x{W}": NC.module_bwd_problem(H, W, w, b).kappa_ref() for H, W in NC.MODULE_SIZES}
    if "dense" in sections:
        out["dense"] = {DC.case_id(c): DC.DenseProblem(c).kappa_ref() for c in DC.CASES}
    return {s: {k: {t: float(f"{v:.4e}") for t, v in d.items()} for k, d in sec.items()} for s, sec in out.items()}


def main():
    import torch
    torch.set_num_threads(1)  # the float32 sums' order, and so the last digits, follow the thread count
    out = {"source": "max_i |g32_i - g64_i| / A_i of the reference's op sequence in float32 (CPU autograd) against "
                     "float64 of the same fp32-rounded operands; written by tools/bwd_kappa.py"}
    out.update(compute())
    path = os.path.join(ROOT, "tests", "golden", "bwd_bound_kappa.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    worst = max(v for s in out.values() if isinstance(s, dict) for d in s.values() for v in d.values())
    print(f"wrote {path}: largest kappa_ref {worst:.2e}")


if __name__ == "__main__":
    main()
