#!/usr/bin/env python3
"""Dev: capture the goldens of tests/test_gpu_onchip32_model.py on a GPU, from the commit BEFORE csrc/mpcqp_duo.hip got its
shared-model mode (check that commit out, build, copy this file and the helper modules of tests/ it imports next to it, run):

  tests/golden/onchip32_fused_parent.npz          U, lam, status, iters of the flagged fused launch (MPCQP_OPT_ON_CHIP_32) on the
                                                  families FUSED_GOLDEN of onchip32_cases (61 problems each)
  tests/golden/onchip32_model_default_parent.npz  the same four of mpcqp_solve_model_batch without a flag on the nine problems of
                                                  variant 3 of (3, 1, 24, 2): the default route of shared-model solves

Both launches are those of tests/test_gpu_onchip32_model.py (fused_outputs, default_route_outputs: the same calls on the same
cases), so the goldens are what those calls returned there. Data only.
usage: gen_golden_onchip32_parent.py [output directory]   (default tests/golden)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import onchip32_cases as OC
import onchip32_model_cases as MC
import operand_layouts as OL
from guarded_launch import F, ModelCase, _flag, solve_outputs

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out, exist_ok=True)
    fused = {}
    for fam in MC.FUSED_GOLDEN:
        tag = "x".join(str(v) for v in fam[0])
        for name, arr in zip(("U", "lam", "status", "iters"), solve_outputs(OC.family(*fam), _flag())):
            fused[f"{name}_{tag}"] = arr
        print(f"fused {fam}: status {np.unique(fused['status_' + tag]).tolist()}, iters mean {fused['iters_' + tag].mean():.2f}")
    np.savez(os.path.join(out, "onchip32_fused_parent.npz"), **fused)
    d = ModelCase(MC.case(MC.PLAIN, MC.DEFAULT_GOLDEN_VARIANT)[0], OL.model_pads(MC.DEFAULT_GOLDEN_VARIANT)).run(F, 0, bounds=False)
    print(f"model default route: status {d['status'].tolist()}, iters {d['iters'].tolist()}")
    np.savez(os.path.join(out, "onchip32_model_default_parent.npz"), **{k: d[k] for k in ("U", "lam", "status", "iters")})
    print("written to", out)
