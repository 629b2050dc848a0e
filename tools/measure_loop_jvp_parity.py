#!/usr/bin/env python
"""Dev tool: the provenance of COMPOSED_PATH_ERROR in tests/loop_tangent_np.py (profiles/loop_jvp.md, section 1).

On every case, batch, period count and T of tests/test_gpu_loop_jvp.py: dX and dU0 of closed_loop_jvp(fused=False) -- the loop
composed in torch from SharedModel.solve and SharedModel.plan_jvp, the kernels of the parent commit -- and of the fused path,
cold and warm, against the NumPy restatement of the recursion (tests/loop_tangent_np.py) fed the oracle loop's multipliers,
with seeded tangents on all six operands: max |got - ref| / max(1, |ref|) over the loops whose oracle margin is at least 1e-6
(the loops do not interact, so the others are left out of the comparison only). Prints one JSON line per case and the
markdown table of the profile; the tests' bound is ten times the largest composed-path figure, never looser than 1e-6.
usage: measure_loop_jvp_parity.py [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools.measure_loop_diff_parity import MARGIN, operands  # noqa: E402
from tools.measure_model_loop_parity import shared_model  # noqa: E402

BATCHES, PERIODS = (1, 5, 67), (1, 7)


def tangent_counts(c):
    """The T of the GPU test: one tangent, the x0 Jacobian's nx, and 17 (a second, ragged pass of the kernel)."""
    return tuple(sorted({1, c["nx"], 17}))


def case_reference(name, B, P, T):
    """(case, oracle loop, kept loops, tangents {operand: [B, T, ...]}, the restatement's dict)."""
    import loop_adjoint_np as LA
    import loop_tangent_np as LT
    import model_loop_cases as MC
    import model_loop_np as ML

    c = MC.make(name, B, P)
    ref = ML.oracle_loop(c, P)
    md = ML.condense_lti(c)
    keep = LA.margins(c, ref, md) >= MARGIN
    tan = LT.tangents(c, P, T)
    if c["targets"] is None:
        tan["targets"] = None
    return c, ref, keep, tan, LT.loop_jvp(c, ref, tan, md)


def tangent_args(tan):
    """The d_* arguments of closed_loop_jvp for the tangents of loop_tangent_np.tangents, as float64 device tensors."""
    import torch

    T = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")  # noqa: E731
    return dict(d_x0=T(tan["x0"]), d_goal=T(tan["goal"]), d_targets=T(tan["targets"]), d_disturbance=T(tan["dist"]),
                d_Ap=T(tan["Ap"]), d_Bp=T(tan["Bp"]))


def sensitivities(sm, c, P, tan, **kw):
    """-> (dX, dU0 as NumPy arrays, info) of closed_loop_jvp on a case."""
    from qpmpc_amd import closed_loop_jvp

    ops = operands(c, grad=False)
    _, _, dX, dU0, info = closed_loop_jvp(sm, ops["x0"], P, goal=ops["goal"], targets=ops["targets"], plant=(ops["Ap"], ops["Bp"]),
                                          disturbance=ops["disturbance"], feas_tol=c["tol"], **tangent_args(tan), **kw)
    return dX.cpu().numpy(), dU0.cpu().numpy(), info


def worst(got, want, keep):
    """{record: max |got - ref| / max(1, |ref|)} over the kept loops; got = (dX, dU0), want the restatement's dict."""
    out = {}
    for k, g in zip(("dX", "dU0"), got):
        r = want[k][keep]
        out[k] = float((np.abs(g[keep] - r) / np.maximum(1.0, np.abs(r))).max()) if keep.any() else 0.0
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_loop_jvp_parity.py measures on the GPU only")
    import model_loop_cases as MC

    rows = []
    for name in MC.NAMES + ("triple_infeasible",):
        sm = shared_model(MC.make(name, 67, 7))
        for B in BATCHES:
            for P in PERIODS:
                for T in tangent_counts(MC.make(name, B, P)):
                    c, ref, keep, tan, want = case_reference(name, B, P, T)
                    row = dict(case=name, B=B, P=P, T=T, kept=int(keep.sum()))
                    for mode, kw in (("composed", dict(fused=False)), ("fused_cold", {}), ("fused_warm", dict(warm=True))):
                        dX, dU0, info = sensitivities(sm, c, P, tan, **kw)
                        row[mode] = worst((dX, dU0), want, keep)
                        if mode != "composed":
                            row[mode]["replay_error"] = float(info.replay_error.item())
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    top = lambda r, m: max(v for k, v in r[m].items() if k != "replay_error")  # noqa: E731
    print("| case | B | periods | T | loops kept | composed (fused=False) | fused cold | fused warm |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['B']} | {r['P']} | {r['T']} | {r['kept']} | {top(r, 'composed'):.2e} | {top(r, 'fused_cold'):.2e} | "
              f"{top(r, 'fused_warm'):.2e} |")
    print("largest composed-path error over dX and dU0: %.3e; largest fused: %.3e; largest replay error: %.3e" % (
        max(top(r, "composed") for r in rows), max(max(top(r, "fused_cold"), top(r, "fused_warm")) for r in rows),
        max(max(r["fused_cold"]["replay_error"], r["fused_warm"]["replay_error"]) for r in rows)))


if __name__ == "__main__":
    main()
