#!/usr/bin/env python
"""Dev tool: the provenance of PARITY_RTOL in tests/model_loop_cases.py (profiles/model_loop.md, section 1).

On every case, batch and period count of tests/test_gpu_model_loop.py: the error of the per-period path --
ModelClosedLoop.step(1, fused=False), a PreparedModelSolve launch plus the plant step in torch -- and of the fused launch,
cold and warm, against the oracle loop of tests/model_loop_np.py: max |got - ref| / max(1, |ref|) over X and U0, the last
period's multipliers relative to the loop's largest one, iterations, failed periods. Prints one JSON line per case and the
markdown table of the profile; PARITY_RTOL is ten times the largest per-period-path figure.
usage: measure_model_loop_parity.py [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def shared_model(c):
    """The SharedModel of a case of tests/model_loop_cases.py."""
    from qpmpc_amd import BatchMPCProblem, SharedModel

    nx, N = c["nx"], c["N"]
    tmpl = BatchMPCProblem(c["A"], c["B"], c["C"], c["D"], c["e"], N, c["wt"], c["wx"], c["wu"], np.zeros((1, nx)),
                           goal_state=np.zeros((1, nx)), target_states=None if c["targets"] is None else np.zeros((1, N * nx)))
    return SharedModel(tmpl)


def loop_of_case(c, **kw):
    """The ModelClosedLoop of a case: its references, plant, disturbance and tolerance."""
    from qpmpc_amd import ModelClosedLoop

    goal = c["goal"][None] if c["goal_by_period"] else c["goal"]
    tg = c["targets"]
    return ModelClosedLoop(shared_model(c), c["x0"], goal=goal, targets=None if tg is None else (tg[0] if tg.ndim == 2 else tg),
                           plant=(c["Ap"], c["Bp"]), disturbance=c["dist"], feas_tol=c["tol"], **kw)


def rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def main():
    import torch

    import model_loop_cases as MC
    import model_loop_np as ML

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_model_loop_parity.py measures on the GPU only")
    rows = []
    for name in MC.NAMES + ("triple_infeasible",):
        for B in MC.BATCHES:
            for P in MC.PERIODS + ((MC.WARM_PERIODS,) if name == "triple" and B == 67 else ()):
                if name == "triple_infeasible" and (B, P) != (67, 7):
                    continue
                c = MC.make(name, B, P)
                ref = ML.oracle_loop(c, P)
                row = dict(case=name, B=B, P=P, oracle_iters=int(ref["iters"].sum()), oracle_failed=int(ref["failed"].sum()))
                ok = ref["status"][-1] == 0
                lo = ref["lam"][-1][ok]
                lscale = np.maximum(1.0, np.abs(lo).max(axis=1, keepdims=True)) if lo.size else 1.0
                for mode in ("by_hand", "fused_cold", "fused_warm"):
                    lp = loop_of_case(c, warm=(mode == "fused_warm"))
                    if mode == "by_hand":
                        lp.step(P, fused=False)
                    else:
                        lp.step(P)
                    torch.cuda.synchronize()
                    st = lp.stats()
                    lam = lp.lam.cpu().numpy()[ok]
                    row[mode] = dict(X=rel(lp.X.cpu().numpy(), ref["X"]), U0=rel(lp.U0.cpu().numpy(), ref["U0"]),
                                     lam=float((np.abs(lam - lo) / lscale).max()) if lo.size else 0.0,
                                     failed=st["failed"], iters=int(lp.iters_total.item()), recold=st["resolved_cold"])
                print(json.dumps(row), flush=True)
                rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    print("| case | B | periods | per-period path | fused cold | fused warm | last plan's lam: per-period / cold / warm | "
          "iterations oracle / per-period / cold / warm | warm periods re-solved cold | failed periods GPU / oracle |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        bh, fc, fw = r["by_hand"], r["fused_cold"], r["fused_warm"]
        print(f"| {r['case']} | {r['B']} | {r['P']} | {max(bh['X'], bh['U0']):.2e} | {max(fc['X'], fc['U0']):.2e} | "
              f"{max(fw['X'], fw['U0']):.2e} | {bh['lam']:.1e} / {fc['lam']:.1e} / {fw['lam']:.1e} | "
              f"{r['oracle_iters']} / {bh['iters']} / {fc['iters']} / {fw['iters']} | {fw['recold']} | {fc['failed']} / {r['oracle_failed']} |")
    print("largest per-period-path error over X and U0: %.3e; over the last plan's multipliers: %.3e" % (
        max(max(r["by_hand"]["X"], r["by_hand"]["U0"]) for r in rows), max(r["by_hand"]["lam"] for r in rows)))


if __name__ == "__main__":
    main()
