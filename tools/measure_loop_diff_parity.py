#!/usr/bin/env python
"""Dev tool: the provenance of COMPOSED_PATH_ERROR in tests/loop_adjoint_np.py (profiles/loop_diff.md, section 1).

On every case, batch and period count of tests/test_gpu_loop_diff.py: the gradients of closed_loop_diff(fused=False) -- the
loop composed in torch from SharedModel.solve_diff, the kernels of the parent commit -- and of the fused path, cold and warm,
against the NumPy restatement of the recursion (tests/loop_adjoint_np.py) fed the oracle loop's multipliers:
max |got - ref| / max(1, |ref|) over every gradient (x0, goal, targets, disturbance, Ap, Bp), over the loops whose oracle margin
is at least 1e-6 (the others get zero cotangents: the loops do not interact, so they drop out of every sum over the batch).
Prints one JSON line per case and the markdown table of the profile; the tests' bound is ten times the largest
composed-path figure, never looser than 1e-6.
usage: measure_loop_diff_parity.py [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools.measure_model_loop_parity import shared_model  # noqa: E402

NAMES = ("x0", "goal", "targets", "disturbance", "Ap", "Bp")
MARGIN = 1e-6  # loops compared on the GPU: strictly complementary by this much in every period (loop_adjoint_np.margins)


def operands(c, grad=True):
    """The arguments of closed_loop_diff for a case of tests/model_loop_cases.py, as float64 device tensors."""
    import torch

    T = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda",  # noqa: E731
                                                      requires_grad=grad)
    tg = c["targets"]
    return dict(x0=T(c["x0"]), goal=T(c["goal"][None] if c["goal_by_period"] else c["goal"]),
                targets=T(None if tg is None else (tg[0] if tg.ndim == 2 else tg)), disturbance=T(c["dist"]),
                Ap=T(c["Ap"]), Bp=T(c["Bp"]))


def reduced_reference(c, g):
    """loop_adjoint_np.loop_vjp's per-loop gradients reduced to the shapes of `operands`: the batch sum for what the batch
    shares, the period sum for what is constant in time."""
    tg = c["targets"]
    out = dict(x0=g["x0"], disturbance=g["states"][:, 1:])
    out["goal"] = g["goal"].sum(0, keepdims=True) if c["goal_by_period"] else g["goal"].sum(1)
    out["targets"] = None if tg is None else (g["targets"].sum((0, 1)) if tg.ndim == 2 else g["targets"])
    for k in ("Ap", "Bp"):
        out[k] = g[k] if c[k].ndim == 3 else g[k].sum(0)
    return out


def gradients(sm, c, ops, P, gX, gU0, **kw):
    """-> (dict of gradients as NumPy arrays, info, X, U0) of loss = <gX, X> + <gU0, U0> through closed_loop_diff."""
    import torch

    from qpmpc_amd import closed_loop_diff

    X, U0, info = closed_loop_diff(sm, ops["x0"], P, goal=ops["goal"], targets=ops["targets"], plant=(ops["Ap"], ops["Bp"]),
                                   disturbance=ops["disturbance"], feas_tol=c["tol"], **kw)
    loss = (X * torch.as_tensor(gX, device="cuda")).sum() + (U0 * torch.as_tensor(gU0, device="cuda")).sum()
    names = [k for k in NAMES if ops[k] is not None]
    grads = torch.autograd.grad(loss, [ops[k] for k in names], allow_unused=True)
    return {k: (None if g is None else g.cpu().numpy()) for k, g in zip(names, grads)}, info, X, U0


def worst(got, ref):
    """{name: max |got - ref| / max(1, |ref|)} over the gradients both have."""
    out = {}
    for k, r in ref.items():
        if r is None or got.get(k) is None:
            continue
        out[k] = float((np.abs(got[k].reshape(r.shape) - r) / np.maximum(1.0, np.abs(r))).max())
    return out


def case_reference(name, B, P):
    """(case, oracle loop, kept loops, gX, gU0, reduced restatement) -- the cotangents of loops under MARGIN are zero."""
    import loop_adjoint_np as LA
    import model_loop_cases as MC
    import model_loop_np as ML

    c = MC.make(name, B, P)
    ref = ML.oracle_loop(c, P)
    md = ML.condense_lti(c)
    keep = LA.margins(c, ref, md) >= MARGIN
    gX, gU0 = LA.cotangents(c, P, ref)
    gX[~keep] = 0.0
    gU0[~keep] = 0.0
    return c, ref, keep, gX, gU0, reduced_reference(c, LA.loop_vjp(c, ref, gX, gU0, md))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_loop_diff_parity.py measures on the GPU only")
    import model_loop_cases as MC

    rows = []
    for name in MC.NAMES + ("triple_infeasible",):
        for B in (1, 5, 67):
            for P in (1, 7):
                c, ref, keep, gX, gU0, want = case_reference(name, B, P)
                sm = shared_model(c)
                row = dict(case=name, B=B, P=P, kept=int(keep.sum()))
                for mode, kw in (("composed", dict(fused=False)), ("fused_cold", {}), ("fused_warm", dict(warm=True))):
                    got, info, _, _ = gradients(sm, c, operands(c), P, gX, gU0, **kw)
                    row[mode] = worst(got, want)
                    if mode != "composed":
                        row[mode]["replay_error"] = float(info.replay_error.item())
                print(json.dumps(row), flush=True)
                rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    top = lambda r, m: max(v for k, v in r[m].items() if k != "replay_error")  # noqa: E731
    print("| case | B | periods | loops kept | composed (fused=False) | fused cold | fused warm | replay error cold / warm |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['B']} | {r['P']} | {r['kept']} | {top(r, 'composed'):.2e} | {top(r, 'fused_cold'):.2e} | "
              f"{top(r, 'fused_warm'):.2e} | {r['fused_cold']['replay_error']:.1e} / {r['fused_warm']['replay_error']:.1e} |")
    print("largest composed-path error over every gradient: %.3e; largest fused: %.3e; largest replay error: %.3e" % (
        max(top(r, "composed") for r in rows), max(max(top(r, "fused_cold"), top(r, "fused_warm")) for r in rows),
        max(max(r["fused_cold"]["replay_error"], r["fused_warm"]["replay_error"]) for r in rows)))


if __name__ == "__main__":
    main()
