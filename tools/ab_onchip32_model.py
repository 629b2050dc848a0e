#!/usr/bin/env python3
"""Dev: the shared-model mode of csrc/mpcqp_duo.hip (17 .. 32 variables on chip, two problems per wavefront, the rows of M and L^-T
read from the factored model) against the other launches that solve the same problems, in one process. The problems share A, B, C,
D, e and the targets (random LTV, qpmpc_amd.workloads.random_ltv) and have x0 (0.1 N(0, 1) around one state) and goal per problem;
e = max over the batch of C x_free + slack, so u = 0 is feasible for every problem and rows bind (13 .. 24 iterations). Launches:
  (a) mpcqp_solve_model_batch with MPCQP_OPT_ON_CHIP_32           the new kernel, bounds from the model
  (b) mpcqp_solve_model_batch, no flag                             today's default model route (the workgroup kernel)
  (c) solve_mpc_batch(flags=OPT_ON_CHIP_32)                        the flagged fused launch: build + factorisation + the same loop
  (d) mpcqp_solve_model_bounds_batch, e per problem (materialised) the new kernel, bounds per problem
Printed per shape and batch: equal statuses, max |dU| of (a), (b), (d) against (c) on the items all solved, mean iterations, and us per
launch of each: the minimum over two alternating rounds of series of back-to-back launches, and the spread (the difference of the
two rounds' minima) a difference between launches has to exceed. Device events around each series; ten launches of warm-up each.
usage: ab_onchip32_model.py [batch ...]   (default 256 4096 16384; on a shared machine one batch per process, each under its own
time limit: timeout -k 10 240 python tools/ab_onchip32_model.py 4096)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
from qpmpc_amd import BatchMPCProblem, PreparedSolve, SharedModel, _capi
from qpmpc_amd.workloads import random_ltv

SHAPES = ((3, 1, 24, 2), (3, 1, 32, 2), (4, 2, 16, 2))

def problems(shape, batch, seed=7, margin=0.1, spread=0.1):
    nx, nu, N, mk = shape
    rng = np.random.default_rng(seed)
    w = random_ltv(rng, 1, nx, nu, N, mk, margin)  # the shared matrices, weights and targets
    x0, goal = w["x0"] + spread * rng.standard_normal((batch, nx)), rng.standard_normal((batch, nx))
    slack = margin * (0.05 + 0.5 * np.abs(rng.standard_normal((N, mk))))
    e, x = np.empty((batch, N, mk)), x0.copy()
    for k in range(N):  # e_k = C_k x_free,k + slack_k for every problem, then the largest over the batch
        e[:, k] = x @ w["C"][0, k].T + slack[k]
        x = x @ w["A"][0, k].T
    e = e.max(axis=0, keepdims=True)
    return BatchMPCProblem(w["A"], w["B"], w["C"], w["D"], e, N, w["wt"], w["wx"], w["wu"], x0, goal_state=goal, target_states=w["targets"])

def series(run, n):
    for _ in range(10): run.launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): run.launch()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

def one(shape, batch, rounds=2):
    bp = problems(shape, batch)
    model = SharedModel(bp)
    own = model.problem_for(bp.initial_state, bp.goal_state, bp.target_states, e=bp.e.expand(batch, -1, -1).contiguous())
    runs = dict(a=model.prepare(bp, return_multipliers=True, flags=_capi.OPT_ON_CHIP_32), b=model.prepare(bp, return_multipliers=True),
                c=PreparedSolve(bp, return_multipliers=True, flags=_capi.OPT_ON_CHIP_32), d=model.prepare(own, return_multipliers=True))
    for r in runs.values(): r.launch()
    torch.cuda.synchronize()
    st = {k: r.status.cpu() for k, r in runs.items()}
    ok = (st["a"] == 0) & (st["b"] == 0) & (st["c"] == 0) & (st["d"] == 0)
    du = {k: ((runs[k].U - runs["c"].U).abs().max(dim=1).values.cpu()[ok].max().item() if ok.any() else float("nan")) for k in "abd"}
    same = all(bool((st[k] == st["c"]).all()) for k in "abd")
    n = 200 if batch <= 4096 else 60
    t = {k: [] for k in runs}
    for _ in range(rounds):  # the four launches alternate
        for k, r in runs.items(): t[k].append(series(r, n))
    cell = lambda k: f"{min(t[k]):.1f} ± {abs(t[k][0] - t[k][1]):.1f}"
    print(f"| {shape} | {batch} | {'yes' if same else 'NO'} ({int(ok.sum())} solved) | {du['a']:.1e} / {du['b']:.1e} / {du['d']:.1e} | {runs['a'].iters.float().mean().item():.2f} |"
          f" {cell('a')} | {cell('b')} | {cell('c')} | {cell('d')} |", flush=True)

if __name__ == "__main__":
    print("| shape (nx, nu, N, mk) | batch | equal status | max dU vs (c): a / b / d | mean iters | (a) model, flag | (b) model, default route | (c) fused, flag | (d) bounds per problem |")
    print("|---|---|---|---|---|---|---|---|---|")
    for bsz in [int(x) for x in sys.argv[1:]] or [256, 4096, 16384]:
        for shape in SHAPES:
            one(shape, bsz)
