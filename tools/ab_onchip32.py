#!/usr/bin/env python3
"""Dev: MPCQP_OPT_ON_CHIP_32 (csrc/mpcqp_duo.hip: 17 .. 32 variables on chip, two problems per wavefront) against the default
dispatch on the same seeded problems in one process: equal statuses, max |dU|, mean iterations, us per launch (min and median over
alternating series of back-to-back launches). The default route is timed twice per round; the difference of the two is the spread
a difference between the routes has to exceed. Shapes: the triple integrator of BASELINE config 2 at N = 17, 20, 24, 32 (two rows
per step) and random LTV families (4, 2, 12, 2), (4, 2, 16, 2), (3, 1, 20, 3) with C and D rows and a stage cost.
usage: ab_onchip32.py [batch ...]   (default 256 4096 16384)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
from qpmpc_amd import PreparedSolve, workloads as W, _capi
from qpmpc_amd.workloads import random_ltv

def triple(batch, N, seed=20250614):
    """config 2's problems (workloads.triple_integrator_batch) with the horizon of one second cut into N steps"""
    A, B, C, e = W.triple_integrator_matrices(N)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-0.5, 0.5, batch), rng.uniform(-0.5, 0.5, batch), rng.uniform(-2.5, 2.5, batch)], 1)
    goal = np.stack([rng.uniform(0.5, 1.5, batch), np.zeros(batch), np.zeros(batch)], 1)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (batch, N) + a.shape))  # (one block per problem and step, as config 2)
    return dict(A=rep(A), B=rep(B), C=rep(C), D=None, e=rep(e), N=N, wt=1.0, wx=None, wu=1e-6, x0=x0, goal=goal, targets=None)

def series(run, n):
    for _ in range(10): run.launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): run.launch()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

def one(name, w, batch, rounds=5):
    bp = W.to_batch_problem(w)
    a = PreparedSolve(bp, return_multipliers=True, flags=_capi.OPT_ON_CHIP_32)
    b = PreparedSolve(bp, return_multipliers=True)
    a.launch(); b.launch(); torch.cuda.synchronize()
    sa, sb = a.status.cpu(), b.status.cpu()
    ok = (sa == 0) & (sb == 0)
    du = (a.U - b.U).abs().max(dim=1).values.cpu()
    n = 100 if batch <= 4096 else 30
    ta, tb, tc = [], [], []
    for _ in range(rounds):  # flagged, default, default again: the three series alternate
        ta.append(series(a, n)); tb.append(series(b, n)); tc.append(series(b, n))
    med = lambda t: sorted(t)[len(t) // 2]
    spread = abs(min(tb) - min(tc))
    gain = min(min(tb), min(tc)) - min(ta)
    verdict = "no difference" if abs(gain) <= spread else (f"{min(min(tb), min(tc)) / min(ta):.2f}x faster" if gain > 0 else f"{min(ta) / min(min(tb), min(tc)):.2f}x SLOWER")
    print(f"| {name} | {batch} | {int((sa == sb).sum())}/{batch} ({int((sa == 0).sum())} solved) | {du[ok].max().item() if ok.any() else float('nan'):.1e} |"
          f" {a.iters.float().mean().item():.2f} | {min(ta):.1f} / {med(ta):.1f} | {min(tb):.1f} / {med(tb):.1f} | {min(tc):.1f} / {med(tc):.1f} | {spread:.1f} | {verdict} |", flush=True)

if __name__ == "__main__":
    print("| shape (nx, nu, N, mk) | batch | equal status | max dU | mean iters | flagged us min / med | default us min / med | default again | spread | flagged vs default |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for bsz in [int(x) for x in sys.argv[1:]] or [256, 4096, 16384]:
        for N in (17, 20, 24, 32):
            one(f"triple integrator (3, 1, {N}, 2)", triple(bsz, N), bsz)
        for nx, nu, N, mk in ((4, 2, 12, 2), (4, 2, 16, 2), (3, 1, 20, 3)):
            one(f"random LTV ({nx}, {nu}, {N}, {mk})", random_ltv(np.random.default_rng(3), bsz, nx, nu, N, mk, 0.3), bsz)
