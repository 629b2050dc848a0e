#!/usr/bin/env python3
"""Writes tests/golden/second_opinion_narrow.npz: one nearly fully active problem (nx <= 4, nu <= 2, n = N nu in 17..128) on which
the narrow stage-wise kernel alone ends unsolved although the oracle solves it, so mpcqp_build_solve_batch answers SOLVED only through
its second opinion (the wide kernel behind the narrow one). The problem is item 41 of the stress_tight narrow family at STRESS_TIGHT
0.05, seed 4012 (qpmpc_amd/workloads.py: tight_ltv("narrow", default_rng(4012), 64, 0.05)); the narrow kernel alone (a KEEP_FACTOR launch
before the second opinion applied to it) ended it MPCQP_MAX_ITER after 796 iterations. Stored with the oracle's plan, multipliers and
status. CPU only: usage: gen_golden_second_opinion.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import oracle
from qpmpc_amd.workloads import tight_ltv

SEED, BATCH, TIGHT, ITEM = 4012, 64, 0.05, 41

if __name__ == "__main__":
    w = tight_ltv("narrow", np.random.default_rng(SEED), BATCH, TIGHT)
    one = {k: (v[ITEM:ITEM + 1].copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    U, lam, st, it = oracle.solve_workload(one)
    assert st[0] == 0, st
    out = os.path.join(ROOT, "tests", "golden", "second_opinion_narrow.npz")
    np.savez(out, A=one["A"], B=one["B"], C=one["C"], D=one["D"], e=one["e"], x0=one["x0"], goal=one["goal"],
             targets=one["targets"], N=one["N"], wt=one["wt"], wx=one["wx"], wu=one["wu"], U=U[0], lam=lam[0], status=st[0],
             seed=SEED, item=ITEM, tight=TIGHT)
    print(out, "n =", U.shape[1], "active rows", int((lam[0] > 0).sum()))
