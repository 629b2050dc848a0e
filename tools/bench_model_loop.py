#!/usr/bin/env python
"""Dev tool: where the fused closed loop of a shared model pays (profiles/model_loop.md).

Triple-integrator family (nx = 3, nu = 1, N = 16, two state rows per step: n = 16, m = 32), plant = model, a constant
disturbance on position and velocity, 50 periods per episode from seeded initial states, B loops. Three ways to run an
episode, alternated in ONE process after a warm-up of each:
  by_hand     ModelClosedLoop.step(1, fused=False) per period: a PreparedModelSolve launch plus the plant step in torch
              (what users wrote before; the kernels of the parent commit)
  fused_cold  ModelClosedLoop.step(50): one launch of mpcqp_model_periods_batch
  fused_warm  the same with warm=True
Every timing is a window of whole episodes between two device events, sized to at least --window seconds from a first
episode, repeated --repeats times (alternating the modes) to show the spread; us per period = window / (episodes * 50).
usage: bench_model_loop.py [--batches 256,1024,4096,65536] [--periods 50] [--window 0.3] [--repeats 5] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_loops(B, seed=11):
    import torch  # noqa: F401

    from qpmpc_amd import BatchMPCProblem, ModelClosedLoop, SharedModel
    from qpmpc_amd.workloads import triple_integrator_matrices

    A, Bm, Cm, e = triple_integrator_matrices(16)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), rng.uniform(-2.5, 2.5, B)], 1)
    goal = np.stack([rng.uniform(.5, 1.5, B), np.zeros(B), np.zeros(B)], 1)
    dist = 1e-3 * rng.standard_normal((B, 3))
    dist[:, 2] = 0.0
    sm = SharedModel(BatchMPCProblem(A, Bm, Cm, None, e, 16, 1.0, None, 1e-6, np.zeros((1, 3)), goal_state=np.zeros((1, 3))))
    mk = lambda warm: ModelClosedLoop(sm, x0, goal=goal, disturbance=dist, warm=warm, record=False)  # noqa: E731
    return x0, {"by_hand": mk(False), "fused_cold": mk(False), "fused_warm": mk(True)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024,4096,65536")
    ap.add_argument("--periods", type=int, default=50)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_model_loop.py measures on the GPU only")
    P, rows = a.periods, []
    for B in [int(b) for b in a.batches.split(",")]:
        x0, loops = make_loops(B)
        x0d = torch.as_tensor(x0, dtype=torch.float64, device="cuda")

        def episode(name):
            lp = loops[name]
            lp.states.copy_(x0d)
            if name == "by_hand":
                for _ in range(P):
                    lp.step(1, fused=False)
            else:
                lp.step(P)

        def timed(name, episodes):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(episodes):
                episode(name)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e-3

        row = dict(B=B, periods=P, modes={})
        finals = {}
        for name, lp in loops.items():  # warm-up, iteration totals and final states of ONE episode
            episode(name)
            lp._loopstats.zero_()
            episode(name)
            torch.cuda.synchronize()
            st = lp._loopstats.sum(0).tolist()
            finals[name] = lp.states.clone()
            one = timed(name, 1)
            row["modes"][name] = dict(failed=st[0], iters=st[1], resolved_cold=st[2],
                                      episodes=max(1, int(np.ceil(a.window / max(one, 1e-6)))), us_per_period=[])
        row["max_state_diff_vs_by_hand"] = {k: float((finals[k] - finals["by_hand"]).abs().max()) for k in finals}
        for _ in range(a.repeats):
            for name in loops:
                m = row["modes"][name]
                m["us_per_period"].append(timed(name, m["episodes"]) / (m["episodes"] * P) * 1e6)
        for name, m in row["modes"].items():
            v = np.array(m["us_per_period"])
            m["median"], m["min"], m["max"] = float(np.median(v)), float(v.min()), float(v.max())
            print(f"B={B:6d} {name:11s} {m['median']:9.2f} us/period (min {m['min']:.2f}, max {m['max']:.2f}; {m['episodes']} episodes "
                  f"per window) iterations {m['iters']} failed {m['failed']} re-solved cold {m['resolved_cold']}", flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    print("| B | by hand (us/period) | fused cold | fused warm | iterations by hand / cold / warm | re-solved cold |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        m = r["modes"]
        f = lambda k: f"{m[k]['median']:.1f} ({m[k]['min']:.1f} .. {m[k]['max']:.1f})"  # noqa: E731
        print(f"| {r['B']} | {f('by_hand')} | {f('fused_cold')} | {f('fused_warm')} | "
              f"{m['by_hand']['iters']} / {m['fused_cold']['iters']} / {m['fused_warm']['iters']} | {m['fused_warm']['resolved_cold']} |")


if __name__ == "__main__":
    main()
