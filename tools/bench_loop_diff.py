#!/usr/bin/env python
"""Dev tool: what the fused closed-loop adjoint costs against the loop composed in torch (profiles/loop_diff.md, section 2).

Triple-integrator family of tools/bench_model_loop.py (nx = 3, nu = 1, N = 16: n = 16, m = 32), plant = model, 50 periods
from seeded initial states, B loops; x0 and the goal require grad and the loss is the squared distance of the last state to
the goal plus 1e-4 |U0|^2. One step = forward + backward:
  composed  closed_loop_diff(fused=False): SharedModel.solve_diff and the plant step per period, autograd's chain back
  fused     closed_loop_diff(fused=True): one mpcqp_model_periods_batch launch, one replay launch, one
            mpcqp_model_periods_vjp_batch launch
and the fused step split into its three launches, timed one by one through the same entry points. Every figure is the median of
--steps steps after --warmup, device-event time and wall time (perf_counter around a synchronised step), alternating the modes.
usage: bench_loop_diff.py [--batches 256,1024,4096] [--periods 50] [--steps 20] [--warmup 3] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(B, seed=11):
    import torch

    from qpmpc_amd import BatchMPCProblem, SharedModel
    from qpmpc_amd.workloads import triple_integrator_matrices

    A, Bm, Cm, e = triple_integrator_matrices(16)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), rng.uniform(-2.5, 2.5, B)], 1)
    goal = np.stack([rng.uniform(.5, 1.5, B), np.zeros(B), np.zeros(B)], 1)
    dist = 1e-3 * rng.standard_normal((B, 3))
    dist[:, 2] = 0.0
    sm = SharedModel(BatchMPCProblem(A, Bm, Cm, None, e, 16, 1.0, None, 1e-6, np.zeros((1, 3)), goal_state=np.zeros((1, 3))))
    T = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")  # noqa: E731
    return sm, T(x0), T(goal), T(dist)


def timed(fn, steps, warmup):
    """(median device-event us, median wall us) of fn()."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        wall.append((time.perf_counter() - w0) * 1e6)
        dev.append(t0.elapsed_time(t1) * 1e3)
    return float(np.median(dev)), float(np.median(wall))


def main():
    import torch

    from qpmpc_amd import ModelClosedLoop, closed_loop_diff, loop_diff

    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024,4096")
    ap.add_argument("--periods", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loop_diff.py measures on the GPU only")
    P, rows = a.periods, []
    for B in [int(b) for b in a.batches.split(",")]:
        sm, x0, goal, dist = make(B)
        grads = {}

        def step(fused):
            x, g = x0.clone().requires_grad_(), goal.clone().requires_grad_()
            X, U0, info = closed_loop_diff(sm, x, P, goal=g, disturbance=dist, fused=fused)
            loss = ((X[:, -1] - g) ** 2).sum() + 1e-4 * (U0 ** 2).sum()
            grads[fused] = torch.autograd.grad(loss, (x, g))
            return info

        # the fused step's three launches, one by one
        loop = ModelClosedLoop(sm, x0, goal=goal, disturbance=dist)
        loop.step(P)
        X, U0 = loop.X, loop.U0
        lam, status, err, _ = loop_diff._replay(sm, loop, X, U0, P)
        gX, gU0 = torch.randn_like(X), torch.randn_like(U0)

        def forward():
            lp = ModelClosedLoop(sm, x0, goal=goal, disturbance=dist)
            lp.step(P)

        row = dict(B=B, periods=P)
        for name, fn in (("composed", lambda: step(False)), ("fused", lambda: step(True)), ("fused_forward", forward),
                         ("fused_replay", lambda: loop_diff._replay(sm, loop, X, U0, P)),
                         ("fused_backward", lambda: loop_diff.loop_vjp(sm, loop, lam, status, X, U0, gX, gU0, {"x0", "goal"}))):
            dev, wall = timed(fn, a.steps, a.warmup)
            row[name] = dict(device_us=dev, wall_us=wall)
            print(f"B={B:5d} {name:15s} device {dev:10.1f} us  wall {wall:10.1f} us", flush=True)
        info = step(True)
        step(False)
        torch.cuda.synchronize()
        row["replay_error"] = float(info.replay_error.item())
        row["failed_periods"] = int(info.failed.item())
        row["max_grad_diff_fused_vs_composed"] = max(
            float(((f - c).abs() / c.abs().clamp_min(1.0)).max()) for f, c in zip(grads[True], grads[False]))
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    print("| B | composed: device / wall (ms) | fused: device / wall (ms) | ratio device / wall | fused forward / replay / backward "
          "kernel, device (us) | replay error | fused against composed gradients |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        c, f = r["composed"], r["fused"]
        print(f"| {r['B']} | {c['device_us'] / 1e3:.2f} / {c['wall_us'] / 1e3:.2f} | {f['device_us'] / 1e3:.3f} / {f['wall_us'] / 1e3:.3f} | "
              f"{c['device_us'] / f['device_us']:.1f}x / {c['wall_us'] / f['wall_us']:.1f}x | {r['fused_forward']['device_us']:.0f} / "
              f"{r['fused_replay']['device_us']:.0f} / {r['fused_backward']['device_us']:.0f} | {r['replay_error']:.1e} | "
              f"{r['max_grad_diff_fused_vs_composed']:.1e} |")


if __name__ == "__main__":
    main()
