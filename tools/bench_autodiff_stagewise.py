#!/usr/bin/env python3
"""The stage-wise adjoint (solve_mpc_batch_diff(..., adjoint="stagewise")) timed with device events (median of --steps
after --warmup).

    python tools/bench_autodiff_stagewise.py [--steps 20] [--warmup 5] [--cases a,b] [--out FILE]

Per case: the forward (solve_mpc_batch), the differentiable forward (solve_mpc_batch_diff with x0 and the goal requiring
grad) and its backward through mpcqp_plan_vjp_stagewise_batch, in microseconds per batch; where the condensed adjoint
applies (n <= 128) its backward on the same plan as well. Cases: the BASELINE config-5 shape (synthetic LTV, nx 12, nu 4,
N 64, float32 storage, 8192 problems), a triple integrator with N = 256 (4096 problems), the wheeled inverted pendulum
with N = 200 (1024 problems; T = 0.005 s, where the condensed P of N = 200 is positive definite), BASELINE config 2 and
the pendulum with N = 50. A kernel split comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from qpmpc_amd import solve_mpc_batch, solve_mpc_batch_diff, workloads as W  # noqa: E402


def _triple(batch, N, seed=7):
    A, B, C, e = W.triple_integrator_matrices(N)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-0.5, 0.5, batch), rng.uniform(-0.5, 0.5, batch), rng.uniform(-2.5, 2.5, batch)], 1)
    goal = np.stack([rng.uniform(0.5, 1.5, batch), np.zeros(batch), np.zeros(batch)], 1)
    return W._pack(A, B, C, None, e, N, 1.0, None, 1e-6, x0, goal, name=f"triple_integrator_N{N}")


CASES = {
    "config5_shape_f32": lambda: (W.synthetic_ltv_batch(8192), torch.float32),
    "triple_integrator_N256": lambda: (_triple(4096, 256), torch.float64),
    "wip_N200": lambda: (W.wip_batch(1024, N=200, sampling_period=0.005), torch.float64),
    "config2_triple_integrator": lambda: (W.triple_integrator_batch(4096), torch.float64),
    "wip_N50": lambda: (W.wip_batch(1024, N=50), torch.float64),
}


def _median_us(fn, steps, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def run_case(name, steps, warmup):
    w, dt = CASES[name]()
    bp = W.to_batch_problem(w, dtype=dt)
    x0 = torch.as_tensor(w["x0"], dtype=dt, device=bp.device).clone().requires_grad_()
    goal = torch.as_tensor(w["goal"], dtype=dt, device=bp.device).clone().requires_grad_()
    gU = torch.randn((bp.batch_size, bp.nb_timesteps, bp.input_dim), dtype=dt, device=bp.device)
    held = {}

    def forward(adjoint):
        def f():
            held["U"], _, held["plan"] = solve_mpc_batch_diff(bp, initial_state=x0, goal_state=goal, adjoint=adjoint)
        return f

    def backward():
        x0.grad = goal.grad = None
        held["U"].backward(gU)

    fwd = _median_us(lambda: solve_mpc_batch(bp), steps, warmup)
    dfwd = _median_us(forward("stagewise"), steps, warmup)
    bwd = _median_us(backward, steps, warmup, before=forward("stagewise"))
    plan = held["plan"]
    active = (plan.multipliers > 0).sum(dim=1) if plan.multipliers is not None else torch.zeros(1)
    row = dict(case=name, batch=bp.batch_size, nx=bp.state_dim, nu=bp.input_dim, N=bp.nb_timesteps,
               n=bp.nb_variables, m=bp.nb_constraints, dtype=str(dt).replace("torch.", ""),
               solved=float((plan.status == 0).float().mean()), vjp_ok=float((plan.vjp_status == 0).float().mean()),
               active_rows_max=int(active.max()), active_rows_mean=round(float(active.float().mean()), 1),
               forward_us=round(fwd[0], 2), diff_forward_us=round(dfwd[0], 2), backward_stagewise_us=round(bwd[0], 2),
               backward_stagewise_min_max_us=[round(bwd[1], 2), round(bwd[2], 2)])
    if bp.nb_variables <= 128:
        cond = _median_us(backward, steps, warmup, before=forward("condensed"))
        row.update(backward_condensed_us=round(cond[0], 2), stagewise_over_condensed=round(bwd[0] / cond[0], 3))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autodiff_stagewise.py needs a GPU (no CPU timing is reported)")
    rows = []
    for name in args.cases.split(","):
        rows.append(run_case(name, args.steps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
