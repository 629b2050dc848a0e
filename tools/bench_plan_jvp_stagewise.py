#!/usr/bin/env python3
"""The feedback Jacobian dU/dx0 at any horizon, plan_jacobian(formulation="stagewise"), timed with device events (median
of --steps after --warmup) beside one stage-wise backward on the same plan:

    python tools/bench_plan_jvp_stagewise.py [--steps 20] [--warmup 5] [--cases a,b] [--out FILE]

Cases: the five of tools/bench_autodiff_stagewise.py (the config-5 shape in float32 storage x 8192, a triple integrator with
N = 256 x 4096, the wheeled inverted pendulum with N = 200 x 1024 at T = 0.005 s, BASELINE config 2 x 4096, the pendulum
with N = 50 x 1024). Per case, on one plan solved with multipliers, in microseconds per batch:
  - jacobian_stagewise_us: plan_jacobian(bp, plan, formulation="stagewise"): mpcqp_plan_jvp_stagewise_batch with nx shared
    tangents (its host side included: the max_active sync, the workspace, the casts);
  - backward_stagewise_us: one mpcqp_plan_vjp_stagewise_batch on the same plan (g_x0 and g_goal), the yardstick: the
    Jacobian shares its factorisation phases and replaces its two sweeps by nx side by side, so about 1.5 x is expected,
    against the n x of a Jacobian assembled from VJPs;
  - jacobian_condensed_us: plan_jacobian(bp, plan) where n <= 128.
A kernel split comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_autodiff_stagewise import CASES  # noqa: E402
from qpmpc_amd import autodiff, plan_jacobian, solve_mpc_batch, workloads as W  # noqa: E402


def _median_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
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
    Bn, n, nx = bp.batch_size, bp.nb_variables, bp.state_dim
    plan = solve_mpc_batch(bp, return_multipliers=True)
    gU = torch.randn((Bn, n), dtype=torch.float64, device=bp.device)

    def jacobian(formulation):
        return lambda: plan_jacobian(bp, plan, formulation=formulation)[0]

    def backward():
        return autodiff._plan_vjp_stagewise(bp, plan, gU, None, {"x0", "goal"})

    jac = _median_us(jacobian("stagewise"), steps, warmup)
    jst = plan.jvp_status.clone()
    bwd = _median_us(backward, steps, warmup)
    active = (plan.multipliers > 0).sum(dim=1) if plan.multipliers is not None else torch.zeros(1)
    row = dict(case=name, batch=Bn, nx=nx, nu=bp.input_dim, N=bp.nb_timesteps, n=n, m=bp.nb_constraints,
               dtype=str(dt).replace("torch.", ""), tangents=nx, solved=float((plan.status == 0).float().mean()),
               jvp_ok=float((jst == 0).float().mean()), vjp_ok=float((plan.vjp_status == 0).float().mean()),
               active_rows_max=int(active.max()), active_rows_mean=round(float(active.float().mean()), 1),
               jacobian_stagewise_us=round(jac[0], 2),
               jacobian_stagewise_min_max_us=[round(jac[1], 2), round(jac[2], 2)],
               backward_stagewise_us=round(bwd[0], 2), backward_stagewise_min_max_us=[round(bwd[1], 2), round(bwd[2], 2)],
               jacobian_over_backward=round(jac[0] / bwd[0], 3), n_backwards_over_jacobian=round(n * bwd[0] / jac[0], 1))
    if n <= 128:
        JS = jacobian("stagewise")()
        cond = _median_us(jacobian("condensed"), steps, warmup)
        JC = jacobian("condensed")()
        ok = (jst == 0) & (plan.jvp_status == 0)
        row.update(jacobian_condensed_us=round(cond[0], 2), stagewise_over_condensed=round(jac[0] / cond[0], 3),
                   max_abs_diff_stagewise_vs_condensed=float((JS - JC)[ok].abs().max()) if bool(ok.any()) else float("nan"))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan_jvp_stagewise.py needs a GPU (no CPU timing is reported)")
    rows = []
    for name in args.cases.split(","):
        rows.append(run_case(name, args.steps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
