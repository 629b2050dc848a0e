#!/usr/bin/env python3
"""Forward and backward of solve_mpc_batch_diff, timed separately with device events (median of --steps after --warmup).

    python tools/bench_autodiff.py [--steps 50] [--warmup 10] [--out FILE]

Cases: BASELINE config 2 (4096 triple-integrator problems, n = 16) and 1024 wheeled-inverted-pendulum problems with N = 50.
Per case: the fused forward alone (solve_mpc_batch, no multipliers), the differentiable forward (multipliers kept, graph
recorded) and the backward (mpcqp_condense_batch + the adjoint kernel + the reductions), in microseconds per batch.
A kernel split of the backward comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from qpmpc_amd import solve_mpc_batch, solve_mpc_batch_diff, workloads as W  # noqa: E402


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


def run_case(name, w, steps, warmup):
    bp = W.to_batch_problem(w)
    x0 = torch.as_tensor(w["x0"], device=bp.device).clone().requires_grad_()
    goal = torch.as_tensor(w["goal"], device=bp.device).clone().requires_grad_()
    gU = torch.randn((bp.batch_size, bp.nb_timesteps, bp.input_dim), dtype=torch.float64, device=bp.device)
    fused = _median_us(lambda: solve_mpc_batch(bp), steps, warmup)
    fwd = _median_us(lambda: solve_mpc_batch_diff(bp, initial_state=x0, goal_state=goal), steps, warmup)
    held = {}

    def forward_only():
        held["U"] = solve_mpc_batch_diff(bp, initial_state=x0, goal_state=goal)[0]

    def backward():
        x0.grad = goal.grad = None
        held["U"].backward(gU)

    for _ in range(warmup):
        forward_only()
        backward()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        forward_only()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        backward()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    bwd = (times[len(times) // 2], times[0], times[-1])
    n, m, nx, N = bp.nb_variables, bp.nb_constraints, bp.state_dim, bp.nb_timesteps
    # condensed operands the backward writes to HBM per problem: P, q, G, h, Phi, Psi (float64)
    condensed_bytes = 8 * (n * n + n + m * n + m + (N + 1) * nx * nx + (N + 1) * nx * n)
    return dict(case=name, batch=bp.batch_size, n=n, m=m, fused_forward_us=round(fused[0], 2),
                diff_forward_us=round(fwd[0], 2), backward_us=round(bwd[0], 2),
                backward_over_fused=round(bwd[0] / fused[0], 2), backward_min_max_us=[round(bwd[1], 2), round(bwd[2], 2)],
                condensed_bytes_per_problem=condensed_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autodiff.py needs a GPU (no CPU timing is reported)")
    rows = [run_case("config2_triple_integrator", W.triple_integrator_batch(4096), args.steps, args.warmup),
            run_case("wip_N50", W.wip_batch(1024, N=50), args.steps, args.warmup)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
