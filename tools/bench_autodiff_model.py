#!/usr/bin/env python3
"""Backward of solve_mpc_batch_diff with and without model gradients, timed with device events (median of --steps after
--warmup).

    python tools/bench_autodiff_model.py [--steps 50] [--warmup 10] [--out FILE]

Cases as tools/bench_autodiff.py: BASELINE config 2 (4096 triple-integrator problems, n = 16) and 1024 wheeled-inverted-
pendulum problems with N = 50. Per case, on the same forward plan and the same dL/dU: the backward when x0 and the goal
require grad (mpcqp_plan_vjp_batch) and when A, B, C or D (those present) and the three weights require grad as well
(mpcqp_plan_vjp_model_batch), in microseconds per batch. A kernel split comes from a separate
``rocprofv3 --kernel-trace --stats`` run of this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from qpmpc_amd import solve_mpc_batch_diff, workloads as W  # noqa: E402


def _leaf(a, bp):
    return torch.as_tensor(a, dtype=torch.float64, device=bp.device).clone().requires_grad_()


def _backward_us(bp, kw, leaves, gU, steps, warmup):
    held = {}

    def forward():
        held["U"] = solve_mpc_batch_diff(bp, **kw)[0]

    def backward():
        for t in leaves:
            t.grad = None
        held["U"].backward(gU)

    for _ in range(warmup):
        forward()
        backward()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        forward()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        backward()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def run_case(name, w, steps, warmup):
    bp = W.to_batch_problem(w)
    x0, goal = _leaf(w["x0"], bp), _leaf(w["goal"], bp)
    gU = torch.randn((bp.batch_size, bp.nb_timesteps, bp.input_dim), dtype=torch.float64, device=bp.device)
    plain = _backward_us(bp, dict(initial_state=x0, goal_state=goal), [x0, goal], gU, steps, warmup)
    model_kw = dict(initial_state=x0, goal_state=goal)
    leaves = [x0, goal]
    for key, arg in (("A", "transition_state_matrix"), ("B", "transition_input_matrix"), ("C", "ineq_state_matrix"),
                     ("D", "ineq_input_matrix"), ("wt", "terminal_cost_weight"), ("wx", "stage_state_cost_weight"),
                     ("wu", "stage_input_cost_weight")):
        if w[key] is not None:
            model_kw[arg] = _leaf(w[key], bp)
            leaves.append(model_kw[arg])
    model = _backward_us(bp, model_kw, leaves, gU, steps, warmup)
    return dict(case=name, batch=bp.batch_size, n=bp.nb_variables, m=bp.nb_constraints,
                backward_us=round(plain[0], 2), backward_model_us=round(model[0], 2),
                model_over_plain=round(model[0] / plain[0], 3), backward_min_max_us=[round(plain[1], 2), round(plain[2], 2)],
                backward_model_min_max_us=[round(model[1], 2), round(model[2], 2)],
                model_operands=[k for k in model_kw if k not in ("initial_state", "goal_state")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autodiff_model.py needs a GPU (no CPU timing is reported)")
    rows = [run_case("config2_triple_integrator", W.triple_integrator_batch(4096), args.steps, args.warmup),
            run_case("wip_N50", W.wip_batch(1024, N=50), args.steps, args.warmup)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
