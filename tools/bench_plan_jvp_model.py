#!/usr/bin/env python3
"""Model and weight tangents of plans, plan_jvp with dA, dB and dw, timed with device events (median of --steps after
--warmup) beside the state-only tangent solve and one model backward on the same plan:

    python tools/bench_plan_jvp_model.py [--steps 20] [--warmup 5] [--cases a,b] [--out FILE]

Cases (sizes and T as DESIGN.md section 9's tables): BASELINE config 2 x 4096 and the wheeled inverted pendulum with
N = 50 x 1024, condensed; the config-5 shape in float32 storage x 8192 and the pendulum with N = 200 x 1024 at T = 0.005 s,
stage-wise. T = nx tangents per problem, shared by the batch. Per case, on one plan solved with multipliers in one process,
in microseconds per batch (the host side of each call included: workspace, casts and, stage-wise, the max_active sync):
  - a_state_us: plan_jvp with T tangents of the initial state only (mpcqp_plan_jvp_batch / _stagewise_batch);
  - b_model_us: the same T with tangents of A, B and the three weights added (mpcqp_plan_jvp_model_batch /
    _model_stagewise_batch);
  - c_backward_us: one model backward (mpcqp_plan_vjp_model_batch / mpcqp_plan_vjp_stagewise_batch with g_A .. g_w).
A kernel split comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_autodiff_stagewise import CASES as _ALL  # noqa: E402
from bench_plan_jvp_stagewise import _median_us  # noqa: E402
from qpmpc_amd import autodiff, plan_jvp, solve_mpc_batch, workloads as W  # noqa: E402

CASES = {"config2_triple_integrator": "condensed", "wip_N50": "condensed", "config5_shape_f32": "stagewise",
         "wip_N200": "stagewise"}


def run_case(name, steps, warmup):
    formulation = CASES[name]
    w, dt = _ALL[name]()
    bp = W.to_batch_problem(w, dtype=dt)
    Bn, n, nx, nu, N = bp.batch_size, bp.nb_variables, bp.state_dim, bp.input_dim, bp.nb_timesteps
    plan = solve_mpc_batch(bp, return_multipliers=True, formulation=formulation)
    T = nx
    gen = torch.Generator(device="cpu").manual_seed(1)
    f64 = dict(dtype=torch.float64, device=bp.device)
    dx0 = torch.eye(nx, **f64)[None]
    dA = torch.randn((1, T, N, nx, nx), generator=gen, dtype=torch.float64).to(bp.device)
    dB = torch.randn((1, T, N, nx, nu), generator=gen, dtype=torch.float64).to(bp.device)
    dw = [torch.randn((1, T), generator=gen, dtype=torch.float64).to(bp.device) for _ in range(3)]
    gU = torch.randn((Bn, n), generator=gen, dtype=torch.float64).to(bp.device)

    def state():
        return plan_jvp(bp, plan, initial_state=dx0, formulation=formulation)[0]

    def model():
        return plan_jvp(bp, plan, initial_state=dx0, formulation=formulation, transition_state_matrix=dA,
                        transition_input_matrix=dB, terminal_cost_weight=dw[0], stage_state_cost_weight=dw[1],
                        stage_input_cost_weight=dw[2])[0]

    def backward():
        want = {"x0", "A", "B", "wt", "wx", "wu"}
        return autodiff._vjp(bp, plan, gU, None, want, "model" if formulation == "condensed" else "stagewise")

    a = _median_us(state, steps, warmup)
    b = _median_us(model, steps, warmup)
    jst = plan.jvp_status.clone()
    c = _median_us(backward, steps, warmup)
    active = (plan.multipliers > 0).sum(dim=1) if plan.multipliers is not None else torch.zeros(1)
    return dict(case=name, formulation=formulation, batch=Bn, nx=nx, nu=nu, N=N, n=n, m=bp.nb_constraints,
                dtype=str(dt).replace("torch.", ""), tangents=T, solved=float((plan.status == 0).float().mean()),
                jvp_ok=float((jst == 0).float().mean()), vjp_ok=float((plan.vjp_status == 0).float().mean()),
                active_rows_max=int(active.max()), active_rows_mean=round(float(active.float().mean()), 1),
                a_state_us=round(a[0], 2), a_state_min_max_us=[round(a[1], 2), round(a[2], 2)],
                b_model_us=round(b[0], 2), b_model_min_max_us=[round(b[1], 2), round(b[2], 2)],
                c_backward_us=round(c[0], 2), c_backward_min_max_us=[round(c[1], 2), round(c[2], 2)],
                b_over_a=round(b[0] / a[0], 3), b_over_c=round(b[0] / c[0], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan_jvp_model.py needs a GPU (no CPU timing is reported)")
    rows = []
    for name in args.cases.split(","):
        rows.append(run_case(name, args.steps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
