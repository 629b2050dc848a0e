#!/usr/bin/env python3
"""The feedback Jacobian dU/dx0 of a batch of solved plans, three ways, timed with device events (median of --steps
after --warmup):

    python tools/bench_plan_jvp.py [--steps 30] [--warmup 5] [--out FILE]

Cases: BASELINE config 2 (4096 triple-integrator problems, n = 16) and 1024 wheeled-inverted-pendulum problems with N = 50.
Per case, on one plan solved with multipliers:
  - jacobian_us: plan_jacobian(wrt="initial_state"): one mpcqp_plan_jvp_batch call with nx shared tangents;
  - n_vjp_us: the same Jacobian assembled from n calls of mpcqp_plan_vjp_batch, one per row (what was possible before);
  - backward_us: one backward of solve_mpc_batch_diff (condensing + the adjoint kernel + the reductions).
The two Jacobians are compared (max_abs_diff, over problems both solved). A kernel split comes from a separate
``rocprofv3 --kernel-trace --stats`` run of this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from qpmpc_amd import autodiff, plan_jacobian, solve_mpc_batch, solve_mpc_batch_diff, workloads as W  # noqa: E402


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
    Bn, n, nx = bp.batch_size, bp.nb_variables, bp.state_dim
    plan = solve_mpc_batch(bp, return_multipliers=True)
    rows = []
    for i in range(n):
        g = torch.zeros((Bn, n), dtype=torch.float64, device=bp.device)
        g[:, i] = 1.0
        rows.append(g)

    def jacobian():
        return plan_jacobian(bp, plan)[0]

    def n_vjp():
        return torch.stack([autodiff._plan_vjp(bp, plan, g, None, set())[0] for g in rows], dim=1)  # [B, n, nx]

    jac = _median_us(jacobian, steps, warmup)
    JU = jacobian().reshape(Bn, n, nx)
    jst = plan.jvp_status.clone()
    nv = _median_us(n_vjp, steps, warmup)
    JV = n_vjp()
    ok = (jst == 0) & (plan.vjp_status == 0)
    diff = float((JU - JV)[ok].abs().max()) if bool(ok.any()) else float("nan")

    x0 = torch.as_tensor(w["x0"], device=bp.device).clone().requires_grad_()
    gU = torch.randn((Bn, bp.nb_timesteps, bp.input_dim), dtype=torch.float64, device=bp.device)
    held = {}
    for _ in range(warmup):
        held["U"] = solve_mpc_batch_diff(bp, initial_state=x0)[0]
        held["U"].backward(gU)
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        x0.grad = None
        held["U"] = solve_mpc_batch_diff(bp, initial_state=x0)[0]
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        held["U"].backward(gU)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    bwd = times[len(times) // 2]
    return dict(case=name, batch=Bn, n=n, nx=nx, m=bp.nb_constraints, jacobian_us=round(jac[0], 2),
                jacobian_min_max_us=[round(jac[1], 2), round(jac[2], 2)], n_vjp_us=round(nv[0], 2),
                n_vjp_calls=n, backward_us=round(bwd, 2), n_vjp_over_jacobian=round(nv[0] / jac[0], 2),
                jacobian_over_backward=round(jac[0] / bwd, 2), solved_frac=float(ok.float().mean()),
                max_abs_diff_jacobian_vs_n_vjp=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan_jvp.py needs a GPU (no CPU timing is reported)")
    rows = [run_case("config2_triple_integrator", W.triple_integrator_batch(4096), args.steps, args.warmup),
            run_case("wip_N50", W.wip_batch(1024, N=50), args.steps, args.warmup)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
