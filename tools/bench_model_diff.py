#!/usr/bin/env python3
"""Derivatives of shared-model plans beside the condensed exports, timed with device events (median of --steps after
--warmup), on the same batch and the same plan.

    python tools/bench_model_diff.py [--steps 100] [--warmup 10] [--out FILE] [--only NAME[,NAME]]

Cases: BASELINE config 2's shape with shared operands (4096 problems), config 4's humanoid sweep at 8192 and 65,536
states, and the wheeled inverted pendulum with N = 50 (1024 problems, time-invariant). Per case, in microseconds per batch:
the model forward with multipliers (mpcqp_solve_model_batch), mpcqp_model_vjp_batch, mpcqp_model_jvp_batch with the nx
identity tangents, and the exports they stand beside: mpcqp_plan_vjp_batch and mpcqp_plan_jvp_batch (workspaces
allocated once, outside the timed window, their bytes reported). A kernel split comes from a separate
``rocprofv3 --kernel-trace --stats`` run of this script.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from qpmpc_amd import SharedModel, _capi, workloads as W  # noqa: E402
from qpmpc_amd.autodiff import _workspace_for  # noqa: E402
from qpmpc_amd.batch import BatchMPCProblem, _stream_ptr  # noqa: E402


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
    return times[len(times) // 2]


def run_case(name, w, steps, warmup):
    lib = _capi.load()
    w = dict(w)
    w.pop("pendulum", None)
    bp = W.to_batch_problem(w)
    sm = SharedModel(bp)
    run = sm.prepare(bp, return_multipliers=True)
    run.launch()
    plan = run.plan
    torch.cuda.synchronize()
    Bn, N, nx, nu, mk = bp.batch_size, bp.nb_timesteps, bp.state_dim, bp.input_dim, bp.ineq_dim
    n, m, R = N * nu, N * mk, (N + 1) * nx
    f64 = dict(dtype=torch.float64, device=bp.device)
    gU, gX = torch.randn((Bn, n), **f64), torch.randn((Bn, R), **f64)
    g = [torch.empty((Bn, k), **f64) for k in (nx, nx, N * nx, m)]
    st = torch.empty((Bn,), dtype=torch.int32, device=bp.device)
    eye = torch.eye(nx, **f64).contiguous()
    tan = _capi.Tangents(eye.data_ptr(), None, None, None, 0, 0, 0, 0)
    dU, dX = torch.empty((Bn, nx, n), **f64), torch.empty((Bn, nx, R), **f64)
    A, B = BatchMPCProblem._operand(bp.A), BatchMPCProblem._operand(bp.B)
    dims, cp = sm.dims, bp.c_problem()
    lam, status = plan.multipliers, plan.status
    ws_v = _workspace_for(lib.mpcqp_plan_vjp_workspace_bytes, dims, Bn, bp.device)
    ws_j = _workspace_for(lib.mpcqp_plan_jvp_workspace_bytes, dims, Bn, bp.device, nx)
    sp = _stream_ptr()

    def ok(rc):
        if rc != 0:
            _capi.check(rc, name)

    calls = dict(
        model_forward=run.launch,
        model_vjp=lambda: ok(lib.mpcqp_model_vjp_batch(
            C.byref(dims), sm.model.data_ptr(), Bn, lam.data_ptr(), status.data_ptr(), gU.data_ptr(), gX.data_ptr(),
            C.byref(A), C.byref(B), *[t.data_ptr() for t in g], st.data_ptr(), sp)),
        plan_vjp=lambda: ok(lib.mpcqp_plan_vjp_batch(
            C.byref(dims), C.byref(cp), Bn, lam.data_ptr(), status.data_ptr(), gU.data_ptr(), gX.data_ptr(),
            *[t.data_ptr() for t in g], st.data_ptr(), ws_v.data_ptr(), ws_v.numel(), sp)),
        model_jvp=lambda: ok(lib.mpcqp_model_jvp_batch(
            C.byref(dims), sm.model.data_ptr(), Bn, nx, lam.data_ptr(), status.data_ptr(), C.byref(tan), C.byref(A),
            C.byref(B), dU.data_ptr(), dX.data_ptr(), st.data_ptr(), sp)),
        plan_jvp=lambda: ok(lib.mpcqp_plan_jvp_batch(
            C.byref(dims), C.byref(cp), Bn, nx, lam.data_ptr(), status.data_ptr(), C.byref(tan), dU.data_ptr(),
            dX.data_ptr(), st.data_ptr(), ws_j.data_ptr(), ws_j.numel(), sp)),
    )
    act = ((lam > 0) & (status == 0)[:, None]).sum(dim=1).double() if m else torch.zeros((Bn,), **f64)
    out = dict(case=name, batch=Bn, n=n, m=m, solved=float((status == 0).double().mean()),
               active_rows_mean=round(float(act.mean()), 2), active_rows_max=int(act.max()),
               active_rows_none=round(float((act == 0).double().mean()), 3),
               plan_vjp_workspace_bytes=ws_v.numel(), plan_jvp_workspace_bytes=ws_j.numel(), model_workspace_bytes=0)
    for key, fn in calls.items():
        out[key + "_us"] = round(_median_us(fn, steps, warmup), 2)
    out["vjp_speedup"] = round(out["plan_vjp_us"] / out["model_vjp_us"], 2)
    out["jvp_speedup"] = round(out["plan_jvp_us"] / out["model_jvp_us"], 2)
    return out


CASES = dict(
    config2_shared_4096=lambda: W.triple_integrator_batch(4096, heterogeneous=False),
    humanoid_8192=lambda: W.humanoid_batch(8192),
    humanoid_65536=lambda: W.humanoid_batch(65536),
    wip_n50_lti_1024=lambda: W.wip_batch(1024, N=50, ltv=False),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    only = None if args.only is None else args.only.split(",")
    rows = [run_case(k, make(), args.steps, args.warmup) for k, make in CASES.items() if only is None or k in only]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(steps=args.steps, warmup=args.warmup, cases=rows), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
