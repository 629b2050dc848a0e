#!/usr/bin/env python
"""Dev tool: what the fused closed-loop forward sensitivities cost against the loop composed in torch (profiles/loop_jvp.md,
section 2).

Triple-integrator family of tools/bench_loop_diff.py (nx = 3, nu = 1, N = 16: n = 16, m = 32), plant = model, 50 periods from
seeded initial states, B loops; T = nx (the x0 Jacobian, one identity shared by the batch) and T = 1 (one x0 tangent per
loop). One step = the loop and its tangents:
  composed  closed_loop_jvp(fused=False): SharedModel.solve, SharedModel.plan_jvp and the plant step of both per period
  fused     closed_loop_jvp(fused=True): one mpcqp_model_periods_batch launch, one replay launch, one
            mpcqp_model_periods_jvp_batch launch
and the fused step split into its three launches, timed one by one through the same entry points. Every figure is the median of
--steps steps after --warmup, device-event time and wall time (perf_counter around a synchronised step).
usage: bench_loop_jvp.py [--batches 256,1024,4096] [--periods 50] [--steps 20] [--warmup 3] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_loop_diff import make, timed  # noqa: E402


def main():
    import torch

    from qpmpc_amd import ModelClosedLoop, closed_loop_jvp, loop_diff

    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024,4096")
    ap.add_argument("--periods", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loop_jvp.py measures on the GPU only")
    P, rows = a.periods, []
    for B in [int(b) for b in a.batches.split(",")]:
        sm, x0, goal, dist = make(B)
        nx = x0.shape[1]
        # the fused step's launches, one by one
        loop = ModelClosedLoop(sm, x0, goal=goal, disturbance=dist)
        loop.step(P)
        X, U0 = loop.X, loop.U0
        lam, status, _, _ = loop_diff._replay(sm, loop, X, U0, P)

        def forward():
            lp = ModelClosedLoop(sm, x0, goal=goal, disturbance=dist)
            lp.step(P)

        for T in (nx, 1):
            d_x0 = (torch.eye(nx, dtype=torch.float64, device="cuda")[None] if T == nx
                    else torch.randn((B, 1, nx), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3)))
            tans = loop_diff._loop_tangents((d_x0, None, None, None, None, None), B, P, nx, 1, 16, x0.device)
            out = {}

            def step(fused):
                out[fused] = closed_loop_jvp(sm, x0, P, goal=goal, disturbance=dist, d_x0=d_x0, fused=fused)

            row = dict(B=B, periods=P, T=T)
            for name, fn in (("composed", lambda: step(False)), ("fused", lambda: step(True)), ("fused_forward", forward),
                             ("fused_replay", lambda: loop_diff._replay(sm, loop, X, U0, P)),
                             ("fused_tangent", lambda: loop_diff.loop_jvp(sm, loop, lam, status, X, U0, tans))):
                dev, wall = timed(fn, a.steps, a.warmup)
                row[name] = dict(device_us=dev, wall_us=wall)
                print(f"B={B:5d} T={T} {name:15s} device {dev:10.1f} us  wall {wall:10.1f} us", flush=True)
            torch.cuda.synchronize()
            info = out[True][4]
            row["replay_error"] = float(info.replay_error.item())
            row["failed_periods"] = int(info.failed.item())
            row["counted_periods"] = int(info.jvp_status.sum().item())
            row["max_diff_fused_vs_composed"] = max(
                float(((f - c).abs() / c.abs().clamp_min(1.0)).max()) for f, c in zip(out[True][2:4], out[False][2:4]))
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    print("| B | T | composed: device / wall (ms) | fused: device / wall (ms) | ratio device / wall | fused forward / replay / tangent "
          "kernel, device (us) | tangent kernel per period (us) | fused against composed |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        c, f = r["composed"], r["fused"]
        print(f"| {r['B']} | {r['T']} | {c['device_us'] / 1e3:.2f} / {c['wall_us'] / 1e3:.2f} | {f['device_us'] / 1e3:.3f} / "
              f"{f['wall_us'] / 1e3:.3f} | {c['device_us'] / f['device_us']:.1f}x / {c['wall_us'] / f['wall_us']:.1f}x | "
              f"{r['fused_forward']['device_us']:.0f} / {r['fused_replay']['device_us']:.0f} / {r['fused_tangent']['device_us']:.0f} | "
              f"{r['fused_tangent']['device_us'] / r['periods']:.1f} | {r['max_diff_fused_vs_composed']:.1e} |")


if __name__ == "__main__":
    main()
