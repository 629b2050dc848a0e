#!/usr/bin/env python3
"""Dev: the QP-given mode of csrc/mpcqp_duo.hip (mpcqp_solve_batch with MPCQP_OPT_ON_CHIP_32: dense QPs of up to 32 variables and 64
rows on chip, two problems per wavefront) against the same export without the flag -- the one-per-wavefront kernel up to sixteen
variables, the workgroup kernel beyond --, in one process, on the same seeded problems. Dense QPs are drawn like
tests/guarded_launch.py::_dense_qps (P = M M' / n + 0.1 I, G ~ N(0, 1), h > 0: x = 0 is feasible), on the device from a
seeded generator. MPC batches (random_ltv at tightness 0.3) are condensed by BatchMPCQP; the condense launch is timed apart
(mpcqp_condense_batch on kept buffers), and solve_mpc_batch's own route for the same problems (PreparedSolve, one launch) is timed
next to the two launches.
Printed per size and batch: equal statuses, max |dx| / max(1, |x|) of the flagged launch against the default one on the items both
solved, mean iterations, and us per launch of each: the minimum over two alternating rounds of series of back-to-back launches on
fixed buffers, and the spread (the difference of the two rounds' minima) a difference between launches has to exceed. Device events
around each series; ten launches of warm-up each.
usage: ab_onchip32_qp.py [batch ...]   (default 256 4096 16384)"""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
from qpmpc_amd import BatchMPCQP, PreparedSolve, _capi
from qpmpc_amd.batch import _stream_ptr
from qpmpc_amd.workloads import random_ltv, to_batch_problem

SIZES = ((16, 32), (17, 33), (24, 48), (32, 64))
MPC_SHAPES = ((3, 1, 24, 2), (6, 2, 12, 2))
FLAG = _capi.OPT_ON_CHIP_32

def dense_qps(n, m, batch, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float64)
    M = rn(batch, n, n)
    P = M @ M.transpose(1, 2) / n + 0.1 * torch.eye(n, device="cuda", dtype=torch.float64)
    return P.contiguous(), rn(batch, n), rn(batch, m, n), rn(batch, m).abs() * 0.2 + 0.05

class Solve:
    """mpcqp_solve_batch on fixed buffers: launch() is one C call"""
    def __init__(self, P, q, G, h, flags):
        self.lib = _capi.load()
        B, n = q.shape
        m = G.shape[1]
        mk = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device="cuda")
        self.x, self.lam, self.status, self.iters = mk(B, n), mk(B, m), mk(B, dt=torch.int32), mk(B, dt=torch.int32)
        nbytes = C.c_size_t(0)
        if not flags:
            _capi.check(self.lib.mpcqp_solve_workspace_bytes(n, m, _capi.F64, B, C.byref(nbytes)), "mpcqp_solve_workspace_bytes")
        self.ws = torch.empty((max(nbytes.value, 1),), dtype=torch.uint8, device="cuda")
        self.opts = _capi.SolveOpts()
        self.opts.flags = int(flags)
        self.keep = (P, q, G, h)
        self.args = (n, m, _capi.F64, P.data_ptr(), q.data_ptr(), G.data_ptr(), h.data_ptr(), B, C.byref(self.opts), self.x.data_ptr(),
                     self.lam.data_ptr(), self.status.data_ptr(), self.iters.data_ptr(), self.ws.data_ptr() if nbytes.value else None, nbytes.value)
    def launch(self):
        _capi.check(self.lib.mpcqp_solve_batch(*self.args, _stream_ptr()), "mpcqp_solve_batch")

class Condense:
    """mpcqp_condense_batch into the buffers of a BatchMPCQP"""
    def __init__(self, bp, qp):
        self.lib, self.bp, self.qp = _capi.load(), bp, qp
        self.dims, self.cp = bp.dims(), bp.c_problem()
        ws = qp._ws
        self.args = (C.byref(self.dims), C.byref(self.cp), bp.batch_size, qp.P.data_ptr(), qp.q.data_ptr(), qp.G.data_ptr(), qp.h.data_ptr(),
                     None, None, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel())
    def launch(self):
        _capi.check(self.lib.mpcqp_condense_batch(*self.args, _stream_ptr()), "mpcqp_condense_batch")

def series(run, n):
    for _ in range(10): run.launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): run.launch()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

def timed(runs, batch, rounds=2):
    n = 200 if batch <= 4096 else 60
    t = {k: [] for k in runs}
    for _ in range(rounds):  # the launches alternate
        for k, r in runs.items(): t[k].append(series(r, n))
    return {k: f"{min(v):.1f} ± {abs(v[0] - v[1]):.1f}" for k, v in t.items()}, {k: min(v) for k, v in t.items()}

def agreement(a, b):
    """(equal statuses, solved by both, max relative |dx|) of two launches that have run"""
    torch.cuda.synchronize()
    sa, sb = a.status.cpu(), b.status.cpu()
    ok = (sa == 0) & (sb == 0)
    xa, xb = a.x.cpu()[ok], b.x.cpu()[ok]
    err = ((xa - xb).abs().max(dim=1).values / xb.abs().max(dim=1).values.clamp(min=1.0)).max().item() if ok.any() else float("nan")
    return bool((sa == sb).all()), int(ok.sum()), err

def dense(size, batch):
    n, m = size
    P, q, G, h = dense_qps(n, m, batch, 1000 * n + m)
    runs = dict(flag=Solve(P, q, G, h, FLAG), default=Solve(P, q, G, h, 0))
    for r in runs.values(): r.launch()
    same, solved, err = agreement(runs["flag"], runs["default"])
    cell, best = timed(runs, batch)
    print(f"| ({n}, {m}) | {batch} | {'yes' if same else 'NO'} ({solved} solved) | {err:.1e} | {runs['flag'].iters.float().mean().item():.2f} |"
          f" {cell['flag']} | {cell['default']} | {best['default'] / best['flag']:.2f} |", flush=True)

def mpc(shape, batch):
    nx, nu, N, mk = shape
    bp = to_batch_problem(random_ltv(np.random.default_rng(7), batch, nx, nu, N, mk, 0.3))
    qp = BatchMPCQP(bp, keep_propagators=False)
    runs = dict(condense=Condense(bp, qp), flag=Solve(qp.P, qp.q, qp.G, qp.h, FLAG), default=Solve(qp.P, qp.q, qp.G, qp.h, 0), mpc=PreparedSolve(bp, keep_warm_factor=False))
    for r in runs.values(): r.launch()
    same, solved, err = agreement(runs["flag"], runs["default"])
    torch.cuda.synchronize()
    um = runs["mpc"].U.reshape(batch, -1).cpu()
    okm = (runs["mpc"].status.cpu() == 0) & (runs["flag"].status.cpu() == 0)
    xf = runs["flag"].x.cpu()
    errm = ((xf[okm] - um[okm]).abs().max(dim=1).values / um[okm].abs().max(dim=1).values.clamp(min=1.0)).max().item() if okm.any() else float("nan")
    cell, best = timed(runs, batch)
    print(f"| {shape} | {batch} | {'yes' if same else 'NO'} ({solved} solved) | {err:.1e} / {errm:.1e} | {runs['flag'].iters.float().mean().item():.2f} |"
          f" {cell['condense']} | {cell['flag']} | {cell['default']} | {cell['mpc']} | {best['mpc'] / (best['condense'] + best['flag']):.2f} |", flush=True)

if __name__ == "__main__":
    batches = [int(x) for x in sys.argv[1:]] or [256, 4096, 16384]
    print("| size (n, m) | batch | equal status | max dx, flag vs default | mean iters | flag, us | default route, us | default / flag |")
    print("|---|---|---|---|---|---|---|---|")
    for bsz in batches:
        for size in SIZES:
            dense(size, bsz)
    print()
    print("| shape (nx, nu, N, mk) | batch | equal status | max dx, flag vs default / vs solve_mpc_batch | mean iters | condense, us | solve, flag, us | solve, default route, us | solve_mpc_batch (one launch), us | one launch / (condense + flag) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for bsz in batches:
        for shape in MPC_SHAPES:
            mpc(shape, bsz)
