#!/usr/bin/env python3
"""Fixture generator (needs a GPU; no reference code involved): tests/golden/quad_trip_parent.npz -- what the four-per-wavefront
kernel (csrc/mpcqp_quad.hip) computed for a few small launches, U, lam, status and iters, recorded from the build of the commit
BEFORE the steady loop's lane-mask arithmetic and its single trip counter. tests/test_gpu_quad_trip.py holds the kernel to these bits;
tests/test_quad_trip_cpu.py holds the inputs to the conditions below with the oracle and tools/quad_trip_model.py alone.

The inputs are drawn from fixed seeds (inputs(): nothing is stored but the outputs); every launch is forced through
MPCQP_OPT_FOUR_PER_WAVE and made twice, with equal bits.
  a        10 lean problems (nx, nu, N, mk) = (3, 1, 16, 2), random_ltv with tight_ltv's dynamics, tightness 3.0 .. 0.04 by problem: a
           ragged last wavefront (two problems, two idle rows), rows of one wavefront that finish on different trips
  a_mi1, a_mi2, a_mi8   the same under max_iter = 1, 2, 8: the limit is met inside the steady loop by some rows of a wavefront while
           others have finished
  c        10 problems at N = 9 (n = 9) with state AND input rows (the general build: with state rows alone the last input meets no
           row, so that at most n - 1 rows are ever active), tightness 0.05: some rows reach nq = n
  d        8 lean problems (3, 1, 16, 2), tightness 0.02, under a terminal weight of -50: P = wu I - 50 Psi_N' Psi_N is indefinite for
           the odd problems -- not positive definite, the row is done on entry -- and positive definite for the even ones, whose B is
           a thousand times smaller; they solve in 8 .. 16 trips next to the rows that never start. (The C API refuses wu = 0,
           mpcqp_capi.hip: the indefinite Hessian comes from the terminal weight, as in tests/verdict_cases.py.)
  a_slim   set a tiled to one wavefront more than the device has SIMDs: the slim LDS carve (every tile must repeat a's bits; the
           ten distinct results are stored)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PATH = os.path.join(ROOT, "tests", "golden", "quad_trip_parent.npz")
OPERANDS = ("A", "B", "C", "D", "e", "x0", "goal", "targets")
OUTPUTS = ("U", "lam", "status", "iters")
LIMITS = (1, 2, 8)
LAUNCHES = ("a",) + tuple(f"a_mi{k}" for k in LIMITS) + ("c", "d", "a_slim")
SEED_A, SEED_C, SEED_D = 4, 2, 11
TIGHT_A = (3.0, 0.6, 0.15, 0.04, 0.04)


def _tight_dynamics(w):
    w["A"] = np.eye(w["A"].shape[-1]) + 0.1 * (w["A"] - np.eye(w["A"].shape[-1]))  # (tight_ltv's)
    return w


def _lean(w):
    w["D"] = None
    w["wx"] = w["targets"] = None
    return w


def set_a():
    from qpmpc_amd.workloads import random_ltv

    rng = np.random.default_rng(SEED_A)
    w = _tight_dynamics(random_ltv(rng, 10, 3, 1, 16, 2, 1.0))
    tight = np.asarray(TIGHT_A)[np.arange(10) % len(TIGHT_A)]
    for b in range(10):  # bounds around the free response, as random_ltv makes them, at this problem's tightness
        x = w["x0"][b].copy()
        for k in range(16):
            w["e"][b, k] = w["C"][b, k] @ x + tight[b] * (0.05 + 0.5 * np.abs(rng.standard_normal(2)))
            x = w["A"][b, k] @ x
    return _lean(w)


def set_c():
    from qpmpc_amd.workloads import random_ltv

    w = _tight_dynamics(random_ltv(np.random.default_rng(SEED_C), 10, 3, 1, 9, 2, 0.05))
    w["wx"] = w["targets"] = None
    return w


def set_d():
    from qpmpc_amd.workloads import random_ltv

    w = _lean(_tight_dynamics(random_ltv(np.random.default_rng(SEED_D), 8, 3, 1, 16, 2, 0.02)))
    w["B"][0::2] *= 1e-3
    w["wt"] = -50.0
    return w


def inputs():
    return {"a": set_a(), "c": set_c(), "d": set_d()}


def tiled(w, count):
    out = dict(w)
    for k in OPERANDS:
        if isinstance(w.get(k), np.ndarray):
            v = w[k]
            out[k] = np.ascontiguousarray(np.concatenate([v] * (count // len(v) + 1))[:count])
    return out


def slim_batch():
    """four problems per wavefront, one wavefront more than the device has SIMDs (four per compute unit)"""
    import torch

    return 4 * (4 * torch.cuda.get_device_properties(0).multi_processor_count + 1)


def solve(w, max_iter=None):
    """(U, lam, status, iters) of the forced four-per-wavefront launch, as numpy arrays"""
    import torch
    from qpmpc_amd import _capi, solve_mpc_batch
    from qpmpc_amd import workloads as W

    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True, max_iter=max_iter, flags=_capi.OPT_FOUR_PER_WAVE)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (plan.U, plan.multipliers, plan.status, plan.iters))


def run_launch(name, sets):
    """what the kernel computes NOW for launch `name` (a_slim: all slim_batch() problems)"""
    if name == "a_slim":
        return solve(tiled(sets["a"], slim_batch()))
    if name.startswith("a_mi"):
        return solve(sets["a"], int(name[4:]))
    return solve(sets[name])


def load():
    """{launch: (U, lam, status, iters)} of the stored fixture"""
    z = np.load(PATH)
    return {name: tuple(z[f"{name}__{k}"] for k in OUTPUTS) for name in LAUNCHES}


def main():
    sets = inputs()
    results = {name: run_launch(name, sets) for name in LAUNCHES}
    again = {name: run_launch(name, sets) for name in LAUNCHES}  # (the kernel is deterministic: the bits of a second launch)
    for name in LAUNCHES:
        for a, b in zip(results[name], again[name]):
            assert a.tobytes() == b.tobytes(), name
    slim, count = results["a_slim"], slim_batch()
    for v in slim:  # every tile of the slim launch: the same bits
        assert len(v) == count and np.concatenate([v[:10]] * (count // 10 + 1))[:count].tobytes() == v.tobytes(), "slim tiles differ"
    results["a_slim"] = tuple(v[:10] for v in slim)
    for name in LAUNCHES:
        st, it = results[name][2], results[name][3]
        print(f"{name:8s} statuses {st.tolist()} iters {it.tolist()}")
    np.savez_compressed(PATH, **{f"{name}__{k}": v for name, res in results.items() for k, v in zip(OUTPUTS, res)})
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
