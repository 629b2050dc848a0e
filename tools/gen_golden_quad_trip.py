#!/usr/bin/env python3
"""Fixture generator (needs a GPU; no reference code involved): tests/golden/quad_trip_parent.npz -- what the four-per-wavefront
kernel (csrc/mpcqp_quad.hip) computed for a few small launches, U, lam, status and iters, recorded from the build of the commit
BEFORE the steady loop's lane-mask arithmetic and its single trip counter. tests/test_gpu_quad_parent_bits.py holds the kernel to these
bits (what the four fixtures of this kind share is tools/quad_parent_bits.py);
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

import tools.quad_parent_bits as H

PATH = os.path.join(ROOT, "tests", "golden", "quad_trip_parent.npz")
LIMITS = (1, 2, 8)
LAUNCHES = {
    "a": H.Launch("a"),
    **{f"a_mi{k}": H.Launch("a", max_iter=k) for k in LIMITS},
    "c": H.Launch("c"),
    "d": H.Launch("d"),
    "a_slim": H.Launch("a", tile=H.WAVE_PAST_SIMDS, stored=10),
}
SETS = tuple(LAUNCHES)
SEED_A, SEED_C, SEED_D = 4, 2, 11
TIGHT_A = (3.0, 0.6, 0.15, 0.04, 0.04)


def _draw(rng, batch, N, tight):
    """random_ltv at (nx, nu, mk) = (3, 1, 2) with tight_ltv's dynamics"""
    from qpmpc_amd.workloads import random_ltv, tight_dynamics

    return tight_dynamics(random_ltv(rng, batch, 3, 1, N, 2, tight))


def _lean(w):
    w["D"] = None
    w["wx"] = w["targets"] = None
    return w


def set_a():
    rng = np.random.default_rng(SEED_A)
    w = _draw(rng, 10, 16, 1.0)
    tight = np.asarray(TIGHT_A)[np.arange(10) % len(TIGHT_A)]
    for b in range(10):  # bounds around the free response, as random_ltv makes them, at this problem's tightness
        x = w["x0"][b].copy()
        for k in range(16):
            w["e"][b, k] = w["C"][b, k] @ x + tight[b] * (0.05 + 0.5 * np.abs(rng.standard_normal(2)))
            x = w["A"][b, k] @ x
    return _lean(w)


def set_c():
    w = _draw(np.random.default_rng(SEED_C), 10, 9, 0.05)
    w["wx"] = w["targets"] = None
    return w


def set_d():
    w = _lean(_draw(np.random.default_rng(SEED_D), 8, 16, 0.02))
    w["B"][0::2] *= 1e-3
    w["wt"] = -50.0
    return w


def inputs():
    return {"a": set_a(), "c": set_c(), "d": set_d()}


def load():
    """{launch: (U, lam, status, iters)} of the stored fixture: outputs only, as {launch}__{output}"""
    return H.unpack(np.load(PATH), (), LAUNCHES, out_prefix="")[1]


def fixture():
    """(launches, the inputs, the recorded outputs)"""
    return LAUNCHES, inputs(), load()


def main():
    sets = inputs()
    results = H.stored(LAUNCHES, H.record(lambda name: H.run(LAUNCHES[name], sets), LAUNCHES))
    for name, (_, _, st, it) in results.items():
        print(f"{name:8s} statuses {st.tolist()} iters {it.tolist()}")
    np.savez_compressed(PATH, **H.pack({}, results, out_prefix=""))
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
