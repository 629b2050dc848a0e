#!/usr/bin/env python3
"""Fixture generator (needs a GPU; no reference code involved): tests/golden/quad_steady_parent.npz -- the operands of a few small
problem sets and what the four-per-wavefront kernel (csrc/mpcqp_quad.hip) computed for them, U, lam, status and iters, recorded from
the build of the commit BEFORE the kernel's steady loop. tests/test_gpu_quad_parent_bits.py holds the kernel to these bits; what the
four fixtures of this kind share is tools/quad_parent_bits.py.

Sets (LAUNCHES; every launch forced through MPCQP_OPT_FOUR_PER_WAVE):
  lean16       lean build, (nx, nu, N, mk) = (3, 1, 16, 2), 64 problems, max_iter = MAX_ITER_MAIN (so that the iteration limit ends
               some rows next to rows that solve, drop or are inconsistent)
  lean16_cut5  its first five problems (the second wavefront has one problem: idle rows repeat it)
  lean16_mi5   the 64 problems under max_iter = 5 (the limit exit in nearly every wavefront)
  lean16_slim  the 64 problems tiled to 4100: more wavefronts than SIMDs, the slim LDS carve. Every tile must give the same bits
               (a row's arithmetic does not depend on its wavefront): the 64 distinct results are stored
  lean9        lean build, N = 9 (m = 18: the lanes' second register row is partly populated), 32 problems
  gen12        general build, (4, 1, 12) with state and input rows and a stage cost, 32 problems
  model        shared-model mode, the humanoid model, 32 initial states
Families: random LTV problems (qpmpc_amd/workloads.py: mixed_family) with A and C taken from the first step -- bounds generated along that
time-invariant system (consistent; tightness 0.05 / 0.2 / 3.0) or along the per-step one (rows no longer consistent with e: the
inconsistent family of tests/test_gpu_quad.py) --, interleaved so that the four rows of a wavefront differ in kind.
The generator draws seeds until the recorded outputs of lean16 satisfy conditions() below; the test asserts them again."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import tools.quad_parent_bits as H

PATH = os.path.join(ROOT, "tests", "golden", "quad_steady_parent.npz")
MAX_ITER_MAIN = 20
SLIM_BATCH = 4100
OPERAND_SETS = ("lean16", "lean9", "gen12", "model")
LAUNCHES = {
    "lean16": H.Launch("lean16", max_iter=MAX_ITER_MAIN),
    "lean16_cut5": H.Launch("lean16", cut=5, max_iter=MAX_ITER_MAIN),
    "lean16_mi5": H.Launch("lean16", max_iter=5),
    "lean16_slim": H.Launch("lean16", tile=SLIM_BATCH, stored=64, max_iter=MAX_ITER_MAIN),
    "lean9": H.Launch("lean9"),
    "gen12": H.Launch("gen12"),
    "model": H.Launch("model", model=True),
}
SETS = tuple(LAUNCHES)


def conditions(U, lam, status, iters):
    """what the main set's recorded outputs must show (the names of the conditions that FAIL)"""
    npos = (lam > 0).sum(axis=1)
    st4, it4 = status.reshape(-1, 4), np.sort(iters.reshape(-1, 4), axis=1)
    checks = {
        "solved with zero iterations": bool(((status == 0) & (iters == 0)).any()),
        "solved after a drop": bool(((status == 0) & (iters > npos)).any()),
        "infeasible": bool((status == 2).any()),
        "iteration limit": bool((status == 1).any()),
        "four wavefronts with mixed statuses": int((st4.min(axis=1) != st4.max(axis=1)).sum()) >= 4,
        "four wavefronts with one row >= 4 iterations behind the others": int((it4[:, 3] - it4[:, 2] >= 4).sum()) >= 4,
    }
    return [k for k, ok in checks.items() if not ok]


def fixture():
    """(launches, operand dictionaries by set, recorded outputs by launch) of the stored fixture"""
    return (LAUNCHES,) + H.unpack(np.load(PATH), OPERAND_SETS, SETS)


def main():
    from qpmpc_amd import workloads as W

    for seed in range(400):
        rng = np.random.default_rng(20261019 + seed)
        sets = {"lean16": W.mixed_family(rng, 64, 3, 1, 16, 2, False)}
        res = H.run(LAUNCHES["lean16"], sets)
        failed = conditions(*res)
        print("seed", seed, "statuses", np.bincount(res[2], minlength=4), "fails:", failed, flush=True)
        if not failed:
            break
    else:
        raise SystemExit("no seed satisfied the conditions")
    sets["lean9"] = W.mixed_family(rng, 32, 3, 1, 9, 2, False)
    sets["gen12"] = W.mixed_family(rng, 32, 4, 1, 12, 2, True)
    sets["model"] = {"x0": 2.0 * W.humanoid_batch(32, seed=20261019 + seed)["x0"]}  # (twice the sweep's range: 0 .. 19 iterations)
    results = H.stored(LAUNCHES, H.record(lambda name: H.run(LAUNCHES[name], sets), SETS))
    H.report(results)
    assert (results["lean16_mi5"][2] == 1).any()
    np.savez_compressed(PATH, **H.pack(sets, results, seed=np.int64(seed)))
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
