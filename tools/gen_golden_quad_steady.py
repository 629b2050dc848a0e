#!/usr/bin/env python3
"""Fixture generator (needs a GPU; no reference code involved): tests/golden/quad_steady_parent.npz -- the operands of a few small
problem sets and what the four-per-wavefront kernel (csrc/mpcqp_quad.hip) computed for them, U, lam, status and iters, recorded from
the build of the commit BEFORE the kernel's steady loop. tests/test_gpu_quad_steady.py holds the kernel to these bits.

Sets (every launch forced through MPCQP_OPT_FOUR_PER_WAVE):
  lean16       lean build, (nx, nu, N, mk) = (3, 1, 16, 2), 64 problems, max_iter = MAX_ITER_MAIN (so that the iteration limit ends
               some rows next to rows that solve, drop or are inconsistent)
  lean16_cut5  its first five problems (the second wavefront has one problem: idle rows repeat it)
  lean16_mi5   the 64 problems under max_iter = 5 (the limit exit in nearly every wavefront)
  lean16_slim  the 64 problems tiled to 4100: more wavefronts than SIMDs, the slim LDS carve. Every tile must give the same bits
               (a row's arithmetic does not depend on its wavefront): the 64 distinct results are stored
  lean9        lean build, N = 9 (m = 18: the lanes' second register row is partly populated), 32 problems
  gen12        general build, (4, 1, 12) with state and input rows and a stage cost, 32 problems
  model        shared-model mode, the humanoid model, 32 initial states
Families: random LTV problems (qpmpc_amd/workloads.py: random_ltv) with A and C taken from the first step -- bounds generated along that
time-invariant system (consistent; tightness 0.05 / 0.2 / 3.0) or along the per-step one (rows no longer consistent with e: the
inconsistent family of tests/test_gpu_quad.py) --, interleaved so that the four rows of a wavefront differ in kind.
The generator draws seeds until the recorded outputs of lean16 satisfy conditions() below; the test asserts them again."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PATH = os.path.join(ROOT, "tests", "golden", "quad_steady_parent.npz")
MAX_ITER_MAIN = 20
SLIM_BATCH = 4100
OPERANDS = ("A", "B", "C", "D", "e", "x0", "goal", "targets")
OUTPUTS = ("U", "lam", "status", "iters")
SETS = ("lean16", "lean16_cut5", "lean16_mi5", "lean16_slim", "lean9", "gen12", "model")


def mixed_family(rng, batch, nx, nu, N, mk, general):
    """`batch` problems, row i of kind i % 4: tight (0.05), loose (3.0), inconsistent and tight (0.05), inconsistent (0.2)"""
    from qpmpc_amd.workloads import random_ltv

    w = random_ltv(rng, batch, nx, nu, N, mk, 1.0)
    tight = np.array([0.05, 3.0, 0.05, 0.2])[np.arange(batch) % 4]
    broken = np.arange(batch) % 4 >= 2
    shift = rng.integers(0, 4, batch // 4)  # (the kinds sit in another row of every wavefront)
    for g in range(batch // 4):
        sl = slice(4 * g, 4 * g + 4)
        tight[sl], broken[sl] = np.roll(tight[sl], shift[g]), np.roll(broken[sl], shift[g])
    A, Cm, e = w["A"], w["C"], w["e"]
    for b in range(batch):
        x = w["x0"][b].copy()
        for k in range(N):
            kk = k if broken[b] else 0
            e[b, k] = Cm[b, kk] @ x + tight[b] * (0.05 + 0.5 * np.abs(rng.standard_normal(mk)))
            x = A[b, kk] @ x
    w["A"] = np.ascontiguousarray(A[:, :1])
    w["C"] = np.ascontiguousarray(Cm[:, :1])
    if general:
        w["D"] = np.ascontiguousarray(w["D"][:, :1])
    else:
        w["wx"] = w["targets"] = w["D"] = None
    return w


def cut(w, count):
    out = dict(w)
    for k in OPERANDS:
        if isinstance(w.get(k), np.ndarray):
            out[k] = w[k][:count]
    return out


def tiled(w, count):
    out = dict(w)
    for k in OPERANDS:
        if isinstance(w.get(k), np.ndarray):
            v = w[k]
            out[k] = np.ascontiguousarray(np.concatenate([v] * (count // len(v) + 1))[:count])
    return out


def solve(w, max_iter=None):
    """(U, lam, status, iters) of the forced four-per-wavefront launch, as numpy arrays"""
    import torch
    from qpmpc_amd import _capi, solve_mpc_batch
    from qpmpc_amd import workloads as W

    plan = solve_mpc_batch(W.to_batch_problem(w), return_multipliers=True, max_iter=max_iter, flags=_capi.OPT_FOUR_PER_WAVE)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (plan.U, plan.multipliers, plan.status, plan.iters))


def solve_model(x0):
    """the same through a shared model factored from the humanoid problem (qpmpc_amd.workloads.humanoid_matrices)"""
    import torch
    from qpmpc_amd import SharedModel, _capi
    from qpmpc_amd import workloads as W

    w = W.humanoid_batch(len(x0))
    w["x0"] = x0
    bp = W.to_batch_problem(w)
    plan = SharedModel(bp).solve(bp.initial_state, bp.goal_state, bp.target_states, return_multipliers=True, flags=_capi.OPT_FOUR_PER_WAVE)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (plan.U, plan.multipliers, plan.status, plan.iters))


def run_set(name, sets):
    """what the kernel computes NOW for set `name` of the operand dictionary `sets` (lean16_slim: all SLIM_BATCH problems)"""
    base = sets["lean16"]
    if name == "lean16":
        return solve(base, MAX_ITER_MAIN)
    if name == "lean16_cut5":
        return solve(cut(base, 5), MAX_ITER_MAIN)
    if name == "lean16_mi5":
        return solve(base, 5)
    if name == "lean16_slim":
        return solve(tiled(base, SLIM_BATCH), MAX_ITER_MAIN)
    if name == "model":
        return solve_model(sets["model"]["x0"])
    return solve(sets[name])


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


def pack(sets, results, seed):
    out = {"seed": np.int64(seed)}
    for name, w in sets.items():
        for k in OPERANDS:
            if isinstance(w.get(k), np.ndarray):
                out[f"{name}__{k}"] = w[k]
        for k in ("N", "wt", "wx", "wu"):
            if k in w:
                out[f"{name}__{k}"] = np.float64(-1.0 if w[k] is None else w[k])
    for name, res in results.items():
        for k, v in zip(OUTPUTS, res):
            out[f"{name}__out_{k}"] = v
    return out


def unpack(z):
    """(operand dictionaries by set, recorded outputs by set) of the loaded fixture"""
    sets, results = {}, {}
    for name in ("lean16", "lean9", "gen12", "model"):
        w = {k: (z[f"{name}__{k}"] if f"{name}__{k}" in z.files else None) for k in OPERANDS}
        for k in ("N", "wt", "wx", "wu"):
            if f"{name}__{k}" in z.files:
                v = float(z[f"{name}__{k}"])
                w[k] = int(v) if k == "N" else (None if v < 0 else v)
        sets[name] = w
    for name in SETS:
        results[name] = tuple(z[f"{name}__out_{k}"] for k in OUTPUTS)
    return sets, results


def main():
    from qpmpc_amd import workloads as W

    for seed in range(400):
        rng = np.random.default_rng(20261019 + seed)
        sets = {"lean16": mixed_family(rng, 64, 3, 1, 16, 2, False)}
        res = solve(sets["lean16"], MAX_ITER_MAIN)
        failed = conditions(*res)
        print("seed", seed, "statuses", np.bincount(res[2], minlength=4), "fails:", failed, flush=True)
        if not failed:
            break
    else:
        raise SystemExit("no seed satisfied the conditions")
    sets["lean9"] = mixed_family(rng, 32, 3, 1, 9, 2, False)
    sets["gen12"] = mixed_family(rng, 32, 4, 1, 12, 2, True)
    sets["model"] = {"x0": 2.0 * W.humanoid_batch(32, seed=20261019 + seed)["x0"]}  # (twice the sweep's range: 0 .. 19 iterations)
    results = {name: run_set(name, sets) for name in SETS}
    again = {name: run_set(name, sets) for name in SETS}  # (the kernel is deterministic: the bits of a second launch)
    for name in SETS:
        for a, b in zip(results[name], again[name]):
            assert a.tobytes() == b.tobytes(), name
    slim = results["lean16_slim"]
    for v in slim:  # every tile of the slim launch: the same bits
        ref = np.concatenate([v[:64]] * (SLIM_BATCH // 64 + 1))[:SLIM_BATCH]
        assert ref.tobytes() == v.tobytes(), "slim tiles differ"
    results["lean16_slim"] = tuple(v[:64] for v in slim)
    for name in SETS:
        st, it = results[name][2], results[name][3]
        print(f"{name:12s} statuses {np.bincount(st, minlength=4)} iters mean {it.mean():.2f} max {it.max()}")
    assert (results["lean16_mi5"][2] == 1).any()
    np.savez_compressed(PATH, **pack(sets, results, seed))
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
