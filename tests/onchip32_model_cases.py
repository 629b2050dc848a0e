"""Inputs of the tests of the shared-model mode of csrc/mpcqp_duo.hip (17 .. 32 variables on chip, two problems per wavefront, the
rows of M and L^-T read from a factored model); test helper, NumPy only, no GPU. tests/test_onchip32_model_cpu.py holds these
inputs, on the C oracle, to the conditions that make a green GPU test (tests/test_gpu_onchip32_model.py) mean something.

Cases: nine problems of operand_layouts.model_case(shape, variant) -- A, B, C, D shared and per step; x0, goal, targets and e per
problem or shared, the odd variants behind padded batch strides -- for every shape of SHAPES, verdict_cases.model_mixed for the
verdicts, and many(count): `count` problems on the shared matrices of variant 0 of (3, 1, 24, 2) for the batch-size tests."""
from __future__ import annotations

import functools

import numpy as np

import operand_layouts as OL

SHAPES = (  # ((nx, nu, N, mk), why): each a place where the model prologue can go wrong
    ((3, 1, 17, 2), "n = 17: odd row stride, the first variable of the second lane row; m = 34"),
    ((3, 1, 24, 2), "the plain case"),
    ((3, 1, 32, 2), "full: n = 32, m = 64"),
    ((2, 1, 32, 1), "one row per step, the second M row empty"),
    ((4, 3, 7, 2), "n = 21: lanes without a variable"),
    ((3, 1, 21, 3), "m = 63"),
    ((3, 2, 10, 5), "five rows per step: outside the fused build's envelope"),
    ((4, 2, 9, 6), "six rows per step"),
    ((6, 2, 12, 3), "nx = 6: no fused instantiation"),
    ((12, 2, 10, 2), "nx = 12: rows of Wt of 120 entries"),
    ((16, 4, 6, 2), "nx = 16"),
)
VARIANTS = tuple(range(len(OL.MODEL_VARIANTS)))
PLAIN = (3, 1, 24, 2)
VERDICT_SHAPES = ((3, 1, 24, 2), (4, 2, 16, 2))
# what tests/golden/onchip32_model_default_parent.npz and onchip32_fused_parent.npz were captured on
# (tools/gen_golden_onchip32_parent.py): the first variant that shares e (the export without bounds runs on it), and two
# families of onchip32_cases
DEFAULT_GOLDEN_VARIANT = 3
FUSED_GOLDEN = (((3, 1, 24, 2), "lean", 0.05, False), ((4, 2, 16, 2), "general", 0.2, False))
MANY = 61          # several wavefronts and an idle half
MANY_SEED = 4100
MANY_MARGIN = 0.2
# the walking loop of the GPU test: the reference's walking controller sampled twice as fine over the same 1.6 s horizon
WALK = dict(walkers=24, nb_timesteps=32, sampling_period=0.05, periods=40, seed=11, compared=8)


@functools.lru_cache(maxsize=None)
def case(shape, variant):
    """(w, full) of operand_layouts.model_case, made once"""
    return OL.model_case(shape, variant)


@functools.lru_cache(maxsize=None)
def reference(shape, variant):
    """(U, lam, status, iters) of the C oracle on the materialised problems of a case"""
    import oracle

    return oracle.solve_workload(case(shape, variant)[1])


def shares_e(variant):
    return OL.MODEL_VARIANTS[variant]["e"] == "1"


@functools.lru_cache(maxsize=None)
def many(count=MANY):
    """(w, full): `count` problems on the shared A, B, C, D of variant 0 of PLAIN; x0, goal and targets drawn like
    qpmpc_amd.workloads.random_ltv's, e per problem as operand_layouts.make states it: e = C x_free + margin (0.05 + 0.5 |N(0, 1)|), so
    that u = 0 is feasible for every problem. The first problems of a larger count are those of a smaller one."""
    nx, nu, N, mk = PLAIN
    w9, _ = case(PLAIN, 0)
    rng = np.random.default_rng(MANY_SEED)
    x0 = rng.standard_normal((MANY, nx))
    goal = rng.standard_normal((MANY, nx))
    targets = rng.standard_normal((MANY, N * nx))
    slack = MANY_MARGIN * (0.05 + 0.5 * np.abs(rng.standard_normal((MANY, N, mk))))
    e = np.empty((MANY, N, mk))
    for b in range(MANY):
        x = x0[b].copy()
        for k in range(N):
            e[b, k] = w9["C"][0, k] @ x + slack[b, k]
            x = w9["A"][0, k] @ x
    w = dict(w9)
    w.update(x0=x0[:count].copy(), goal=goal[:count].copy(), targets=targets[:count].copy(), e=e[:count].copy())
    full = dict(w)
    for X in ("A", "B", "C", "D"):
        full[X] = np.ascontiguousarray(np.broadcast_to(w[X], (count,) + w[X].shape[1:]))
    return w, full


@functools.lru_cache(maxsize=None)
def many_reference(count=MANY):
    import oracle

    return oracle.solve_workload(many(count)[1])


def take(w, idx):
    """the problems `idx` of a shared-model workload, in that order. The shared operands stay, and so do the bounds the model is
    factored with ("e_model": the first problem's of `w`; the model's Hx = e - (e - C Phi) rounds with them)"""
    out = dict(w)
    out["e_model"] = w.get("e_model", w["e"][:1])
    for k in ("x0", "goal", "targets", "e"):
        if w[k] is not None and w[k].shape[0] > 1:
            out[k] = np.ascontiguousarray(w[k][idx])
    return out


def drops(lam, iters, ok):
    """number of items of `ok` whose iteration count exceeds their number of positive multipliers: a partial step or drop ran"""
    return int((np.asarray(iters)[ok] > (np.asarray(lam)[ok] > 0).sum(axis=1)).sum())


def clear(full, U, lam, st, tol=1e-6):
    """mask of the clear problems by onchip32_cases.clear's rule: solved, the smallest positive multiplier scaled by 1 + max lam
    above 1e-6, and the smallest inactive slack scaled by 1 + |slack| above 1e-6"""
    from oracle import condense_np
    from qpmpc_amd.workloads import problem_from_workload

    out = np.zeros(len(st), dtype=bool)
    for b in np.flatnonzero(st == 0):
        cq = condense_np.condense(problem_from_workload(full, int(b)))
        act = lam[b] > 0
        slack = np.asarray(cq.h - cq.G @ U[b], dtype=np.float64)
        ok = True
        if act.any():
            ok = lam[b][act].min() / (1.0 + lam[b].max()) > tol
        if ok and (~act).any():
            s = slack[~act]
            ok = (s / (1.0 + np.abs(s))).min() > tol
        out[b] = ok
    return out


# ---------------------------------------------------------------------------------------------- the walking loop
@functools.lru_cache(maxsize=None)
def _walkers():
    rng = np.random.default_rng(WALK["seed"])
    W = WALK["walkers"]
    strides = np.stack([-rng.uniform(0.12, 0.2, W), rng.uniform(0.12, 0.2, W)], axis=1)
    foot = rng.uniform(0.05, 0.08, W)
    index = rng.integers(0, 8, W)
    return strides, foot, index


def walk_kwargs():
    """strides, foot sizes and phase indices of the walkers, drawn as tests/test_gpu_parity.py draws those of its shared-model
    loop (support foot and stride index: the reference's initial ones)"""
    strides, foot, index = _walkers()
    return dict(strides=strides.copy(), foot_size=foot.copy(), index=index.copy())


def oracle_walk(i, solve):
    """(states [periods + 1, 3], inputs, statuses) of walker i through the restated reference loop (oracle/lipm_np.py) with
    ``solve(problem) -> U | None``"""
    from oracle import lipm_np as LN

    strides, foot, index = _walkers()
    p = LN.parameters(strides=tuple(strides[i]), foot_size=float(foot[i]), nb_timesteps=WALK["nb_timesteps"],
                      sampling_period=WALK["sampling_period"])
    return LN.closed_loop(p, LN.new_walker(p, index=int(index[i])), LN.initial_state(p), WALK["periods"], solve=solve)
