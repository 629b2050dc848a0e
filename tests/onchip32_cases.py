"""Inputs of the tests of MPCQP_OPT_ON_CHIP_32 (csrc/mpcqp_duo.hip: 17 .. 32 variables on chip, two problems per wavefront); test
helper, NumPy only, no GPU. tests/test_onchip32_cpu.py holds these inputs, on the C oracle, to the conditions that make a green
GPU test (tests/test_gpu_onchip32.py) mean something.

Families: 61 problems of qpmpc_amd.workloads.random_ltv(rng, 61, nx, nu, N, mk, tight) with rng = default_rng(1000 nx + 10 N + nu),
at tightness 3.0, 0.2 and 0.05, each once per step and once time-invariant (A and C reduced to their first step, as
tests/test_gpu_quad.py::_lean_family does). "lean": terminal cost only, state rows only (wx = targets = D = None); "general": C and
D rows and a stage cost.

The per-step families are solved throughout by the oracle. Reducing A and C to one step leaves the bounds e as they were drawn
around the per-step free response, so some time-invariant families hold problems whose rows are inconsistent (up to 46 of 61):
their verdicts (MPCQP_INFEASIBLE) are compared like every other, and the conditions on solved problems (drops, clear share) are
stated on the solved ones."""
from __future__ import annotations

import functools

import numpy as np

BATCH = 61
TIGHT = (3.0, 0.2, 0.05)
SHAPES = (  # ((nx, nu, N, mk), family, why)
    ((3, 1, 17, 2), "lean", "the first variable in the second lane row; m = 34"),
    ((3, 1, 24, 2), "lean", ""),
    ((3, 1, 32, 2), "lean", "full: n = 32, m = 64"),
    ((2, 1, 32, 1), "lean", "one row per step"),
    ((4, 2, 9, 2), "general", "C + D rows, stage cost; n = 18, the second M row empty"),
    ((4, 2, 16, 2), "general", ""),
    ((4, 3, 7, 2), "general", "n = 21: the last lanes own no variable"),
    ((3, 1, 20, 3), "general", "m = 60"),
    ((3, 1, 21, 3), "general", "m = 63"),
)
FAMILIES = tuple((shape, kind, tight, lti) for shape, kind, _ in SHAPES for tight in TIGHT for lti in (False, True))
CLEAR = 1e-6
VERDICT_SHAPES = ((3, 1, 24, 2), (4, 2, 16, 2))  # the shapes of the verdict tests of tests/test_gpu_onchip32.py
# |lam - lam_ref| / (1 + max lam_ref) on the clear problems. Measured on an MI355X over the 54 families: 8.9e-9 for the default
# route on these problems (the stage-wise kernels; worst on the time-invariant (3, 1, 32, 2) family at 0.05, whose condensed
# Hessian is the worst conditioned) and 3.4e-10 for the flagged launch (the same family at 0.2). The bound is ten times the
# default route's worst value (sums of up to 32 terms in another order, one refinement step), never below 1e-9:
LAM_DEFAULT_ROUTE_WORST = 8.9e-9
LAM_BOUND = max(1e-9, 10 * LAM_DEFAULT_ROUTE_WORST)


@functools.lru_cache(maxsize=None)
def family(shape, kind, tight, lti):
    from qpmpc_amd.workloads import random_ltv

    nx, nu, N, mk = shape
    rng = np.random.default_rng(1000 * nx + 10 * N + nu)
    w = random_ltv(rng, BATCH, nx, nu, N, mk, tight)
    if kind == "lean":
        w["wx"] = w["targets"] = w["D"] = None
    if lti:  # time-invariant A, C (stride 0 along the horizon)
        w["A"] = np.ascontiguousarray(w["A"][:, :1])
        w["C"] = np.ascontiguousarray(w["C"][:, :1])
    return w


@functools.lru_cache(maxsize=None)
def reference(shape, kind, tight, lti):
    """(U, lam, status, iters) of the C oracle on a family, solved once"""
    import oracle

    return oracle.solve_workload(family(shape, kind, tight, lti))


def materialised(w):
    """the same problems with A and C stated for every step"""
    N = int(w["N"])
    full = dict(w)
    for X in ("A", "C"):
        if w[X] is not None and w[X].shape[1] == 1:
            full[X] = np.ascontiguousarray(np.broadcast_to(w[X], (w[X].shape[0], N) + w[X].shape[2:]))
    return full


@functools.lru_cache(maxsize=None)
def clear(shape, kind, tight, lti):
    """mask of the CLEAR problems of a family: solved by the oracle, its smallest positive multiplier, scaled by 1 + max lam, above
    1e-6, and its smallest inactive slack, scaled by 1 + |slack|, above 1e-6 -- problems whose active set is not a matter of
    rounding"""
    from oracle import condense_np
    from qpmpc_amd.workloads import problem_from_workload

    w = materialised(family(shape, kind, tight, lti))
    U, lam, st, _ = reference(shape, kind, tight, lti)
    out = np.zeros(BATCH, dtype=bool)
    for b in np.flatnonzero(st == 0):
        cq = condense_np.condense(problem_from_workload(w, int(b)))
        act = lam[b] > 0
        slack = np.asarray(cq.h - cq.G @ U[b], dtype=np.float64)
        ok = True
        if act.any():
            ok = lam[b][act].min() / (1.0 + lam[b].max()) > CLEAR
        if ok and (~act).any():
            s = slack[~act]
            ok = (s / (1.0 + np.abs(s))).min() > CLEAR
        out[b] = ok
    return out


def drops(lam, iters, ok):
    """number of items of `ok` whose iteration count exceeds their number of positive multipliers: a partial step or drop ran"""
    return int((np.asarray(iters)[ok] > (np.asarray(lam)[ok] > 0).sum(axis=1)).sum())


# the operand-layout cases: the nine problems of operand_layouts.make((3, 1, 24, 2), "cd", True, i, LAYOUT_SEED + i, LAYOUT_MARGIN)
LAYOUT_SHAPE, LAYOUT_SEED, LAYOUT_MARGIN = (3, 1, 24, 2), 1000, 0.2


@functools.lru_cache(maxsize=None)
def layout_case(i):
    import operand_layouts as OL

    return OL.make(LAYOUT_SHAPE, "cd", True, i, LAYOUT_SEED + i, LAYOUT_MARGIN)


@functools.lru_cache(maxsize=None)
def layout_reference(i):
    import oracle

    return oracle.solve_workload(layout_case(i)[1])[:3]
