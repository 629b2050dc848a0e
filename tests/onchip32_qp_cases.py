"""Inputs of the tests of mpcqp_solve_batch with MPCQP_OPT_ON_CHIP_32 (csrc/mpcqp_duo.hip, its QP-given mode: dense QPs of up to
32 variables and 64 rows on chip, two problems per wavefront); test helper, NumPy only, no GPU.
tests/test_onchip32_qp_cpu.py holds these inputs, on the C oracle, to the conditions that make a green GPU test
(tests/test_gpu_onchip32_qp.py) mean something.

Every size is verdict_cases.dense_mixed(n, m): nine problems seeded by n + m, items 1, 6 and 7 infeasible. Nine is odd, so the last
wavefront's second half is idle."""
from __future__ import annotations

import functools

import numpy as np

import verdict_cases as VC

SIZES = (  # ((n, m), what it exercises)
    ((1, 2), "degenerate padding"),
    ((2, 3), "degenerate padding"),
    ((16, 32), "below the old envelope"),
    ((17, 2), "odd stride, nearly no rows"),
    ((17, 33), "one row in the second register row"),
    ((20, 64), "active set reaches n"),
    ((24, 48), "mid-range size"),
    ((31, 63), "odd everything"),
    ((32, 32), "no second row"),
    ((32, 64), "full; one item fills all 32 slots"),
)
CROSS_ROUTE = ((17, 33), (24, 48), (32, 64))
MPC_SHAPES = ((6, 2, 12, 2), (5, 1, 20, 2), (8, 2, 10, 6))  # outside the fused flag's envelope: nx >= 5, six rows per step
MPC_SEED, MPC_BATCH, MPC_TIGHT = 7, 9, 0.3
CLEAR = 1e-6
TOL = 1e-7  # float64 dense QPs: verdict_cases.DENSE_SIZES
INDEFINITE_ITEM, INDEFINITE_ENTRY, INDEFINITE_SHIFT = 3, 5, 50.0


@functools.lru_cache(maxsize=None)
def qps(n, m):
    """(P, q, G, h) of the nine problems of a size; read-only"""
    out = VC.dense_mixed(n, m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(n, m):
    """(x, lam, status, iters) of the C oracle on a size, solved once"""
    import oracle

    P, q, G, h = qps(n, m)
    res = [oracle.gi_solve(P[b], q[b], G[b], h[b]) for b in range(len(q))]
    out = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], dtype=np.int32),
           np.array([r[3] for r in res], dtype=np.int32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def clear(n, m):
    """mask of the CLEAR problems of a size: solved by the oracle, its smallest positive multiplier over 1 + max lam above 1e-6, and
    its smallest inactive slack over 1 + |slack| above 1e-6 (onchip32_cases.clear on a QP that is given)"""
    P, q, G, h = qps(n, m)
    x, lam, st, _ = reference(n, m)
    out = np.zeros(len(st), dtype=bool)
    for b in np.flatnonzero(st == 0):
        act = lam[b] > 0
        slack = h[b] - G[b] @ x[b]
        ok = True
        if act.any():
            ok = lam[b][act].min() / (1.0 + lam[b].max()) > CLEAR
        if ok and (~act).any():
            s = slack[~act]
            ok = (s / (1.0 + np.abs(s))).min() > CLEAR
        out[b] = ok
    return out


def drops(n, m):
    """number of solved items of a size whose iterations exceed their positive multipliers on the oracle"""
    _, lam, st, it = reference(n, m)
    ok = st == 0
    return int((it[ok] > (lam[ok] > 0).sum(axis=1)).sum())


def indefinite(n, m):
    """the problems of a size with P[5][5] of item 3 lowered by 50: that item's P is indefinite"""
    P, q, G, h = (a.copy() for a in qps(n, m))
    P[INDEFINITE_ITEM, INDEFINITE_ENTRY, INDEFINITE_ENTRY] -= INDEFINITE_SHIFT
    return P, q, G, h


@functools.lru_cache(maxsize=None)
def mpc_family(shape):
    from qpmpc_amd.workloads import random_ltv

    nx, nu, N, mk = shape
    return random_ltv(np.random.default_rng(MPC_SEED), MPC_BATCH, nx, nu, N, mk, MPC_TIGHT)


@functools.lru_cache(maxsize=None)
def mpc_reference(shape):
    import oracle

    return oracle.solve_workload(mpc_family(shape))
