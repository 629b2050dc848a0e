"""Inputs for the verdict contract of include/mpcqp.h (test helper, NumPy only, no GPU): status[b] and iters[b] are written for
every problem, U of a problem with status[b] != 0 is all zeros, and MpcqpSolveOpts.max_iter bounds the work per problem.

Every case starts from the nine materialised problems `full` of operand_layouts.route_case(route, 0) (all solved, at least six
with a binding row: tests/test_operand_layouts_cpu.py):

  mixed(full)       items 1, 6 and 7 made infeasible by a pair of rows at step k = N // 2 whose normals are exact negatives and
                    whose bounds are both -1: condensed, g.u <= h0 and -g.u <= h1 with h0 + h1 = -2, infeasible by the Farkas
                    vector (1, 1) whatever the dynamics are. Item 1 shares a wavefront with solvable items at two and at four
                    problems per wavefront, 6 and 7 fill one two-per-wavefront slot and share a four-per-wavefront slot with 4
                    and 5, and item 8 sits alone in the ragged last wavefront.
  indefinite(full)  the clean problems with a terminal weight of -50: P is indefinite, MPCQP_NOT_PD for all nine.
  choose_limit(c)   the iteration limit k that splits a launch's own counts c into at least two items clearly below it and two
                    clearly above it.

tests/test_verdict_cases_cpu.py shows on the C oracle that the inputs are what they claim to be;
tests/test_gpu_verdicts.py launches them through every forward route."""
from __future__ import annotations

import numpy as np

import operand_layouts as OL

INFEASIBLE = (1, 6, 7)
GOOD = tuple(b for b in range(OL.BATCH) if b not in INFEASIBLE)
MIXED_STATUS = np.array([2 if b in INFEASIBLE else 0 for b in range(OL.BATCH)], dtype=np.int32)
W_TERMINAL_INDEFINITE = -50.0
DENSE_SIZES = ((10, 24, False, 1e-7), (40, 90, False, 1e-7), (96, 203, True, 2e-3), (100, 300, True, 2e-3), (160, 512, False, 1e-8),
               (256, 1024, True, 2e-3))  # (n, m, float32, bound) of tests/test_gpu_memory_discipline.py::test_dense_qp_solver


def _copy(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def distinct_cases():
    """route names grouped by the problems they share: {case key: [routes]}"""
    groups = {}
    for route in OL.ROUTES:
        groups.setdefault(OL.route_case(route, 0)[0], []).append(route)
    return groups


def mixed(full):
    """(the batch with items INFEASIBLE made infeasible, the step k that holds the row pair)"""
    w = _copy(full)
    k = int(w["N"]) // 2
    assert w["e"].shape[0] == OL.BATCH and w["e"].shape[-1] >= 2
    for b in INFEASIBLE:
        for X in ("C", "D"):
            if w[X] is not None:
                w[X][b, k, 1] = -w[X][b, k, 0]
        w["e"][b, k, 0] = w["e"][b, k, 1] = -1.0
    return w, k


def indefinite(full):
    w = _copy(full)
    w["wt"] = W_TERMINAL_INDEFINITE
    return w


def condensed_row_pair(w, b, k):
    """(G0, G1, h0, h1): rows 0 and 1 of step k of problem b condensed in np.longdouble, G_r = C_r Psi_k + D_r (block k),
    h_r = e_r - C_r Phi_k x0 with x_{j+1} = A_j x_j + B_j u_j (the roll-out of oracle/condense_np.py, restated)"""
    LD = np.longdouble
    N = int(w["N"])
    nx, nu = w["A"].shape[-1], w["B"].shape[-1]
    Psi, x = np.zeros((nx, N * nu), dtype=LD), w["x0"][b].astype(LD)
    for j in range(k):
        A, B = w["A"][b, j].astype(LD), w["B"][b, j].astype(LD)
        Psi = A @ Psi
        Psi[:, j * nu:(j + 1) * nu] += B
        x = A @ x
    out = []
    for r in (0, 1):
        g, h = np.zeros(N * nu, dtype=LD), LD(w["e"][b, k, r])
        if w["C"] is not None:
            c = w["C"][b, k, r].astype(LD)
            g, h = g + c @ Psi, h - c @ x
        if w["D"] is not None:
            g[k * nu:(k + 1) * nu] += w["D"][b, k, r].astype(LD)
        out.append((g, h))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def condensed(w, b):
    """the condensed QP of problem b of a workload (oracle/condense_np.py)"""
    from oracle import condense_np
    from qpmpc_amd.workloads import problem_from_workload

    return condense_np.condense(problem_from_workload(w, b))


def active_counts(lam):
    """a[b]: the number of multipliers of problem b above 1e-6 (1 + max lam[b])"""
    lam = np.asarray(lam, dtype=np.float64)
    return (lam > 1e-6 * (1.0 + lam.max(axis=1, keepdims=True))).sum(axis=1)


def interior(w):
    """mask of the problems whose unconstrained minimiser -P^-1 q satisfies every row with a margin of 1e-6: no iteration"""
    out = np.zeros(w["x0"].shape[0], dtype=bool)
    for b in range(len(out)):
        cq = condensed(w, b)
        u = -np.linalg.solve(cq.P, cq.q)
        out[b] = bool((cq.h - cq.G @ u >= 1e-6).all())
    return out


def choose_limit(c):
    """(k, below, above): the limit k that maximises min(#{c <= k - 1}, #{c >= k + 1}), the smallest such k; (None, 0, 0) if no k
    leaves two items on either side"""
    c = np.asarray(c)
    best = (None, 0, 0)
    for k in range(1, int(c.max()) + 1):
        lo, hi = int((c <= k - 1).sum()), int((c >= k + 1).sum())
        if min(lo, hi) >= 2 and min(lo, hi) > min(best[1], best[2]):
            best = (k, lo, hi)
    return best


def boundary_limits(c, a, k, most=4):
    """further limits, each the count c[b] of an item: under max_iter = c[b] item b sits exactly on the boundary. First the counts
    of the items with c[b] > a[b] -- such an item took a partial step, so its wavefront made a trip for it that its own count
    does not hold, and a limit compared with anything but the item's own count gives it up --, the largest c[b] - a[b] first, at
    most `most` of them; a route without such an item gets the median count (or the next one above or below it that is not k)."""
    c, a = np.asarray(c), np.asarray(a)
    order = sorted((b for b in range(len(c)) if c[b] > a[b]), key=lambda b: (-(c[b] - a[b]), b))
    out = []
    for b in order:
        if int(c[b]) not in out and int(c[b]) != k and len(out) < most:
            out.append(int(c[b]))
    if not out:
        ranked = sorted(set(int(v) for v in c if v > 0), key=lambda v: (abs(v - float(np.median(c))), v))
        out = [v for v in ranked if v != k][:1]
    return out


# ---------------------------------------------------------------------------------------------- the shared-model export
def model_mixed(shape):
    """(w, full, k) for mpcqp_solve_model_bounds_batch: variant 0 of operand_layouts.model_case (A, B, C, D shared, per step; x0,
    goal, targets, e per problem). The model is shared, so every problem gets the band: row 1 of C and D at step k is the negative
    of row 0. e of the good items is recomputed as make() does, e_r = C_r x_free + slack_r with the slack the row had before, so
    u = 0 stays feasible (-slack_1 <= C_0 (x - x_free) + D_0 u <= slack_0); e of items INFEASIBLE is -1, -1."""
    w, full = OL.model_case(shape, 0)
    w, full = _copy(w), _copy(full)
    N = int(w["N"])
    k = N // 2
    assert w["C"].shape[0] == 1 and w["e"].shape[0] == OL.BATCH
    c1_old = w["C"][0, k, 1].copy()
    for X in ("C", "D"):
        w[X][0, k, 1] = -w[X][0, k, 0]
        full[X][:, k, 1] = -full[X][:, k, 0]
    for b in range(OL.BATCH):
        if b in INFEASIBLE:
            w["e"][b, k, :2] = -1.0
            continue
        x = full["x0"][b].copy()
        for j in range(k):
            x = full["A"][b, j] @ x
        slack = w["e"][b, k, 1] - c1_old @ x
        assert slack > 0
        w["e"][b, k, 1] = w["C"][0, k, 1] @ x + slack
    full["e"] = w["e"].copy()
    return w, full, k


# ---------------------------------------------------------------------------------------------- the dense-QP export
def dense_mixed(n, m):
    """(P, q, G, h) of nine dense QPs drawn like tests/guarded_launch.py::_dense_qps (h > 0: x = 0 is feasible), rows 0 and 1
    of items INFEASIBLE overwritten: G_1 = -G_0, h_0 = h_1 = -1"""
    rng = np.random.default_rng(n + m)
    Ps, qs, Gs, hs = [], [], [], []
    for _ in range(OL.BATCH):
        M = rng.standard_normal((n, n))
        Ps.append(M @ M.T / n + 0.1 * np.eye(n))
        qs.append(rng.standard_normal(n))
        Gs.append(rng.standard_normal((m, n)))
        hs.append(np.abs(rng.standard_normal(m)) * 0.2 + 0.05)
    P, q, G, h = (np.stack(a) for a in (Ps, qs, Gs, hs))
    for b in INFEASIBLE:
        G[b, 1] = -G[b, 0]
        h[b, :2] = -1.0
    return P, q, G, h
