"""Degenerate active sets for every forward route (test helper, NumPy only, no GPU, no fixtures): problems on which the linear
dependence, ratio-test and drop branches of a dual active-set kernel decide the outcome -- exact ties, rows through the optimum,
duplicated rows, zero-width bands -- and whose answer is nevertheless known.

The condensed Hessian is positive definite, so the minimiser is unique even where the multipliers are not. Moving the bound of a
row that is inactive at the optimum u* onto u*, rounded OUTWARD, only shrinks the feasible set around a point that stays feasible:
u* is still the exact answer, whatever way a solver breaks the ties. Every variant starts from `full`, the nine materialised
problems of operand_layouts.route_case(route, 0), and the C oracle's (Uo, lamo) on it:

  touch(full, Uo, lamo, steps, f32)  e of every row of the chosen steps whose oracle multiplier is zero becomes up(row value at
                                     Uo). Exact answer: Uo. TOUCH_STEPS holds the steps per route (None: all of them).
  free(full, f32)                    every row of every step is touched at the unconstrained minimiser u0 = -P^-1 q (which
                                     replaces every bound: none is left to loosen first). Exact answer: u0, with no active row.
  duplicate(full, Uo, f32)           step N // 2: row 1 of C and D becomes row 0 (e_1 = e_0); step N // 4: row 1 becomes exactly
                                     2 x row 0 with e_1 = 2 e_0. In both places e_0 is set BELOW the row's value at Uo, so the
                                     pair binds. No closed-form answer: the reference is the oracle on the variant.
  band(full, Uo, f32)                step N // 2: row 1 is the exact negative of row 0 with e_1 = -e_0, e_0 tightened as in
                                     duplicate: a zero-width band, an equality written as two inequalities. include/mpcqp.h calls
                                     a row violated only when (h_i - G_i u) / (1 + |h_i|) < -feas_tol, so this is feasible.
                                     Reference: the oracle on the variant.

Row values at a plan are formed in np.longdouble by roll-out, C_k x_k + D_k u_k. up(value, f32) rounds to the storage type and,
if the result is below the long-double value, steps to the next representable number above: a float32 route's variant is stated
in float32-representable numbers throughout (operand_layouts.f32_view of it is a no-op). Rounding to nearest instead leaves the
touched rows violated by up to 6e-8, and the float64 oracle then calls such items infeasible.

The same constructions serve the shared-model export (operand_layouts.model_case(shape, 0): the model is shared, so duplicate and
band change rows of every problem, and e is set per problem) and the dense-QP export (the nine QPs of verdict_cases.dense_mixed
before its infeasible rows are written; touch on h, duplicate and band on rows 0 and 1 of G).

tests/test_degenerate_cases_cpu.py shows on the C oracle that each input is what it claims to be; tests/test_gpu_degenerate.py
launches them through every forward route."""
from __future__ import annotations

import numpy as np

import operand_layouts as OL
import verdict_cases as VC

LD = np.longdouble
VARIANTS = ("touch", "free", "duplicate", "band")
# e_0 of a duplicated or banded row: its value at the nominal optimum minus (TIGHTEN_FRACTION x its former slack + TIGHTEN_FLOOR).
# The random families draw slacks of margin (0.05 + 0.5 |N(0, 1)|) with margin 0.2, so the floor is a fifth of the smallest slack.
# Tuned on the C oracle and an LP: at (0.25, 0.01) item 5 of "promoted f32 (3, 1, 16, 2)" has no feasible point under its band
# (the largest margin any u leaves is -0.007), at (0.5, 0.01) three items of three cases; at (0.1, 0.002) every item of every
# case is solvable, and the pair still binds everywhere, because the nominal optimum violates the tightened row.
TIGHTEN_FRACTION, TIGHTEN_FLOOR = 0.1, 0.002
# The dense QPs (bounds 0.05 + 0.2 |N(0, 1)|, x = 0 feasible) replace a row that may have been active, so the new optimum can
# leave the tightened pair again: at (0.1, 0.002) only 5 of 9 items of the 32 x 64 size keep a positive multiplier on the pair.
# At (0.5, 0.01) every item of every size is solvable and at least 7 of 9 keep one.
DENSE_TIGHTEN_FRACTION, DENSE_TIGHTEN_FLOOR = 0.5, 0.01


def spaced(N, count):
    """`count` evenly spaced steps of a horizon of N: the midpoints of `count` equal parts"""
    return tuple((2 * i + 1) * N // (2 * count) for i in range(count))


# route -> the steps whose inactive rows touch() moves onto the optimum (None: every step). Routes with n <= 64 touch every step;
# on the larger ones the oracle's path grows with the number of touched rows (the dense case with all 1024 - active rows touched
# takes 2,600 .. 10,001 iterations), so they touch evenly spaced steps, as many as keep every item's count within n + m
# (tests/test_degenerate_cases_cpu.py::test_iteration_counts).
TOUCH_STEPS = {route: None for route, r in OL.ROUTES.items() if r["shape"][1] * r["shape"][2] <= 64}
TOUCH_STEPS.update({route: spaced(r["shape"][2], 8 if route == "wide stage-wise f32" else 4)
                    for route, r in OL.ROUTES.items() if r["shape"][1] * r["shape"][2] > 64})


def _copy(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def up(value, f32):
    """`value` (long double) rounded to the storage type, then stepped to the next representable number above wherever the
    rounded number is below `value`; returned as float64 (exact for either storage type)"""
    t = np.float32 if f32 else np.float64
    v = np.asarray(value, dtype=LD)
    r = v.astype(t)
    r = np.where(r.astype(LD) < v, np.nextafter(r, t(np.inf)), r).astype(t)
    assert (r.astype(LD) >= v).all()
    return r.astype(np.float64)


def ulp(f32):
    return 2.0 ** -23 if f32 else 2.0 ** -52


def row_values(w, U):
    """[B, N, mk] in np.longdouble: C_k x_k + D_k u_k of every problem along the roll-out x_{k+1} = A_k x_k + B_k u_k of plan U"""
    B, N, mk = w["e"].shape
    nu = w["B"].shape[-1]
    out = np.zeros((B, N, mk), dtype=LD)
    for b in range(B):
        x, u = w["x0"][b].astype(LD), np.asarray(U[b]).reshape(N, nu).astype(LD)
        for k in range(N):
            if w["C"] is not None:
                out[b, k] += w["C"][b, k].astype(LD) @ x
            if w["D"] is not None:
                out[b, k] += w["D"][b, k].astype(LD) @ u[k]
            x = w["A"][b, k].astype(LD) @ x + w["B"][b, k].astype(LD) @ u[k]
    return out


def touch(full, Uo, lamo, steps, f32):
    """(variant, touched [B, N, mk] bool)"""
    w = _copy(full)
    B, N, mk = w["e"].shape
    chosen = np.zeros(N, dtype=bool)
    chosen[list(range(N) if steps is None else steps)] = True
    touched = (np.asarray(lamo).reshape(B, N, mk) == 0) & chosen[None, :, None]
    w["e"][touched] = up(row_values(full, Uo), f32)[touched]
    return w, touched


_COST = {}


def cost_ld(w, b):
    """(P, q) of problem b condensed in np.longdouble: oracle/condense_np.py's loop and cost_vector restated on long doubles
    (the float64 P and q of condense_np are themselves 1e-15 off, which cond(P) multiplies into the minimiser); memoised per
    workload dict and item. Neither depends on e, so a variant shares them with its nominal problems."""
    hit = _COST.get((id(w), b))
    if hit is not None and hit[0] is w:
        return hit[1]
    _COST[(id(w), b)] = (w, _cost_ld(w, b))
    return _COST[(id(w), b)][1]


def _cost_ld(w, b):
    N, nx, nu = int(w["N"]), w["A"].shape[-1], w["B"].shape[-1]
    n = N * nu
    phi, psi, x0 = np.eye(nx, dtype=LD), np.zeros((nx, n), dtype=LD), w["x0"][b].astype(LD)
    P, q = LD(w["wu"]) * np.eye(n, dtype=LD), np.zeros(n, dtype=LD)
    for k in range(N):
        if w["wx"] is not None:
            P = P + LD(w["wx"]) * (psi.T @ psi)
            if w["wx"] > 1e-10 and w["targets"] is not None:
                q = q + LD(w["wx"]) * ((phi @ x0 - w["targets"][b].reshape(N, nx)[k].astype(LD)) @ psi)
        A = w["A"][b, k].astype(LD)
        phi, psi = A @ phi, A @ psi
        psi[:, k * nu:(k + 1) * nu] = w["B"][b, k].astype(LD)
    if w["wt"] is not None:
        P = P + LD(w["wt"]) * (psi.T @ psi)
        if w["wt"] > 1e-10 and w["goal"] is not None:
            q = q + LD(w["wt"]) * ((phi @ x0 - w["goal"][b].astype(LD)) @ psi)
    return P, q


def unconstrained(full):
    """u0 [B, n] in np.longdouble: -P^-1 q with P and q of oracle/condense_np.py restated in long double (cost_ld), by four
    steps of iterative refinement with the float64 factorisation: the residual -q - P u is formed in long double"""
    out = []
    for b in range(full["x0"].shape[0]):
        cq = VC.condensed(full, b)
        P, q = cost_ld(full, b)
        u = -np.linalg.solve(cq.P, cq.q).astype(LD)
        for _ in range(4):
            u = u + np.linalg.solve(cq.P, (-q - P @ u).astype(np.float64)).astype(LD)
        out.append(u)
    return np.stack(out)


def free(full, f32):
    """(variant, u0 [B, n] long double, bound [B, m]): bound is n 2^-53 sum_j |G_ij u0_j| / (1 + |h_i|), the rounding error of a
    float64 evaluation of row i's slack at u0, relative to the scale include/mpcqp.h measures a violation on"""
    w = _copy(full)
    B, N, mk = w["e"].shape
    u0 = unconstrained(full)
    values = row_values(full, u0)
    w["e"] = up(values, f32)  # (every row of every step is touched, so no bound is left that needed loosening first)
    bound = np.empty((B, N * mk))
    for b in range(B):
        cq = VC.condensed(w, b)
        n = cq.G.shape[1]
        bound[b] = n * 2.0 ** -53 * (np.abs(cq.G) @ np.abs(u0[b].astype(np.float64))) / (1.0 + np.abs(cq.h))
    return w, u0, bound


def _tightened(full, Uo, k, f32):
    """e_0 [B] of step k: row 0's value at Uo minus (TIGHTEN_FRACTION x its former slack + TIGHTEN_FLOOR), in the storage type"""
    v = row_values(full, Uo)[:, k, 0]
    slack = np.maximum(full["e"][:, k, 0].astype(LD) - v, 0)
    e0 = (v - (TIGHTEN_FRACTION * slack + TIGHTEN_FLOOR)).astype(np.float32 if f32 else np.float64).astype(np.float64)
    assert (e0.astype(LD) < v).all()
    return e0


def _pair(w, full, Uo, k, factor, f32):
    """row 1 of step k := factor x row 0 (C, D and e), e_0 tightened"""
    assert w["e"].shape[-1] >= 2
    for X in ("C", "D"):
        if w[X] is not None:
            w[X][:, k, 1] = factor * w[X][:, k, 0]
    w["e"][:, k, 0] = _tightened(full, Uo, k, f32)
    w["e"][:, k, 1] = factor * w["e"][:, k, 0]


def duplicate(full, Uo, f32):
    """(variant, [(step, 0), (step, 1), ...] the modified rows)"""
    w = _copy(full)
    N = int(w["N"])
    assert N // 4 != N // 2
    _pair(w, full, Uo, N // 2, 1.0, f32)
    _pair(w, full, Uo, N // 4, 2.0, f32)
    return w, [(N // 2, 0), (N // 2, 1), (N // 4, 0), (N // 4, 1)]


def band(full, Uo, f32):
    w = _copy(full)
    N = int(w["N"])
    _pair(w, full, Uo, N // 2, -1.0, f32)
    return w, [(N // 2, 0), (N // 2, 1)]


# ---------------------------------------------------------------------------------------------- per case, made once
_MADE = {}


def _variant(key, full, Uo, lamo, name, steps, f32):
    """dict(w, exact (U or None; exact_ld: the long doubles the rows were touched at), rows (modified or touched rows, [B, N, mk]
    bool), bound (free only)) of one variant of a case"""
    if (key, name) not in _MADE:
        B, N, mk = full["e"].shape
        out = dict(exact=None, bound=None)
        if name == "touch":
            out["w"], out["rows"] = touch(full, Uo, lamo, steps, f32)
            out["exact"], out["exact_ld"] = Uo, Uo.astype(LD)
        elif name == "free":
            out["w"], out["exact_ld"], out["bound"] = free(full, f32)
            out["exact"] = out["exact_ld"].astype(np.float64)
            out["rows"] = np.ones((B, N, mk), dtype=bool)
        else:
            out["w"], pairs = (duplicate if name == "duplicate" else band)(full, Uo, f32)
            out["rows"] = np.zeros((B, N, mk), dtype=bool)
            for k, r in pairs:
                out["rows"][:, k, r] = True
        _MADE[(key, name)] = out
    return _MADE[(key, name)]


_NOMINAL = {}


def nominal(key, full):
    """(U, lam, status, iters) of the C oracle on a case's nominal problems, solved once (operand_layouts.oracle_on_full keeps no
    iteration counts, which conditions (c) and (d) compare)"""
    import oracle

    if key not in _NOMINAL:
        _NOMINAL[key] = oracle.solve_workload(full)
    return _NOMINAL[key]


def case_variant(key, full, name, steps=None, f32=False):
    """a variant of any nine materialised problems (the shared-model and on-chip groups), keyed by `key`"""
    Uo, lamo, sto, _ = nominal(key, full)
    assert (sto == 0).all(), sto
    return _variant(key, full, Uo, lamo, name, steps, f32)


_SOLVED = {}


def oracle_on(key, name, w):
    """(U, lam, status, iters) of the C oracle on a variant, solved once"""
    import oracle

    if (key, name) not in _SOLVED:
        _SOLVED[(key, name)] = oracle.solve_workload(w)
    return _SOLVED[(key, name)]


def shared(full):
    """the materialised problems of a shared-model case with A, B, C, D stored once"""
    w = dict(full)
    for X in ("A", "B", "C", "D"):
        assert (full[X] == full[X][:1]).all(), X
        w[X] = np.ascontiguousarray(full[X][:1])
    return w


# ---------------------------------------------------------------------------------------------- the dense-QP export
# (n, m) -> every how-manieth row of h touch moves onto the optimum (1: every row with a zero multiplier). The sizes with
# n <= 64 touch every row, the larger ones as many as keep the oracle's count within n + m, as TOUCH_STEPS does.
DENSE_TOUCH_STRIDE = {(10, 24): 1, (40, 90): 1, (96, 203): 4, (100, 300): 4, (160, 512): 8, (256, 1024): 16}


def dense_nominal(n, m, f32):
    """(P, q, G, h) of the nine dense QPs of verdict_cases.dense_mixed, drawn the same way, without its infeasible rows; for a
    float32 size in float32-representable numbers"""
    rng = np.random.default_rng(n + m)
    Ps, qs, Gs, hs = [], [], [], []
    for _ in range(OL.BATCH):
        M = rng.standard_normal((n, n))
        Ps.append(M @ M.T / n + 0.1 * np.eye(n))
        qs.append(rng.standard_normal(n))
        Gs.append(rng.standard_normal((m, n)))
        hs.append(np.abs(rng.standard_normal(m)) * 0.2 + 0.05)
    P, q, G, h = (np.stack(a) for a in (Ps, qs, Gs, hs))
    if f32:
        P, q, G, h = (a.astype(np.float32).astype(np.float64) for a in (P, q, G, h))
    return P, q, G, h


_DENSE = {}


def dense_oracle(key, P, q, G, h):
    """(x [B, n], lam [B, m], status [B], iters [B]) of oracle.gi_solve on nine dense QPs, solved once per key"""
    import oracle

    if key not in _DENSE:
        got = [oracle.gi_solve(P[b], q[b], G[b], h[b]) for b in range(len(P))]
        _DENSE[key] = tuple(np.stack([np.asarray(g[i]) for g in got]) for i in range(4))
    return _DENSE[key]


def dense_variant(n, m, f32, name):
    """dict(qp=(P, q, G, h), exact (x or None), rows [B, m] bool, bound) of a variant of the dense QPs, made once"""
    key = ("dense", n, m, f32, name)
    if key in _MADE:
        return _MADE[key]
    P, q, G, h = dense_nominal(n, m, f32)
    xo, lamo, sto, _ = dense_oracle(("dense", n, m, f32), P, q, G, h)
    assert (sto == 0).all(), sto
    t = np.float32 if f32 else np.float64
    G, h = G.copy(), h.copy()
    out = dict(exact=None, bound=None, rows=np.zeros(h.shape, dtype=bool))
    if name == "touch":
        out["rows"][:, ::DENSE_TOUCH_STRIDE.get((n, m), 1)] = True
        out["rows"] &= lamo == 0
        values = np.einsum("bij,bj->bi", G.astype(LD), xo.astype(LD))
        h[out["rows"]] = up(values, f32)[out["rows"]]
        out["exact"], out["exact_ld"] = xo, xo.astype(LD)
    elif name == "free":
        x0 = []
        for b in range(len(P)):
            x = -np.linalg.solve(P[b], q[b]).astype(LD)
            for _ in range(3):
                x = x + np.linalg.solve(P[b], (-q[b].astype(LD) - P[b].astype(LD) @ x).astype(np.float64)).astype(LD)
            x0.append(x)
        x0 = np.stack(x0)
        h = up(np.einsum("bij,bj->bi", G.astype(LD), x0), f32)
        out["rows"][:] = True
        out["exact"], out["exact_ld"] = x0.astype(np.float64), x0
        out["bound"] = n * 2.0 ** -53 * np.einsum("bij,bj->bi", np.abs(G), np.abs(out["exact"])) / (1.0 + np.abs(h))
    else:
        v = np.einsum("bj,bj->b", G[:, 0].astype(LD), xo.astype(LD))
        slack = np.maximum(h[:, 0].astype(LD) - v, 0)
        h[:, 0] = (v - (DENSE_TIGHTEN_FRACTION * slack + DENSE_TIGHTEN_FLOOR)).astype(t).astype(np.float64)
        factor = 1.0 if name == "duplicate" else -1.0
        G[:, 1] = factor * G[:, 0]
        h[:, 1] = factor * h[:, 0]
        out["rows"][:, :2] = True
    out["qp"] = (P, q, G, h)
    _MADE[key] = out
    return out


# ---------------------------------------------------------------------------------------------- the other groups' cases
ONCHIP_SHAPES = ((3, 1, 24, 2), (4, 2, 16, 2))  # tests/test_gpu_onchip32.py: VERDICT_SHAPES, tests/onchip32_model_cases.py: VERDICT_SHAPES
ONCHIP_QP_SIZES = ((17, 33), (24, 48), (32, 64))  # tests/onchip32_qp_cases.py: CROSS_ROUTE


def onchip_full(shape):
    """the nine general problems tests/test_gpu_onchip32.py::test_verdicts starts from"""
    import onchip32_cases as OC

    return OL.make(shape, "cd", True, 0, OC.LAYOUT_SEED, OC.LAYOUT_MARGIN)[1]


def other_cases():
    """{label: (key, full)}: the materialised nominal problems behind the shared-model group and the on-chip kernel's fused and
    shared-model modes (float64, every step touched: n <= 32)"""
    out = {f"model {shape}": (("model", shape), OL.model_case(shape, 0)[1]) for shape in OL.MODEL_SHAPES + ONCHIP_SHAPES}
    out.update({f"on chip {shape}": (("on chip", shape), onchip_full(shape)) for shape in ONCHIP_SHAPES})
    return out


# `free`: an item is held to 0 iterations only where a float64 minimiser keeps every row within a twentieth of feas_tol = 1e-12
# (two float64 evaluations of one slack differ by about as much as each is off, which leaves a solver's own a factor of twenty)
FREE_SLACK = -5e-14


def min_slack_qp(P, q, G, h):
    """min_slack_f64 of a dense QP"""
    x = -np.linalg.solve(P, q)
    return float(((h - G @ x) / (1.0 + np.abs(h))).min())


def min_slack_f64(w, b):
    """min_i (h_i - G_i u) / (1 + |h_i|) of variant w's problem b at the float64 minimiser u = -P^-1 q as NumPy computes it from
    oracle/condense_np.py's P and q: what a float64 solver sees of rows that sit on the exact minimiser. Its own error in u,
    about cond(P) 2^-53 |u|, enters every slack through G."""
    cq = VC.condensed(w, b)
    u = -np.linalg.solve(cq.P, cq.q)
    return float(((cq.h - cq.G @ u) / (1.0 + np.abs(cq.h))).min())
