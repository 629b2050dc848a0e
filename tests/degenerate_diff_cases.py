"""Degenerate active sets for every derivative export (test helper, NumPy only, no GPU, no fixtures): the variants of
tests/degenerate_cases.py (touch, free, duplicate, band) at the shapes where the adjoint and tangent kernels take their distinct
code paths, the multiplier constructions that state one KKT point of `duplicate` in three ways, and the references.

Cases, nine problems each (operand_layouts.BATCH), every operand materialised per problem:

  kind "condensed"  (3, 2, 8, 2) n = 16: 64 threads, the carve in LDS; (4, 2, 20, 2) n = 40: 256 threads, the carve in LDS;
                    (3, 2, 45, 2) n = 90: the carve in the workspace (mpcqp_adjoint.hip, about n > 78). The exports
                    mpcqp_plan_vjp_batch, mpcqp_plan_vjp_model_batch, mpcqp_plan_jvp_batch, mpcqp_plan_jvp_model_batch.
  kind "stagewise"  (3, 2, 8, 2) and operand_layouts.DIFF_SHAPES[1] = (3, 2, 70, 2), the only one beyond 128 variables, with its
                    contractive draw. mpcqp_plan_vjp_stagewise_batch, mpcqp_plan_jvp_stagewise_batch,
                    mpcqp_plan_jvp_model_stagewise_batch.
  kind "model"      operand_layouts.MODEL_SHAPES (n = 16: the sixteen-lane kernel) and degenerate_cases.ONCHIP_SHAPES[0] =
                    (3, 1, 24, 2) (n = 24: the general kernel); the problems of degenerate_cases.other_cases(), whose model is
                    shared. mpcqp_model_vjp_batch, mpcqp_model_jvp_batch.

The draws: operand_layouts.diff_case(shape, 0) where the shape is one of its DIFF_SHAPES, operand_layouts.model_case(shape, 0)
for the model kind, and for the two shapes in between operand_layouts.make with the seed of SEEDS (margin 0.5, contractive
beyond 40 steps, as diff_case draws). SEEDS records the first seed from 5100 on at which the oracle solves all nine items of
every variant and conditions (a) .. (e) of tests/test_degenerate_diff_cpu.py hold.

A pair (i0, i1, factor) is two rows of one problem with G_i1 = factor G_i0 and h_i1 = factor h_i0: factor 1 (a row stated
twice), 2 (a row and its double) on `duplicate`, -1 on `band` (an equality written as two inequalities). On a binding pair the
multipliers are not unique -- only lam_i0 + factor lam_i1 is -- and neither is the gradient with respect to the pair's own
bounds: g_e[i0] + factor g_e[i1] is, and so is the response to a tangent that moves both bounds together, de[i1] = factor de[i0].

  canonical(lam, pairs)  the whole multiplier of each binding pair on its first member, lam_i0 + factor lam_i1 (factor > 0; a
                         band's multiplier stays where the solver put it: the two members carry opposite signs)
  other(lam, pairs)      ... on its second member, (lam_i0 + factor lam_i1) / factor; on a band the active member swapped
  split(lam, pairs)      both members positive with G' lam unchanged: t / 2 and t / 2 for the exact copy, t / 2 and t / 4 for the
                         doubled row (factor > 0 only). A valid KKT multiplier vector whose active rows are linearly dependent.

unique(g, pairs) folds a gradient over the rows (g_e, or g_C / g_D with a trailing axis) into its unique part: row i0 becomes
g[i0] + factor g[i1], row i1 zero. vjp_ld / jvp_ld are adjoint_np.vjp / tangent_np.jvp with the KKT solve and everything
behind it in np.longdouble (three steps of iterative refinement on the float64 factorisation, residuals in long double);
model_vjp_ld is adjoint_model_np.model_vjp (g_A .. g_D, g_w) on the same long-double solve and long-double roll-outs."""
from __future__ import annotations

import numpy as np

import degenerate_cases as DC
import operand_layouts as OL

LD = np.longdouble
VARIANTS = DC.VARIANTS
CONDENSED = ((3, 2, 8, 2), (4, 2, 20, 2), (3, 2, 45, 2))
STAGEWISE = ((3, 2, 8, 2), OL.DIFF_SHAPES[1])
MODEL = tuple(OL.MODEL_SHAPES) + (DC.ONCHIP_SHAPES[0],)
SEEDS = {(4, 2, 20, 2): 5100, (3, 2, 45, 2): 5100}
CASES = [("plan", s) for s in dict.fromkeys(CONDENSED + STAGEWISE)] + [("model", s) for s in MODEL]
RANK_TOL = 1e-12  # singular values of a Gram matrix below this fraction of the largest count as zero


def label(kind, shape):
    return f"{kind} {shape}"


def case(kind, shape):
    """(key, full, touch steps) of a case: `full` is the nine materialised nominal problems, key what degenerate_cases memoises
    the oracle's solves under. Beyond 64 variables touch moves four evenly spaced steps (degenerate_cases.TOUCH_STEPS)."""
    nx, nu, N, mk = shape
    if kind == "model":
        return ("model", shape), OL.model_case(shape, 0)[1], None
    steps = None if N * nu <= 64 else DC.spaced(N, 4)
    if shape in OL.DIFF_SHAPES:
        return ("diff", shape), OL.diff_case(shape, 0)[1], steps
    return ("diff", shape), OL.make(shape, "cd", True, 0, SEEDS[shape], 0.5, contractive=N > 40)[1], steps


def pairs_of(shape, name):
    """[(i0, i1, factor)] of a variant, rows numbered step * mk + row as lam and g_e number them"""
    nx, nu, N, mk = shape
    if name == "duplicate":
        return [((N // 2) * mk, (N // 2) * mk + 1, 1.0), ((N // 4) * mk, (N // 4) * mk + 1, 2.0)]
    if name == "band":
        return [((N // 2) * mk, (N // 2) * mk + 1, -1.0)]
    return []


_MADE = {}


def variant(kind, shape, name):
    """dict(w: the nine problems, pairs, U, lam, status, iters: the C oracle on them, full, key) of one variant, made once"""
    if (kind, shape, name) not in _MADE:
        key, full, steps = case(kind, shape)
        v = DC.case_variant(key, full, name, steps, False)
        U, lam, st, it = DC.oracle_on(key, name, v["w"])
        _MADE[(kind, shape, name)] = dict(w=v["w"], pairs=pairs_of(shape, name), U=U, lam=lam, status=st, iters=it, full=full,
                                          key=key, exact=v["exact"])
    return _MADE[(kind, shape, name)]


# ---------------------------------------------------------------------------------------------- multipliers of a pair
def binding(lam, pairs):
    """the pairs with a positive multiplier on a member"""
    return [p for p in pairs if lam[p[0]] > 0 or lam[p[1]] > 0]


def both_positive(lam, pairs):
    return sum(1 for i0, i1, f in pairs if lam[i0] > 0 and lam[i1] > 0)


def canonical(lam, pairs):
    out = np.array(lam, dtype=float)
    for i0, i1, f in pairs:
        if f > 0:
            out[i0], out[i1] = lam[i0] + f * lam[i1], 0.0
        else:
            assert not (lam[i0] > 0 and lam[i1] > 0), "a band with both members active"
    return out


def other(lam, pairs):
    out = np.array(lam, dtype=float)
    for i0, i1, f in pairs:
        if f > 0:
            out[i0], out[i1] = 0.0, (lam[i0] + f * lam[i1]) / f
        else:
            out[i0], out[i1] = lam[i1], lam[i0]
    return out


def split(lam, pairs):
    out = np.array(lam, dtype=float)
    for i0, i1, f in pairs:
        assert f > 0
        t = lam[i0] + f * lam[i1]
        out[i0], out[i1] = t / 2, t / (2 * f)
    return out


def unique(g, pairs):
    """the unique part of a gradient over the rows, [m] or [m, ...] (flattened input is reshaped by the caller)"""
    out = np.array(g, dtype=g.dtype if hasattr(g, "dtype") else float)
    for i0, i1, f in pairs:
        out[i0] = g[i0] + f * g[i1]
        out[i1] = 0
    return out


def consistent(de, pairs):
    """a tangent of e [m] with both bounds of every pair moving together"""
    out = np.array(de, dtype=float)
    for i0, i1, f in pairs:
        out[i1] = f * out[i0]
    return out


# ---------------------------------------------------------------------------------------------- the whitened active rows
def condensed_of(w1):
    from oracle.condense_np import condense
    from qpmpc_amd.workloads import problem_from_workload

    p = problem_from_workload(w1, 0)
    return p, condense(p)


def gram(cq, lam):
    """(active row ids, S = M_A M_A' with M_A = G_A L^-T, P = L L')"""
    act = np.flatnonzero(np.asarray(lam) > 0.0)
    L = np.linalg.cholesky(cq.P)
    M = np.linalg.solve(L, cq.G[act].T).T
    return act, M @ M.T


def rank(S):
    """numerical rank of a Gram matrix: singular values above RANK_TOL times the largest"""
    if S.shape[0] == 0:
        return 0
    s = np.linalg.svd(S, compute_uv=False)
    return int((s > RANK_TOL * s[0]).sum())


def independent(cq, lam):
    act, S = gram(cq, lam)
    return len(act) <= cq.P.shape[0] and rank(S) == len(act)


# ---------------------------------------------------------------------------------------------- long-double references
def _kkt_ld(P, GA, r1, r2):
    """[P GA'; GA 0] [x; y] = [r1; r2] in long double: the float64 solve refined three times on long-double residuals"""
    n, k = P.shape[0], GA.shape[0]
    K = np.zeros((n + k, n + k))
    K[:n, :n], K[:n, n:], K[n:, :n] = P, GA.T, GA
    Kl, rhs = K.astype(LD), np.concatenate([np.asarray(r1, dtype=LD), np.asarray(r2, dtype=LD)])
    x = np.linalg.solve(K, rhs.astype(np.float64)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(K, (rhs - Kl @ x).astype(np.float64)).astype(LD)
    return x[:n], x[n:]


def _maps(w1):
    from oracle.capi import FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of

    p, cq = condensed_of(w1)
    f = flags_of(p)
    Phi = np.vstack([cq.Phi, cq.phi_last]).astype(LD)
    Psi = np.vstack([cq.Psi, cq.psi_last]).astype(LD)
    return p, cq, Phi, Psi, bool(f & FLAG_Q_TERMINAL), bool(f & FLAG_Q_STAGE), LD(p.terminal_cost_weight or 0.0), LD(p.stage_state_cost_weight or 0.0)


def vjp_ld(w1, lam, gU, gX=None):
    """adjoint_np.vjp in np.longdouble (the condensed operands are those of oracle/condense_np.py, float64)"""
    p, cq, Phi, Psi, qt, qs, wt, wx = _maps(w1)
    N, nx = int(w1["N"]), p.state_dim
    gX = np.zeros((N + 1) * nx, dtype=LD) if gX is None else np.asarray(gX, dtype=LD).ravel()
    g = np.asarray(gU, dtype=LD) + Psi.T @ gX
    act = np.flatnonzero(np.asarray(lam) > 0.0)
    a, bm = _kkt_ld(cq.P, cq.G[act], g, np.zeros(len(act)))  # (w, nu) of adjoint_np.vjp
    gh = np.zeros(cq.G.shape[0], dtype=LD)
    gh[act] = bm
    y = (Psi @ -a).reshape(N + 1, nx)
    v = gX.reshape(N + 1, nx).copy()
    if qs:
        v[:N] += wx * y[:N]
    if qt:
        v[N] += wt * y[N]
    mk = len(gh) // N
    for k, Ck in enumerate(cq.C_blocks):
        if Ck is not None:
            v[k] -= Ck.astype(LD).T @ gh[k * mk:(k + 1) * mk]
    return dict(x0=Phi.T @ v.ravel(), goal=(-wt * y[N]) if qt else np.zeros(nx, dtype=LD),
                targets=(-wx * y[:N]).ravel() if qs else np.zeros(N * nx, dtype=LD), e=gh)


def _rollout_ld(A, B, x0, U):
    X = [np.asarray(x0, dtype=LD)]
    for k in range(A.shape[0]):
        X.append(A[k] @ X[-1] + B[k] @ U[k])
    return np.stack(X)


def model_vjp_ld(w1, U, lam, gU, gX=None):
    """adjoint_model_np.model_vjp in np.longdouble: dL/dA, dL/dB, dL/dC, dL/dD and dL/dw (terminal, stage, input) of one problem
    (a workload of one with C and D) at its plan U and multipliers lam, from the long-double KKT solve of vjp_ld"""
    from oracle.capi import FLAG_P_STAGE, FLAG_P_TERMINAL, flags_of

    p, cq, Phi, Psi, qt, qs, wt, wx = _maps(w1)
    f = flags_of(p)
    pt, ps = bool(f & FLAG_P_TERMINAL), bool(f & FLAG_P_STAGE)
    N, nx = int(w1["N"]), p.state_dim
    A, B, C, D = (np.asarray(w1[k][0], dtype=LD) for k in ("A", "B", "C", "D"))
    nu, mk = B.shape[-1], C.shape[1]
    gXs = np.zeros((N + 1, nx), dtype=LD) if gX is None else np.asarray(gX, dtype=LD).reshape(N + 1, nx)
    act = np.flatnonzero(np.asarray(lam) > 0.0)
    w, bm = _kkt_ld(cq.P, cq.G[act], np.asarray(gU, dtype=LD) + Psi.T @ gXs.ravel(), np.zeros(len(act)))
    nuv = np.zeros(N * mk, dtype=LD)
    nuv[act] = bm
    u, wk = np.asarray(U, dtype=LD).reshape(N, nu), w.reshape(N, nu)
    x0 = np.asarray(w1["x0"][0], dtype=LD)
    X, Z, Y = _rollout_ld(A, B, x0, u), _rollout_ld(A, B, np.zeros(nx, dtype=LD), u), _rollout_ld(A, B, np.zeros(nx, dtype=LD), wk)
    lk, nk = np.asarray(lam, dtype=LD).reshape(N, mk), nuv.reshape(N, mk)
    E = np.zeros((N + 1, nx), dtype=LD)
    if ps:
        E[:N] = (X[:N] - np.asarray(w1["targets"][0], dtype=LD).reshape(N, nx)) if qs else Z[:N]
    if pt:
        E[N] = (X[N] - np.asarray(w1["goal"][0], dtype=LD)) if qt else Z[N]
    a, az, b = gXs.copy(), np.zeros((N + 1, nx), dtype=LD), np.zeros((N + 1, nx), dtype=LD)
    if ps:
        (a if qs else az)[:N] -= wx * Y[:N]
    if pt:
        (a if qt else az)[N] -= wt * Y[N]
    b[:N] -= wx * E[:N]
    b[N] -= wt * E[N]
    a[:N] -= np.einsum("kri,kr->ki", C, nk)
    b[:N] -= np.einsum("kri,kr->ki", C, lk)
    for k in range(N - 1, -1, -1):
        a[k] += A[k].T @ a[k + 1]
        az[k] += A[k].T @ az[k + 1]
        b[k] += A[k].T @ b[k + 1]
    out = dict(A=np.einsum("ki,kj->kij", a[1:], X[:N]) + np.einsum("ki,kj->kij", az[1:], Z[:N]) + np.einsum("ki,kj->kij", b[1:], Y[:N]),
               B=np.einsum("ki,kj->kij", a[1:] + az[1:], u) + np.einsum("ki,kj->kij", b[1:], wk),
               C=-(np.einsum("kr,ki->kri", lk, Y[:N]) + np.einsum("kr,ki->kri", nk, X[:N])),
               D=-(np.einsum("kr,ki->kri", lk, wk) + np.einsum("kr,ki->kri", nk, u)))
    out["w"] = np.array([-(Y[N] @ E[N]) if pt else LD(0), -np.sum(Y[:N] * E[:N]) if ps else LD(0), -(w @ u.ravel())], dtype=LD)
    return out


def jvp_ld(w1, lam, tan):
    """tangent_np.jvp in np.longdouble"""
    p, cq, Phi, Psi, qt, qs, wt, wx = _maps(w1)
    N, nx, n, m = int(w1["N"]), p.state_dim, cq.P.shape[0], cq.G.shape[0]
    t = dict(x0=np.zeros(nx), goal=np.zeros(nx), targets=np.zeros(N * nx), e=np.zeros(m))
    t.update({k: np.asarray(v, dtype=float).ravel() for k, v in tan.items() if v is not None})
    t = {k: v.astype(LD) for k, v in t.items()}
    dq = np.zeros(n, dtype=LD)
    if qt:
        dq += wt * Psi[N * nx:].T @ (Phi[N * nx:] @ t["x0"] - t["goal"])
    if qs:
        dq += wx * Psi[:N * nx].T @ (Phi[:N * nx] @ t["x0"] - t["targets"])
    dh = t["e"].copy()
    mk = m // N
    for k, Ck in enumerate(cq.C_blocks):
        if Ck is not None:
            dh[k * mk:(k + 1) * mk] -= Ck.astype(LD) @ (Phi[k * nx:(k + 1) * nx] @ t["x0"])
    act = np.flatnonzero(np.asarray(lam) > 0.0)
    dU, _ = _kkt_ld(cq.P, cq.G[act], -dq, dh[act])
    return dict(U=dU, X=Phi @ t["x0"] + Psi @ dU)


# ---------------------------------------------------------------------------------------------- seeded cotangents and tangents
def cotangents(shape, seed=31):
    """(gU [B, n], gX [B, (N + 1) nx]) of a case"""
    nx, nu, N, mk = shape
    rng = np.random.default_rng(seed + N)
    return rng.standard_normal((OL.BATCH, N * nu)), rng.standard_normal((OL.BATCH, (N + 1) * nx))


def tangents(shape, pairs, T=2, seed=37):
    """{x0 [B, T, nx], goal, targets [B, T, N nx], e [B, T, N mk]}: T seeded tangents per problem, those of e moving the two bounds
    of every pair together"""
    nx, nu, N, mk = shape
    rng = np.random.default_rng(seed + N)
    B = OL.BATCH
    tan = dict(x0=rng.standard_normal((B, T, nx)), goal=rng.standard_normal((B, T, nx)), targets=rng.standard_normal((B, T, N * nx)),
               e=rng.standard_normal((B, T, N * mk)))
    for b in range(B):
        for t in range(T):
            tan["e"][b, t] = consistent(tan["e"][b, t], pairs)
    return tan


def model_tangents(shape, T=2, seed=41):
    """tangents of B [B, T, N, nx, nu] and of the three weights [B, T] (terminal, stage, input): what sends a tangent solve to the
    `_model` exports. Neither touches a constraint row, so the response stays unique on a binding pair."""
    nx, nu, N, mk = shape
    rng = np.random.default_rng(seed + N)
    return dict(B=rng.standard_normal((OL.BATCH, T, N, nx, nu)), w=rng.standard_normal((OL.BATCH, T, 3)))
