"""NumPy float64 restatement of the stage-wise adjoint (test helper, not an oracle module).

The same KKT adjoint as tests/adjoint_np.py and tests/adjoint_model_np.py,

    [P  G_A'] [a]   [gU + Psi' gX]
    [G_A  0 ] [b] = [     0      ],     A = {i : lam_i > 0},

solved without condensing: P = L L' is the whitened Riccati recursion of ``oracle.stagewise_qr_np.WhitenedRiccati``.
One backward sweep gives t = L^-1 (gU + Psi' gX); one backward sweep per active row, started at its step, gives its
whitened vector y_a = L^-1 g_a'; then S = Y_A Y_A' = R R', b = S^-1 Y_A t, and one forward sweep from x0 = 0 gives
a = L^-T (t - Y_A' b) with its states Y = Psi a. Everything after that is a costate recursion over A_k (DESIGN.md section 9,
"Stage-wise adjoint"). This is what qpmpc_amd/csrc/mpcqp_adjoint_stagewise.hip computes, step for step.
"""
from __future__ import annotations

import numpy as np

from oracle.capi import FLAG_P_STAGE, FLAG_P_TERMINAL, FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
from oracle.stagewise_np import from_mpc_problem
from oracle.stagewise_qr_np import WhitenedRiccati
from qpmpc_amd.workloads import problem_from_workload

NOT_PD = 3


def _rollout(A, B, x0, U):
    N = A.shape[0]
    X = np.zeros((N + 1, A.shape[1]))
    X[0] = x0
    for k in range(N):
        X[k + 1] = A[k] @ X[k] + B[k] @ U[k]
    return X


def _steps(w1: dict, key: str, shape):
    N = int(w1["N"])
    a = w1[key]
    if a is None:
        return np.zeros((N,) + tuple(shape))
    a = np.asarray(a, dtype=float)
    if -1 not in shape and a.size == int(np.prod(shape)):  # one block for every step
        return np.broadcast_to(a.reshape(shape), (N,) + tuple(shape))
    return a.reshape(N, *shape)


def stagewise_vjp(w1: dict, lam, gU, gX=None, U=None) -> dict:
    """Gradients of one problem (workload of one, ``adjoint_np.single``) at multipliers ``lam``: x0 [nx], goal [nx],
    targets [N*nx], e [N*mk]; with the plan ``U`` also A [N,nx,nx], B [N,nx,nu], C [N,mk,nx], D [N,mk,nu] (absent C or D:
    at zero) and w [3]. ``status`` is 0, or NOT_PD (every gradient zero) when a stage Hessian or the active rows' Gram
    matrix is not positive definite or more rows are active than there are variables."""
    p = problem_from_workload(w1, 0)
    sp = from_mpc_problem(p)
    N, nx, nu = sp.N, sp.nx, sp.nu
    n = N * nu
    lam = np.asarray(lam, dtype=float)
    mk = len(lam) // N if N else 0
    f = flags_of(p)
    pt, ps = bool(f & FLAG_P_TERMINAL), bool(f & FLAG_P_STAGE)
    qt, qs = bool(f & FLAG_Q_TERMINAL), bool(f & FLAG_Q_STAGE)
    wt = p.terminal_cost_weight or 0.0
    wx = p.stage_state_cost_weight or 0.0
    A, B = _steps(w1, "A", (nx, nx)), _steps(w1, "B", (nx, nu))
    C, D = _steps(w1, "C", (mk, nx)), _steps(w1, "D", (mk, nu))

    def zeros(status):
        out = dict(x0=np.zeros(nx), goal=np.zeros(nx), targets=np.zeros(N * nx), e=np.zeros(N * mk), status=status)
        if U is not None:
            out.update(A=np.zeros_like(A), B=np.zeros_like(B), C=np.zeros_like(C), D=np.zeros_like(D), w=np.zeros(3))
        return out

    ric = WhitenedRiccati(sp)
    if not ric.pd:
        return zeros(NOT_PD)
    gXs = np.zeros((N + 1, nx)) if gX is None else np.asarray(gX, dtype=float).reshape(N + 1, nx)
    # 2. t = L^-1 (gU + Psi' gX): WhitenedRiccati.backward(q, r, pN) is -L^-1 (Psi' q + r + Psi_N' pN)
    t = ric.backward(-gXs[:N], -np.asarray(gU, dtype=float).reshape(N, nu), pN=-gXs[N]).reshape(n)
    # 3. the active rows' whitened vectors, one backward sweep each from the row's step (oracle's row_y)
    act = np.flatnonzero(lam > 0.0)
    k = len(act)
    if k > n:
        return zeros(NOT_PD)
    Y = np.zeros((k, n))
    for a, i in enumerate(act):
        j, r = divmod(int(i), mk)
        ql, rl = np.zeros((N, nx)), np.zeros((N, nu))
        ql[j], rl[j] = -C[j, r], -D[j, r]
        Y[a] = ric.backward(ql, rl, ktop=j).reshape(n)
    # 4. multipliers: S = Y_A Y_A' = R R', b = S^-1 Y_A t
    if k:
        try:
            R = np.linalg.cholesky(Y @ Y.T)
        except np.linalg.LinAlgError:
            return zeros(NOT_PD)
        b = np.linalg.solve(R.T, np.linalg.solve(R, Y @ t))
    else:
        b = np.zeros(0)
    # 5. a = L^-T (t - Y_A' b) with its states: one forward sweep from x0 = 0
    wu_, Ys = ric.forward((t - Y.T @ b).reshape(N, nu))
    w = wu_.reshape(n)
    y = -Ys  # DESIGN section 9's y = Psi dL/dq
    gh = np.zeros(N * mk)
    gh[act] = b
    v = gXs.copy()
    if qs:
        v[:N] += wx * y[:N]
    if qt:
        v[N] += wt * y[N]
    v[:N] -= np.einsum("kri,kr->ki", C, gh.reshape(N, mk))
    pc = v.copy()
    for kk in range(N - 1, -1, -1):
        pc[kk] += A[kk].T @ pc[kk + 1]
    out = dict(x0=pc[0].copy(), goal=(-wt * y[N]) if qt else np.zeros(nx),
               targets=(-wx * y[:N]).ravel() if qs else np.zeros(N * nx), e=gh, status=0)
    if U is None:
        return out
    # 6. model and cost gradients: rollouts instead of Phi and Psi, then the costates of adjoint_model_np
    u = np.asarray(U, dtype=float).reshape(N, nu)
    x0 = np.asarray(w1["x0"][0], dtype=float)
    X = _rollout(A, B, x0, u)
    Z = _rollout(A, B, np.zeros(nx), u)
    wk = w.reshape(N, nu)
    lk, nk = lam.reshape(N, mk), gh.reshape(N, mk)
    E = np.zeros((N + 1, nx))
    if ps:
        E[:N] = (X[:N] - np.asarray(w1["targets"][0], dtype=float).reshape(N, nx)) if qs else Z[:N]
    if pt:
        E[N] = (X[N] - np.asarray(w1["goal"][0], dtype=float)) if qt else Z[N]
    az, bb = np.zeros((N + 1, nx)), np.zeros((N + 1, nx))
    if ps and not qs:
        az[:N] -= wx * Ys[:N]
    if pt and not qt:
        az[N] -= wt * Ys[N]
    bb[:N] -= wx * E[:N]
    bb[N] -= wt * E[N]
    bb[:N] -= np.einsum("kri,kr->ki", C, lk)
    pz, s = az, bb
    for kk in range(N - 1, -1, -1):
        pz[kk] += A[kk].T @ pz[kk + 1]
        s[kk] += A[kk].T @ s[kk + 1]
    out["A"] = (np.einsum("ki,kj->kij", pc[1:], X[:N]) + np.einsum("ki,kj->kij", pz[1:], Z[:N])
                + np.einsum("ki,kj->kij", s[1:], Ys[:N]))
    out["B"] = np.einsum("ki,kj->kij", pc[1:] + pz[1:], u) + np.einsum("ki,kj->kij", s[1:], wk)
    out["C"] = -(np.einsum("kr,ki->kri", lk, Ys[:N]) + np.einsum("kr,ki->kri", nk, X[:N]))
    out["D"] = -(np.einsum("kr,ki->kri", lk, wk) + np.einsum("kr,ki->kri", nk, u))
    out["w"] = np.array([-(Ys[N] @ E[N]) if pt else 0.0, -np.sum(Ys[:N] * E[:N]) if ps else 0.0, -(w @ u.ravel())])
    return out
