"""NumPy float64 restatement of the model and cost gradients of a solved plan (test helper, not an oracle module).

Built on tests/adjoint_np.py. With the KKT adjoint (w, nu) of ``adjoint`` and the plan U, lam held fixed, every parameter
theta enters through

    Lambda = -[ w_u w'U + w_t Y_N'E_N + w_x sum_{k<N} Y_k'E_k
                + sum_k lam_k'(C_k Y_k + D_k w_k) + sum_k nu_k'(C_k X_k + D_k u_k - e_k) ] + gX'X,

X = rollout(x0, U), Y = rollout(0, w), Z = rollout(0, U) (the forced response Psi U). E_N = X_N - goal when the terminal
q term is flagged (MPCQP_Q_TERMINAL), else Z_N; E_k = X_k - r_k when MPCQP_Q_STAGE, else Z_k; a P term that is not flagged
drops out. dL/dtheta = dLambda/dtheta: the weights and C, D directly, A and B by backward costate recursions over the
trajectories X (p), Z (pz) and Y (s):

    p_N = a_N,  p_k = a_k + A_k' p_{k+1}     (pz from az, s from b, the same way)
    g_A_k = p_{k+1} X_k' + pz_{k+1} Z_k' + s_{k+1} Y_k',   g_B_k = (p + pz)_{k+1} u_k' + s_{k+1} w_k'

and p_0 is dL/dx0. ``fd_model_gradients`` differentiates L = gU.U + gX.X by central differences of the C oracle.
"""
from __future__ import annotations

import numpy as np

import adjoint_np as AN
from oracle.capi import FLAG_P_STAGE, FLAG_P_TERMINAL, FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
from oracle.condense_np import condense, integrate
from qpmpc_amd.workloads import problem_from_workload

WEIGHTS = ("wt", "wx", "wu")  # terminal, stage, input: the order of g_w


def adjoint(w1: dict, lam, gU, gX=None):
    """(w [n], nu [m]) of [P G_A'; G_A 0][w; nu] = [gU + Psi' gX; 0] on A = {i : lam_i > 0}; nu is zero off A."""
    p = problem_from_workload(w1, 0)
    cq = condense(p)
    N, nx = int(w1["N"]), p.state_dim
    Psi = np.vstack([cq.Psi, cq.psi_last])
    gX = np.zeros((N + 1) * nx) if gX is None else np.asarray(gX, dtype=float).ravel()
    g = np.asarray(gU, dtype=float) + Psi.T @ gX
    act = np.flatnonzero(np.asarray(lam) > 0.0)
    n, k = len(g), len(act)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = cq.P
    K[n:, :n] = cq.G[act]
    K[:n, n:] = cq.G[act].T
    sol = np.linalg.solve(K, np.concatenate([g, np.zeros(k)]))
    nu = np.zeros(cq.G.shape[0])
    nu[act] = sol[n:]
    return sol[:n], nu


def _steps(w1: dict, key: str, shape):
    """Per-step blocks [N, *shape] of operand ``key`` of a workload of one (zeros when absent)."""
    N = int(w1["N"])
    a = w1[key]
    if a is None:
        return np.zeros((N,) + tuple(shape))
    return np.asarray(a, dtype=float).reshape(N, *shape)


def model_vjp(w1: dict, U, lam, gU, gX=None) -> dict:
    """dL/dA [N,nx,nx], dL/dB [N,nx,nu], dL/dC [N,mk,nx], dL/dD [N,mk,nu] (for absent C or D: at zero) and
    dL/dw [3] (terminal, stage, input) of one problem at its plan ``U`` and multipliers ``lam``, plus dL/dx0 from p_0."""
    p = problem_from_workload(w1, 0)
    N, nx, nu = int(w1["N"]), p.state_dim, p.input_dim
    mk = len(lam) // N
    f = flags_of(p)
    pt, ps = bool(f & FLAG_P_TERMINAL), bool(f & FLAG_P_STAGE)
    qt, qs = bool(f & FLAG_Q_TERMINAL), bool(f & FLAG_Q_STAGE)
    wt = p.terminal_cost_weight or 0.0
    wx = p.stage_state_cost_weight or 0.0
    w, nuv = adjoint(w1, lam, gU, gX)
    A, B = _steps(w1, "A", (nx, nx)), _steps(w1, "B", (nx, nu))
    C, D = _steps(w1, "C", (mk, nx)), _steps(w1, "D", (mk, nu))
    x0 = np.asarray(w1["x0"][0], dtype=float)
    X = integrate(p, x0, U)
    Z = integrate(p, np.zeros(nx), U)
    Y = integrate(p, np.zeros(nx), w)
    u, wk = np.asarray(U).reshape(N, nu), w.reshape(N, nu)
    lk, nk = np.asarray(lam, dtype=float).reshape(N, mk), nuv.reshape(N, mk)
    gXs = np.zeros((N + 1, nx)) if gX is None else np.asarray(gX, dtype=float).reshape(N + 1, nx)
    E = np.zeros((N + 1, nx))  # the error trajectory of the weighted terms (zero where no P term)
    if ps:
        E[:N] = (X[:N] - np.asarray(w1["targets"][0], dtype=float).reshape(N, nx)) if qs else Z[:N]
    if pt:
        E[N] = (X[N] - np.asarray(w1["goal"][0], dtype=float)) if qt else Z[N]
    a, az, b = gXs.copy(), np.zeros((N + 1, nx)), np.zeros((N + 1, nx))
    (a if qs else az)[:N] -= wx * Y[:N] if ps else 0.0
    (a if qt else az)[N] -= wt * Y[N] if pt else 0.0
    b[:N] -= wx * E[:N]
    b[N] -= wt * E[N]
    a[:N] -= np.einsum("kri,kr->ki", C, nk)
    b[:N] -= np.einsum("kri,kr->ki", C, lk)
    pc, pz, s = a.copy(), az.copy(), b.copy()
    for k in range(N - 1, -1, -1):
        pc[k] += A[k].T @ pc[k + 1]
        pz[k] += A[k].T @ pz[k + 1]
        s[k] += A[k].T @ s[k + 1]
    gA = (np.einsum("ki,kj->kij", pc[1:], X[:N]) + np.einsum("ki,kj->kij", pz[1:], Z[:N])
          + np.einsum("ki,kj->kij", s[1:], Y[:N]))
    gB = np.einsum("ki,kj->kij", pc[1:] + pz[1:], u) + np.einsum("ki,kj->kij", s[1:], wk)
    gC = -(np.einsum("kr,ki->kri", lk, Y[:N]) + np.einsum("kr,ki->kri", nk, X[:N]))
    gD = -(np.einsum("kr,ki->kri", lk, wk) + np.einsum("kr,ki->kri", nk, u))
    gw = np.array([-(Y[N] @ E[N]) if pt else 0.0, -np.sum(Y[:N] * E[:N]) if ps else 0.0, -(w @ np.asarray(U))])
    return dict(A=gA, B=gB, C=gC, D=gD, w=gw, x0=pc[0])


def fd_model_gradients(w1: dict, gU, gX=None, step: float = 1e-6) -> dict:
    """Central differences of L = gU.U + gX.X with respect to every entry of A, B, C, D (those present) and the three
    weights (those set) of a workload of one."""
    out = {}
    for key in ("A", "B", "C", "D"):
        if w1[key] is None:
            continue
        base = np.asarray(w1[key], dtype=float)
        g = np.zeros(base.size)
        for i in range(base.size):
            vals = []
            for s in (step, -step):
                pert = base.copy().ravel()
                pert[i] += s
                w2 = dict(w1)
                w2[key] = pert.reshape(base.shape)
                vals.append(AN.loss(w2, gU, gX))
            g[i] = (vals[0] - vals[1]) / (2 * step)
        out[key] = g.reshape(base.shape[1:])
    gw = np.full(3, np.nan)
    for i, key in enumerate(WEIGHTS):
        if w1[key] is None:
            continue
        h = min(step, 1e-3 * abs(float(w1[key])))  # (w_u = 1e-6 must stay positive)
        vals = []
        for s in (h, -h):
            w2 = dict(w1)
            w2[key] = float(w1[key]) + s
            vals.append(AN.loss(w2, gU, gX))
        gw[i] = (vals[0] - vals[1]) / (2 * h)
    out["w"] = gw
    return out
