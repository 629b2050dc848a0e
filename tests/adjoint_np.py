"""NumPy float64 restatement of the vector-Jacobian product of a solved plan (test helper, not an oracle module).

For one problem of a workload dict (qpmpc_amd.workloads layout), condensed by ``oracle.condense_np.condense``, the KKT
adjoint is solved densely on the active set {i : lam_i > 0}:

    [P  G_A'] [a]   [gU + Psi' gX]
    [G_A  0 ] [b] = [     0      ],     dL/dq = -a,  dL/dh_A = b,  dL/dh_i = 0 off A,

and mapped back through q = w_t psi_N'(phi_N x0 - goal) + w_x Psi'(Phi x0 - targets), h = e - C Phi x0 and
X = Phi x0 + Psi U. ``fd_gradients`` differentiates L = gU.U + gX.X by central differences of the C oracle's solve.
"""
from __future__ import annotations

import numpy as np

from oracle.capi import FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of, gi_solve
from oracle.condense_np import condense, integrate
from qpmpc_amd.workloads import problem_from_workload


def single(w: dict, b: int) -> dict:
    """Problem ``b`` of a workload as a workload of one, every operand stored per step (so it can be perturbed)."""
    N = int(w["N"])
    out = dict(w)
    for key, block in (("A", 2), ("B", 2), ("C", 2), ("D", 2), ("e", 1)):
        a = w[key]
        if a is None:
            continue
        a = np.asarray(a, dtype=float)
        if a.ndim == block + 2:
            a = a[b] if a.shape[0] > 1 else a[0]
        if a.ndim == block:
            a = np.broadcast_to(a, (N,) + a.shape)
        out[key] = np.ascontiguousarray(a)[None]
    for key in ("x0", "goal", "targets"):
        a = w[key]
        if a is not None:
            a = np.asarray(a, dtype=float)
            out[key] = (a[b] if a.ndim == 2 else a).copy()[None]
    return out


def solve(w1: dict):
    """(U [n], lam [m], slack [m], status) of a workload of one, by the C oracle on the NumPy condensing."""
    p = problem_from_workload(w1, 0)
    cq = condense(p)
    x, lam, st, _ = gi_solve(cq.P, cq.q, cq.G, cq.h)
    return x, lam, cq.h - cq.G @ x, st


def loss(w1: dict, gU, gX) -> float:
    p = problem_from_workload(w1, 0)
    U, _, _, st = solve(w1)
    assert st == 0
    val = float(gU @ U)
    if gX is not None:
        val += float(gX.ravel() @ integrate(p, np.asarray(w1["x0"][0]), U).ravel())
    return val


def vjp(w1: dict, lam, gU, gX=None) -> dict:
    """dL/dx0, dL/dgoal, dL/dtargets [N*nx], dL/de [N*mk] of one problem (workload of one) at multipliers ``lam``."""
    p = problem_from_workload(w1, 0)
    cq = condense(p)
    N, nx = int(w1["N"]), p.state_dim
    Phi = np.vstack([cq.Phi, cq.phi_last])
    Psi = np.vstack([cq.Psi, cq.psi_last])
    gX = np.zeros((N + 1) * nx) if gX is None else np.asarray(gX, dtype=float).ravel()
    g = np.asarray(gU, dtype=float) + Psi.T @ gX
    act = np.flatnonzero(np.asarray(lam) > 0.0)
    Lc = np.linalg.cholesky(cq.P)
    t = np.linalg.solve(Lc, g)
    M = np.linalg.solve(Lc, cq.G[act].T).T  # G_A L^-T
    nu = np.linalg.solve(M @ M.T, M @ t) if len(act) else np.zeros(0)
    w = np.linalg.solve(Lc.T, t - M.T @ nu)
    gh = np.zeros(cq.G.shape[0])
    gh[act] = nu
    y = (Psi @ -w).reshape(N + 1, nx)
    f = flags_of(p)
    qt, qs = bool(f & FLAG_Q_TERMINAL), bool(f & FLAG_Q_STAGE)
    wt = p.terminal_cost_weight or 0.0
    wx = p.stage_state_cost_weight or 0.0
    v = gX.reshape(N + 1, nx).copy()
    if qs:
        v[:N] += wx * y[:N]
    if qt:
        v[N] += wt * y[N]
    mk = len(gh) // N
    for k, Ck in enumerate(cq.C_blocks):
        if Ck is not None:
            v[k] -= Ck.T @ gh[k * mk:(k + 1) * mk]
    return dict(x0=Phi.T @ v.ravel(), goal=(-wt * y[N]) if qt else np.zeros(nx),
                targets=(-wx * y[:N]).ravel() if qs else np.zeros(N * nx), e=gh)


def fd_gradients(w1: dict, gU, gX=None, step: float = 1e-6) -> dict:
    """Central differences of L = gU.U + gX.X with respect to x0, goal, targets and e of a workload of one."""
    out = {}
    for key in ("x0", "goal", "targets", "e"):
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
                vals.append(loss(w2, gU, gX))
            g[i] = (vals[0] - vals[1]) / (2 * step)
        out[key] = g
    return out


def strictly_complementary(lam, slack, margin: float = 1e-4) -> bool:
    return bool(np.all((np.asarray(lam) > margin) | (np.asarray(slack) > margin)))


def complementary(w, count):
    """Indices of the first ``count`` strictly complementary problems of a workload (by the C oracle)."""
    picked = []
    for b in range(np.asarray(w["x0"]).shape[0]):
        U, lam, slack, st = solve(single(w, b))
        if st == 0 and strictly_complementary(lam, slack):
            picked.append(b)
        if len(picked) == count:
            return picked
    raise AssertionError(f"only {len(picked)} strictly complementary problems")
