"""NumPy float64 restatement of the Jacobian-vector product of a solved plan (test helper, not an oracle module).

For one problem of a workload dict (qpmpc_amd.workloads layout), condensed by ``oracle.condense_np.condense``, the plan
U solves P U + q + G_A' lam_A = 0, G_A U = h_A on the active set A = {i : lam_i > 0}. Its tangent is the same KKT
system, solved densely:

    [P  G_A'] [dU    ]   [-dq ]
    [G_A  0 ] [dlam_A] = [dh_A],    dq = w_t psi_N'(phi_N dx0 - dgoal) + w_x Psi'(Phi dx0 - dtargets),
                                    dh = de - C Phi dx0,   dX = Phi dx0 + Psi dU

(each q term only where dims flags it, as ``adjoint_np.vjp`` has it). ``fd_jvp`` differentiates the C oracle's solve by
central differences along the same tangent.
"""
from __future__ import annotations

import numpy as np

from oracle.capi import FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
from oracle.condense_np import condense, integrate
from qpmpc_amd.workloads import problem_from_workload

import adjoint_np as AN

KEYS = ("x0", "goal", "targets", "e")


def _zeros_like_keys(w1: dict) -> dict:
    N, nx = int(w1["N"]), np.asarray(w1["x0"]).shape[-1]
    m = 0 if w1["e"] is None else np.asarray(w1["e"])[0].size
    return dict(x0=np.zeros(nx), goal=np.zeros(nx), targets=np.zeros(N * nx), e=np.zeros(m))


def jvp(w1: dict, lam, tan: dict) -> dict:
    """dU [n] and dX [(N+1)*nx] of one problem (workload of one) at multipliers ``lam`` along ``tan`` (a dict over
    ``KEYS``; a missing key is a zero tangent)."""
    t = _zeros_like_keys(w1)
    t.update({k: np.asarray(v, dtype=float).ravel() for k, v in tan.items() if v is not None})
    p = problem_from_workload(w1, 0)
    cq = condense(p)
    N, nx, n = int(w1["N"]), p.state_dim, cq.P.shape[0]
    Phi = np.vstack([cq.Phi, cq.phi_last])
    Psi = np.vstack([cq.Psi, cq.psi_last])
    f = flags_of(p)
    wt = p.terminal_cost_weight or 0.0
    wx = p.stage_state_cost_weight or 0.0
    dq = np.zeros(n)
    if f & FLAG_Q_TERMINAL:
        dq += wt * cq.psi_last.T @ (cq.phi_last @ t["x0"] - t["goal"])
    if f & FLAG_Q_STAGE:
        dq += wx * cq.Psi.T @ (cq.Phi @ t["x0"] - t["targets"])
    m = cq.G.shape[0]
    dh = t["e"].copy() if m else np.zeros(0)
    mk = m // N if m else 0
    for k, Ck in enumerate(cq.C_blocks):
        if Ck is not None:
            dh[k * mk:(k + 1) * mk] -= Ck @ (Phi[k * nx:(k + 1) * nx] @ t["x0"])
    act = np.flatnonzero(np.asarray(lam) > 0.0)
    GA = cq.G[act]
    k = len(act)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = cq.P
    K[:n, n:] = GA.T
    K[n:, :n] = GA
    sol = np.linalg.solve(K, np.concatenate([-dq, dh[act]]))
    dU = sol[:n]
    return dict(U=dU, X=Phi @ t["x0"] + Psi @ dU, lam=sol[n:], active=act)


def fd_jvp(w1: dict, tan: dict, step: float = 1e-6) -> dict:
    """Central differences of the C oracle's U and its rollout X along ``tan`` (a workload of one)."""
    outs = []
    for s in (step, -step):
        w2 = dict(w1)
        for key, d in tan.items():
            if d is None:
                continue
            base = np.asarray(w1[key], dtype=float)
            w2[key] = base + s * np.asarray(d, dtype=float).reshape(base.shape)
        U, _, _, st = AN.solve(w2)
        assert st == 0
        X = integrate(problem_from_workload(w2, 0), np.asarray(w2["x0"][0]), U)
        outs.append((U, np.asarray(X).ravel()))
    return dict(U=(outs[0][0] - outs[1][0]) / (2 * step), X=(outs[0][1] - outs[1][1]) / (2 * step))


def random_tangent(w1: dict, rng) -> dict:
    """One random tangent of every operand the problem has."""
    t = _zeros_like_keys(w1)
    out = {k: rng.standard_normal(v.size) for k, v in t.items() if v.size}
    for key in ("goal", "targets"):
        if w1[key] is None:
            out.pop(key, None)
    return out
