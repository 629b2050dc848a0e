"""NumPy float64 restatement of the Jacobian-vector product of a solved plan along tangents of the model matrices A, B,
C, D and the three cost weights as well as x0, goal, targets and e (test helper, not an oracle module).

Built on tests/tangent_np.py and tests/adjoint_model_np.py. At the plan (U, lam) on A = {i : lam_i > 0}, with
X = rollout(x0, U), Z = rollout(0, U) and E the error trajectory of ``adjoint_model_np.model_vjp`` (X_k - r_k where the q
term is flagged, Z_k where only the P term is, 0 where neither), the costate of the stationarity condition is

    s_k = w_x E_k + C_k' lam_k (k < N),  s_N = w_t E_N,   pi_N = s_N,  pi_k = s_k + A_k' pi_{k+1},

so that 0 = w_u u_k + B_k' pi_{k+1} + D_k' lam_k. Per tangent, with U and lam held fixed:

    xs_0 = dx0,  xs_{k+1} = A_k xs_k + dA_k X_k + dB_k u_k       (zs the same from 0 with Z_k)
    dE_k = xs_k - dtargets_k (Q_STAGE) | zs_k (P_STAGE only) | 0;  dE_N likewise with dgoal
    c_k  = [P_STAGE] dw_x E_k + w_x dE_k + dC_k' lam_k + dA_k' pi_{k+1}  (k < N),   c_N = [P_TERMINAL] dw_t E_N + w_t dE_N
    g_k  = dw_u u_k + dB_k' pi_{k+1} + dD_k' lam_k
    dq   = Psi' c + g,   dh_k = de_k - C_k xs_k - dC_k X_k - dD_k u_k
    [P G_A'; G_A 0][dU; dlam_A] = [-dq; dh_A],   dX = xs + Psi dU

A tangent of an absent C or D is the tangent at zero. ``fd_jvp_model`` differentiates the C oracle's solve by central
differences along the same joint tangent.
"""
from __future__ import annotations

import numpy as np

import adjoint_np as AN
import tangent_np as TN
from adjoint_model_np import _steps
from oracle.capi import FLAG_P_STAGE, FLAG_P_TERMINAL, FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
from oracle.condense_np import condense, integrate
from qpmpc_amd.workloads import problem_from_workload

MODEL_KEYS = ("A", "B", "C", "D", "w")  # w: (dw_t, dw_x, dw_u), the order of g_w
WEIGHTS = ("wt", "wx", "wu")


class Shared:
    """What every tangent of one problem shares: the trajectories X, Z, the error E, the costate pi and the flags."""

    def __init__(self, w1: dict, U, lam):
        self.p = p = problem_from_workload(w1, 0)
        self.N, self.nx, self.nu = N, nx, nu = int(w1["N"]), p.state_dim, p.input_dim
        lam = np.asarray(lam, dtype=float)
        self.mk = mk = len(lam) // N
        f = flags_of(p)
        self.pt, self.ps = bool(f & FLAG_P_TERMINAL), bool(f & FLAG_P_STAGE)
        self.qt, self.qs = bool(f & FLAG_Q_TERMINAL), bool(f & FLAG_Q_STAGE)
        self.wt = p.terminal_cost_weight or 0.0
        self.wx = p.stage_state_cost_weight or 0.0
        self.A, self.B = _steps(w1, "A", (nx, nx)), _steps(w1, "B", (nx, nu))
        self.C, self.D = _steps(w1, "C", (mk, nx)), _steps(w1, "D", (mk, nu))
        self.u = np.asarray(U, dtype=float).reshape(N, nu)
        self.lk = lam.reshape(N, mk)
        self.act = np.flatnonzero(lam > 0.0)
        self.X = integrate(p, np.asarray(w1["x0"][0], dtype=float), U)
        self.Z = integrate(p, np.zeros(nx), U)
        E = np.zeros((N + 1, nx))
        if self.ps:
            E[:N] = (self.X[:N] - np.asarray(w1["targets"][0], dtype=float).reshape(N, nx)) if self.qs else self.Z[:N]
        if self.pt:
            E[N] = (self.X[N] - np.asarray(w1["goal"][0], dtype=float)) if self.qt else self.Z[N]
        self.E = E
        s = np.zeros((N + 1, nx))
        s[:N] = self.wx * E[:N] + np.einsum("kri,kr->ki", self.C, self.lk)
        s[N] = self.wt * E[N]
        pi = s.copy()
        for k in range(N - 1, -1, -1):
            pi[k] += self.A[k].T @ pi[k + 1]
        self.pi = pi

    def tangent(self, tan: dict):
        """Every operand's tangent as an array (zeros where ``tan`` has none)."""
        N, nx, nu, mk = self.N, self.nx, self.nu, self.mk
        shapes = dict(x0=(nx,), goal=(nx,), targets=(N, nx), e=(N, mk), A=(N, nx, nx), B=(N, nx, nu), C=(N, mk, nx),
                      D=(N, mk, nu), w=(3,))
        out = {}
        for key, shp in shapes.items():
            v = tan.get(key)
            out[key] = np.zeros(shp) if v is None else np.asarray(v, dtype=float).reshape(shp)
        return out

    def rhs(self, tan: dict):
        """(xs [N+1, nx], c [N+1, nx], g [N, nu], dh [N, mk]) of one tangent."""
        N, nx = self.N, self.nx
        t = self.tangent(tan)
        xs, zs = np.zeros((N + 1, nx)), np.zeros((N + 1, nx))
        xs[0] = t["x0"]
        for k in range(N):
            xs[k + 1] = self.A[k] @ xs[k] + t["A"][k] @ self.X[k] + t["B"][k] @ self.u[k]
            zs[k + 1] = self.A[k] @ zs[k] + t["A"][k] @ self.Z[k] + t["B"][k] @ self.u[k]
        dE = np.zeros((N + 1, nx))
        if self.qs:
            dE[:N] = xs[:N] - t["targets"]
        elif self.ps:
            dE[:N] = zs[:N]
        if self.qt:
            dE[N] = xs[N] - t["goal"]
        elif self.pt:
            dE[N] = zs[N]
        dwt, dwx, dwu = t["w"]
        c = np.zeros((N + 1, nx))
        c[:N] = ((dwx * self.E[:N] if self.ps else 0.0) + self.wx * dE[:N] + np.einsum("kri,kr->ki", t["C"], self.lk)
                 + np.einsum("kji,kj->ki", t["A"], self.pi[1:]))
        c[N] = (dwt * self.E[N] if self.pt else 0.0) + self.wt * dE[N]
        g = dwu * self.u + np.einsum("kij,ki->kj", t["B"], self.pi[1:]) + np.einsum("krj,kr->kj", t["D"], self.lk)
        dh = (t["e"] - np.einsum("kri,ki->kr", self.C, xs[:N]) - np.einsum("kri,ki->kr", t["C"], self.X[:N])
              - np.einsum("krj,kj->kr", t["D"], self.u))
        return xs, c, g, dh


def jvp_model(w1: dict, U, lam, tan: dict) -> dict:
    """dU [n] and dX [(N+1)*nx] of one problem (workload of one) at its plan ``U`` and multipliers ``lam`` along ``tan``
    (a dict over tangent_np's KEYS and MODEL_KEYS; a missing key is a zero tangent)."""
    sh = Shared(w1, U, lam)
    cq = condense(sh.p)
    Psi = np.vstack([cq.Psi, cq.psi_last])
    xs, c, g, dh = sh.rhs(tan)
    dq = Psi.T @ c.ravel() + g.ravel()
    act, n = sh.act, cq.P.shape[0]
    k = len(act)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = cq.P
    K[:n, n:] = cq.G[act].T
    K[n:, :n] = cq.G[act]
    sol = np.linalg.solve(K, np.concatenate([-dq, dh.ravel()[act]]))
    dU = sol[:n]
    return dict(U=dU, X=xs.ravel() + Psi @ dU, lam=sol[n:], active=act)


def fd_jvp_model(w1: dict, tan: dict, step: float = 1e-6) -> dict:
    """Central differences of the C oracle's U and its rollout X along ``tan`` (a workload of one): every operand of
    ``tan`` moves at once, the weights by ``tan["w"]``."""
    outs = []
    for s in (step, -step):
        w2 = dict(w1)
        for key, d in tan.items():
            if d is None:
                continue
            if key == "w":
                for name, dw in zip(WEIGHTS, np.asarray(d, dtype=float)):
                    if w1[name] is not None:
                        w2[name] = float(w1[name]) + s * float(dw)
                continue
            base = np.asarray(w1[key], dtype=float)
            w2[key] = base + s * np.asarray(d, dtype=float).reshape(base.shape)
        U, _, _, st = AN.solve(w2)
        assert st == 0
        X = integrate(problem_from_workload(w2, 0), np.asarray(w2["x0"][0]), U)
        outs.append((U, np.asarray(X).ravel()))
    return dict(U=(outs[0][0] - outs[1][0]) / (2 * step), X=(outs[0][1] - outs[1][1]) / (2 * step))


def random_model_tangent(w1: dict, rng, lam_size: int) -> dict:
    """One random unit-normal tangent of every operand the problem has, x0 .. e as ``tangent_np.random_tangent``. The
    weights' tangent is relative, dw_i = w_i z_i (w_u may be 1e-6: an absolute unit step would leave the positive
    weights a difference quotient needs), and zero for a weight that is not set."""
    N = int(w1["N"])
    nx, nu = np.asarray(w1["x0"]).shape[-1], np.asarray(w1["B"]).shape[-1]
    mk = lam_size // N
    out = TN.random_tangent(w1, rng)
    for key, shp in (("A", (N, nx, nx)), ("B", (N, nx, nu)), ("C", (N, mk, nx)), ("D", (N, mk, nu))):
        if w1[key] is not None and mk + (key in "AB") > 0:
            out[key] = rng.standard_normal(shp)
    out["w"] = np.array([0.0 if w1[k] is None else float(w1[k]) * rng.standard_normal() for k in WEIGHTS])
    return out


def pairing(tan: dict, g: dict, gm: dict) -> float:
    """sum over operands of <gradient, tangent>: ``g`` from adjoint_np.vjp, ``gm`` from adjoint_model_np.model_vjp."""
    total = 0.0
    for key, d in tan.items():
        grad = g[key] if key in TN.KEYS else gm[key]
        total += float(np.asarray(grad, dtype=float).ravel() @ np.asarray(d, dtype=float).ravel())
    return total
