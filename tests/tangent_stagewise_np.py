"""NumPy float64 restatement of the stage-wise tangent (test helper, not an oracle module).

The same KKT system as tests/tangent_np.py,

    [P  G_A'] [dU    ]   [-dq ]
    [G_A  0 ] [dlam_A] = [dh_A],     A = {i : lam_i > 0},

solved without condensing: P = L L' is the whitened Riccati recursion of ``oracle.stagewise_qr_np.WhitenedRiccati``, as in
tests/adjoint_stagewise_np.py. Per tangent (dx0, dgoal, dtargets, de):

1. xs = rollout(dx0, 0) with the problem's A_k (this is Phi dx0);
2. dq = Psi' c with c_k = w_x (xs_k - dtargets_k) on states 0 .. N-1 (MPCQP_Q_STAGE; state 0 does not reach the inputs) and
   c_N = w_t (xs_N - dgoal) (MPCQP_Q_TERMINAL), as ``oracle.condense_np.cost_vector`` indexes them;
3. r = -L^-1 dq: one backward sweep;
4. dh_A = de_A - (C xs)_A, mu = S^-1 (Y_A r - dh_A) with S = Y_A Y_A' = R R' of the active rows' whitened vectors;
5. dU = L^-T (r - Y_A' mu): one forward sweep from x = 0, whose states are Psi dU; dX = xs + Psi dU.

The factorisation, Y_A and R do not depend on the tangent. This is what mpcqp_tangent_stagewise_kernel
(qpmpc_amd/csrc/mpcqp_adjoint_stagewise.hip) computes, step for step ("Stage-wise forward
sensitivities").
"""
from __future__ import annotations

import numpy as np

from oracle.capi import FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
from oracle.stagewise_np import from_mpc_problem
from oracle.stagewise_qr_np import WhitenedRiccati
from qpmpc_amd.workloads import problem_from_workload

from adjoint_stagewise_np import _steps

NOT_PD = 3


class Factorisation:
    """What does not depend on the tangent: the Riccati records, the active rows' whitened vectors and their Gram factor.
    ``status`` is 0, or NOT_PD when a stage Hessian or the Gram matrix is not positive definite or more rows are active
    than there are variables."""

    def __init__(self, w1: dict, lam):
        p = problem_from_workload(w1, 0)
        sp = from_mpc_problem(p)
        self.N, self.nx, self.nu = N, nx, nu = sp.N, sp.nx, sp.nu
        self.n = n = N * nu
        lam = np.asarray(lam, dtype=float)
        self.mk = mk = len(lam) // N if N else 0
        f = flags_of(p)
        self.qt, self.qs = bool(f & FLAG_Q_TERMINAL), bool(f & FLAG_Q_STAGE)
        self.wt = p.terminal_cost_weight or 0.0
        self.wx = p.stage_state_cost_weight or 0.0
        self.A = _steps(w1, "A", (nx, nx))
        self.C, D = _steps(w1, "C", (mk, nx)), _steps(w1, "D", (mk, nu))
        self.status = 0
        self.ric = ric = WhitenedRiccati(sp)
        self.act = act = np.flatnonzero(lam > 0.0)
        k = len(act)
        if not ric.pd or k > n:
            self.status = NOT_PD
            return
        self.Y = Y = np.zeros((k, n))
        for a, i in enumerate(act):
            j, r = divmod(int(i), mk)
            ql, rl = np.zeros((N, nx)), np.zeros((N, nu))
            ql[j], rl[j] = -self.C[j, r], -D[j, r]
            Y[a] = ric.backward(ql, rl, ktop=j).reshape(n)
        self.R = None
        if k:
            try:
                self.R = np.linalg.cholesky(Y @ Y.T)
            except np.linalg.LinAlgError:
                self.status = NOT_PD

    def jvp(self, tan: dict) -> dict:
        """dU [n] and dX [(N+1)*nx] along ``tan`` (a dict over x0, goal, targets, e; a missing key is a zero tangent)."""
        N, nx, nu, n, mk = self.N, self.nx, self.nu, self.n, self.mk
        if self.status:
            return dict(U=np.zeros(n), X=np.zeros((N + 1) * nx), status=self.status)

        def get(key, size):
            v = tan.get(key)
            return np.zeros(size) if v is None else np.asarray(v, dtype=float).reshape(size)

        dx0, dgoal = get("x0", nx), get("goal", nx)
        dtargets, de = get("targets", (N, nx)), get("e", N * mk)
        # 1. xs = rollout(dx0, 0)
        xs = np.zeros((N + 1, nx))
        xs[0] = dx0
        for kk in range(N):
            xs[kk + 1] = self.A[kk] @ xs[kk]
        # 2. the cost tangent's per-state vector c
        c = np.zeros((N + 1, nx))
        if self.qs:
            c[:N] = self.wx * (xs[:N] - dtargets)
        if self.qt:
            c[N] = self.wt * (xs[N] - dgoal)
        # 3. r = -L^-1 Psi' c: WhitenedRiccati.backward(q, r, pN) is -L^-1 (Psi' q + r + Psi_N' pN)
        r = self.ric.backward(c[:N], np.zeros((N, nu)), pN=c[N]).reshape(n)
        # 4. mu = S^-1 (Y_A r - dh_A)
        s = r
        if len(self.act):
            dh = de[self.act] - np.array([self.C[i // mk, i % mk] @ xs[i // mk] for i in self.act])
            mu = np.linalg.solve(self.R.T, np.linalg.solve(self.R, self.Y @ r - dh))
            s = r - self.Y.T @ mu
        # 5. dU = L^-T s and its states Psi dU: one forward sweep from x = 0
        dU, Z = self.ric.forward(s.reshape(N, nu))
        return dict(U=dU.reshape(n), X=(xs + Z).ravel(), status=0)


def stagewise_jvp(w1: dict, lam, tan: dict) -> dict:
    """One tangent of one problem (workload of one, ``adjoint_np.single``) at multipliers ``lam``."""
    return Factorisation(w1, lam).jvp(tan)
