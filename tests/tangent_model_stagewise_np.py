"""NumPy float64 restatement of the stage-wise tangent with model and weight tangents (test helper, not an oracle module).

tests/tangent_model_np.py's system, solved without condensing on the whitened Riccati recursion as
tests/tangent_stagewise_np.py solves its own, step for step as the kModel instantiation of
mpcqp_tangent_stagewise_kernel (qpmpc_amd/csrc/mpcqp_adjoint_stagewise.hip) does it:

once per problem  X = rollout(x0, U), Z = rollout(0, U), the costate pi by its backward recursion with A_k;
per tangent       a. xs (and zs) by the rollout with the forcing term dA_k X_k + dB_k u_k;
                  b. r = -L^-1 (Psi' c + g): the backward sweep started from gX = -c, gU = -g;
                  c. dh_A = de_A - (C xs)_A - (dC X)_A - (dD u)_A,  mu = S^-1 (Y_A r - dh_A);
                  d. dU = L^-T (r - Y_A' mu) by the forward sweep from x = 0, dX = xs + its states.
"""
from __future__ import annotations

import numpy as np

import tangent_model_np as TM
import tangent_stagewise_np as TS


class ModelFactorisation(TS.Factorisation):
    """``tangent_stagewise_np.Factorisation`` with the plan U: what no tangent changes, X, Z and pi included."""

    def __init__(self, w1: dict, U, lam):
        super().__init__(w1, lam)
        self.shared = TM.Shared(w1, U, lam)

    def jvp_model(self, tan: dict) -> dict:
        """dU [n] and dX [(N+1)*nx] along ``tan`` (a dict over x0, goal, targets, e, A, B, C, D, w)."""
        N, nx, nu, n = self.N, self.nx, self.nu, self.n
        if self.status:
            return dict(U=np.zeros(n), X=np.zeros((N + 1) * nx), status=self.status)
        xs, c, g, dh = self.shared.rhs(tan)
        # b. WhitenedRiccati.backward(q, r, pN) is -L^-1 (Psi' q + r + Psi_N' pN)
        r = self.ric.backward(c[:N], g, pN=c[N]).reshape(n)
        s = r
        if len(self.act):
            mu = np.linalg.solve(self.R.T, np.linalg.solve(self.R, self.Y @ r - dh.ravel()[self.act]))
            s = r - self.Y.T @ mu
        dU, Zs = self.ric.forward(s.reshape(N, nu))
        return dict(U=dU.reshape(n), X=(xs + Zs).ravel(), status=0)


def stagewise_jvp_model(w1: dict, U, lam, tan: dict) -> dict:
    """One tangent of one problem (workload of one, ``adjoint_np.single``) at its plan ``U`` and multipliers ``lam``."""
    return ModelFactorisation(w1, U, lam).jvp_model(tan)
