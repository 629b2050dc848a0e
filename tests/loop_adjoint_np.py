"""The reverse-time recursion of mpcqp_model_periods_vjp_batch restated in NumPy (test helper; no GPU).

Loop b, period t: the plan solves the model's problem at x_t, goal_t, targets_t; u0_t is its first input (zero without a
plan) and x_{t+1} = Ap x_t + Bp u0_t + d_t. Given cotangents gX [B, P+1, nx] and gU0 [B, P, nu], with a = gX_P and
t = P-1 .. 0:

    g_d_t = a;  g_Ap += a x_t';  g_Bp += a u0_t';  ubar = gU0_t + Bp' a;  a_new = gX_t + Ap' a
    a period with a plan, A = {i : lam_i > 0}, S = M_A M_A':
        tt = L^-1 [ubar; 0];  nu = S^-1 M_A tt;  w = tt - M_A' nu
        a_new -= Wx' w + Hx_A' nu;  g_goal_t = Wg' w;  g_targets_t = Wt' w
    a = a_new

and g_x0 = a at the end (include/mpcqp.h; DESIGN.md section 9, "Closed-loop adjoint"). Dense linear algebra per period on
model_loop_np.condense_lti: it states WHAT the kernel computes. `loop_vjp` takes the multipliers and statuses of
model_loop_np.oracle_loop; `margins` is the strict-complementarity margin that decides which loops a test may compare."""
from __future__ import annotations

import numpy as np

import model_loop_cases as cases
import model_loop_np as ML

# GRAD_RTOL: the bound of the GPU gradients against this restatement fed the oracle loop's multipliers, and of the fused path
# against the composed one, |err| <= GRAD_RTOL * max(1, |ref|). Measured, not chosen (profiles/loop_diff.md,
# tools/measure_loop_diff_parity.py): ten times the largest error of closed_loop_diff(fused=False) -- the loop composed from
# SharedModel.solve_diff, the kernels of the parent commit -- against the restatement over every gradient, case, batch and
# period count of tests/test_gpu_loop_diff.py, the factor for re-associated sums; never looser than 1e-6.
# Measured on the MI355X: 1.060e-11 (g_Ap of triple_infeasible at 5 loops x 7 periods; the triple family at w_input = 1e-6 sets
# every large figure, the box cases stay under 1.3e-12), rounded up. The fused path measured 1.058e-11 on the same table.
COMPOSED_PATH_ERROR = 1.1e-11
GRAD_RTOL = min(10.0 * COMPOSED_PATH_ERROR, 1e-6)


def _plant(case, b):
    Ap, Bp = case["Ap"], case["Bp"]
    return (Ap[b] if Ap.ndim == 3 else Ap), (Bp[b] if Bp.ndim == 3 else Bp)


def loop_vjp(case, ref, gX, gU0, md=None):
    """-> dict(x0 [B, nx], states [B, P+1, nx] (the costates a_0 .. a_P: states[:, 1:] is the disturbance's gradient),
    goal [B, P, nx], targets [B, P, N nx], Ap [B, nx, nx], Bp [B, nx, nu], failed [B]) per loop, nothing summed over the batch.
    `ref`: model_loop_np.oracle_loop's dict (X, U0, lam [P, B, m], status [P, B])."""
    c = case
    md = md or ML.condense_lti(c)
    nx, nu, N = c["nx"], c["nu"], c["N"]
    n = md["n"]
    Li = np.linalg.inv(md["L"])
    X, U0 = ref["X"], ref["U0"]
    Bn, P = U0.shape[0], U0.shape[1]
    has_goal = bool(c["wt"])
    has_targets = bool(c["wx"]) and c["targets"] is not None
    out = dict(x0=np.zeros((Bn, nx)), states=np.zeros((Bn, P + 1, nx)), goal=np.zeros((Bn, P, nx)),
               targets=np.zeros((Bn, P, N * nx)), Ap=np.zeros((Bn, nx, nx)), Bp=np.zeros((Bn, nx, nu)),
               failed=np.zeros(Bn, dtype=np.int64))
    for b in range(Bn):
        Ap, Bp = _plant(c, b)
        a = np.array(gX[b, P], dtype=float)
        out["states"][b, P] = a
        for t in range(P - 1, -1, -1):
            out["Ap"][b] += np.outer(a, X[b, t])
            out["Bp"][b] += np.outer(a, U0[b, t])
            ubar = gU0[b, t] + Bp.T @ a
            a_new = gX[b, t] + Ap.T @ a
            if ref["status"][t, b] == 0:
                act = np.flatnonzero(ref["lam"][t, b] > 0)
                u = np.zeros(n)
                u[:nu] = ubar
                tt = Li @ u
                ok = len(act) <= n
                nuv = np.zeros(0)
                if ok and len(act):
                    MA = md["M"][act]
                    try:
                        Lc = np.linalg.cholesky(MA @ MA.T)
                        nuv = np.linalg.solve(Lc.T, np.linalg.solve(Lc, MA @ tt))
                    except np.linalg.LinAlgError:
                        ok = False
                if ok:
                    w = tt - (md["M"][act].T @ nuv if len(act) else 0.0)
                    a_new = a_new - md["Wx"].T @ w
                    if len(act):
                        a_new = a_new - md["Hx"][act].T @ nuv
                    if has_goal:
                        out["goal"][b, t] = md["Wg"].T @ w
                    if has_targets:
                        out["targets"][b, t] = md["Wt"].T @ w
                else:
                    out["failed"][b] += 1
            a = a_new
            out["states"][b, t] = a
        out["x0"][b] = a
    return out


def plant_adjoint(case, gX, b):
    """The costates of loop b when no period has a plan: a_P = gX_P, a_t = gX_t + Ap' a_{t+1}. -> [P+1, nx]"""
    Ap, _ = _plant(case, b)
    P = gX.shape[1] - 1
    a = np.zeros((P + 1, gX.shape[2]))
    a[P] = gX[b, P]
    for t in range(P - 1, -1, -1):
        a[t] = gX[b, t] + Ap.T @ a[t + 1]
    return a


def margins(case, ref, md=None):
    """[B]: per loop, over its periods WITH a plan, the smaller of the smallest positive multiplier and the smallest slack of an
    inactive row whose row of M is not zero (a zero row constrains nothing and is ignored); inf for a loop without any plan.
    A loop whose margin is small sits next to a change of its active set: its plan is not differentiable to the accuracy a
    test asks for, and a central difference straddles the kink."""
    c = case
    md = md or ML.condense_lti(c)
    norms = np.linalg.norm(md["M"], axis=1)
    P, Bn = ref["status"].shape
    out = np.full(Bn, np.inf)
    for t in range(P):
        for b in range(Bn):
            if ref["status"][t, b] != 0:
                continue
            lam = ref["lam"][t, b]
            act = lam > 0
            y = md["L"].T @ ref["U"][t, b]
            slack = md["e"] - md["Hx"] @ ref["X"][b, t] - md["M"] @ y
            free = ~act & (norms > 0)
            mg = min(lam[act].min() if act.any() else np.inf, slack[free].min() if free.any() else np.inf)
            out[b] = min(out[b], mg)
    return out


def cotangents(case, periods, ref=None, seed=11):
    """Seeded cotangents (gX [B, P+1, nx], gU0 [B, P, nu]) of a case: standard normal, and with `ref` (the oracle loop) each
    record in units of its own range, gX / max(1, max |X|) and gU0 / max(1, max |U0|). A central difference of the oracle
    loop carries the oracle's rounding of every record, |c_i| eps_i / 2h, and the records differ in size by orders of
    magnitude (the triple family: |X| <= 3, |U0| up to 86, the jerk being the least certain record at w_input = 1e-6): with
    unit cotangents on both the jerk's rounding alone is the whole error budget of a comparison at h = 1e-6."""
    rng = np.random.default_rng(seed)
    Bn = case["x0"].shape[0]
    gX, gU0 = rng.standard_normal((Bn, periods + 1, case["nx"])), rng.standard_normal((Bn, periods, case["nu"]))
    if ref is not None:
        gX, gU0 = gX / max(1.0, np.abs(ref["X"]).max()), gU0 / max(1.0, np.abs(ref["U0"]).max())
    return gX, gU0


def loss_per_loop(res, gX, gU0):
    """[B]: <gX, X> + <gU0, U0> of every loop."""
    return (gX * res["X"]).sum(axis=(1, 2)) + (gU0 * res["U0"]).sum(axis=(1, 2))


def central_difference(case, periods, gX, gU0, key, index, h=1e-6):
    """[B]: d loss_b / d case[key][..., index] by central differences of the oracle loop; every loop's entry moves at once
    (the loops do not interact), `index` addresses the axes behind the loop axis -- or all axes of an operand the batch shares."""
    per_loop = case[key].ndim > len(index)
    vals = []
    for s in (+h, -h):
        c = dict(case)
        a = np.array(case[key], dtype=float)
        a[(slice(None),) + tuple(index) if per_loop else tuple(index)] += s
        c[key] = a
        vals.append(loss_per_loop(ML.oracle_loop(c, periods), gX, gU0))
    return (vals[0] - vals[1]) / (2.0 * h)


__all__ = ["loop_vjp", "plant_adjoint", "margins", "cotangents", "loss_per_loop", "central_difference", "cases"]
