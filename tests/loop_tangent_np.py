"""The forward-time recursion of mpcqp_model_periods_jvp_batch restated in NumPy (test helper; no GPU).

Loop b, period t, of the loop loop_adjoint_np states: given tangents dx0, dgoal_t, dtargets_t, dd_t (the disturbance), dAp and
dBp, with dx_0 = dx0 and t = 0 .. P-1:

    a period with a plan, A = {i : lam_i > 0}, k = |A| <= n, S = M_A M_A' positive definite:
        r = -(Wx dx_t - Wg dgoal_t - Wt dtargets_t);  mu = S^-1 (M_A r + Hx_A dx_t);  du0_t = [L^-T (r - M_A' mu)]_{0 .. nu-1}
    otherwise du0_t = 0 (a failed S or k > n is counted in `failed`)
    dx_{t+1} = Ap dx_t + Bp du0_t + dd_t + dAp x_t + dBp u0_t

(include/mpcqp.h; DESIGN.md section 9, "Closed-loop forward sensitivities"). Dense linear algebra per period on
model_loop_np.condense_lti: it states WHAT the kernel computes. `loop_jvp` takes the multipliers and statuses of
model_loop_np.oracle_loop, as loop_adjoint_np.loop_vjp does, and is its transpose: <gX, dX> + <gU0, dU0> = <g, tangents>."""
from __future__ import annotations

import numpy as np

import model_loop_np as ML

# TANGENT_RTOL: the bound of the GPU tangents against this restatement fed the oracle loop's multipliers, and of the fused path
# against the composed one, |err| <= TANGENT_RTOL * max(1, |ref|). Measured, not chosen (profiles/loop_jvp.md,
# tools/measure_loop_jvp_parity.py): ten times the largest error of closed_loop_jvp(fused=False) -- the loop composed from
# SharedModel.solve and SharedModel.plan_jvp, the kernels of the parent commit -- against the restatement over dX and dU0 of
# every case, batch, period count and T of tests/test_gpu_loop_jvp.py, the factor for re-associated sums; never looser than 1e-6.
# Measured on the MI355X: 8.711e-09 (dU0 of triple at 67 loops x 7 periods, T = 17; the triple family at w_input = 1e-6 sets
# every large figure; tiny stays under 2.5e-11 and box4, box5 and wide16 under 1.3e-13), rounded up. The fused path measured
# 8.712e-09 on the same table.
COMPOSED_PATH_ERROR = 8.8e-9
TANGENT_RTOL = min(10.0 * COMPOSED_PATH_ERROR, 1e-6)


def _plant(case, b):
    Ap, Bp = case["Ap"], case["Bp"]
    return (Ap[b] if Ap.ndim == 3 else Ap), (Bp[b] if Bp.ndim == 3 else Bp)


def tangent_shapes(case, periods):
    """{operand: the shape behind [B, T]} of a full set of tangents, every reference with a period axis."""
    nx, nu, N = case["nx"], case["nu"], case["N"]
    return dict(x0=(nx,), goal=(periods, nx), targets=(periods, N * nx), dist=(periods, nx), Ap=(nx, nx), Bp=(nx, nu))


def tangents(case, periods, T, seed=5, shared=False):
    """Seeded standard-normal tangents on all six operands: {operand: [B, T, ...]} ([1, T, ...] with `shared`)."""
    rng = np.random.default_rng(seed)
    Bn = 1 if shared else case["x0"].shape[0]
    return {k: rng.standard_normal((Bn, T) + s) for k, s in tangent_shapes(case, periods).items()}


def loop_jvp(case, ref, tan, md=None):
    """-> dict(dX [B, T, P+1, nx], dU0 [B, T, P, nu], failed [B]). `tan`: {operand: [B|1, T, ...] or None}, the shapes of
    `tangent_shapes` (a reference's tangent without the period axis is constant in time); `ref`: model_loop_np.oracle_loop's
    dict (X, U0, lam [P, B, m], status [P, B])."""
    c = case
    md = md or ML.condense_lti(c)
    nx, nu = c["nx"], c["nu"]
    n = md["n"]
    LiT = np.linalg.inv(md["L"]).T
    X, U0 = ref["X"], ref["U0"]
    Bn, P = U0.shape[0], U0.shape[1]
    has_goal = bool(c["wt"])
    has_targets = bool(c["wx"]) and c["targets"] is not None
    T = next(v.shape[1] for v in tan.values() if v is not None)

    def at(key, b, j, t=None):
        v = tan.get(key)
        if v is None:
            return None
        v = v[b if v.shape[0] > 1 else 0, j]
        return v if t is None or v.ndim == 1 else v[t]

    dX, dU0 = np.zeros((Bn, T, P + 1, nx)), np.zeros((Bn, T, P, nu))
    failed = np.zeros(Bn, dtype=np.int64)
    for b in range(Bn):
        Ap, Bp = _plant(c, b)
        for t in range(P):
            plan = ref["status"][t, b] == 0
            ok, act, Lc = plan, np.zeros(0, dtype=int), None
            if plan:
                act = np.flatnonzero(ref["lam"][t, b] > 0)
                ok = len(act) <= n
                if ok and len(act):
                    MA = md["M"][act]
                    try:
                        Lc = np.linalg.cholesky(MA @ MA.T)
                    except np.linalg.LinAlgError:
                        ok = False
                if not ok:
                    failed[b] += 1
            for j in range(T):
                if t == 0:
                    v = at("x0", b, j)
                    dX[b, j, 0] = 0.0 if v is None else v
                dx = dX[b, j, t]
                du0 = np.zeros(nu)
                if ok:
                    r = -(md["Wx"] @ dx)
                    v = at("goal", b, j, t)
                    if has_goal and v is not None:
                        r = r + md["Wg"] @ v
                    v = at("targets", b, j, t)
                    if has_targets and v is not None:
                        r = r + md["Wt"] @ v
                    y = r
                    if len(act):
                        MA = md["M"][act]
                        mu = np.linalg.solve(Lc.T, np.linalg.solve(Lc, MA @ r + md["Hx"][act] @ dx))
                        y = r - MA.T @ mu
                    du0 = (LiT @ y)[:nu]
                nxt = Ap @ dx + Bp @ du0
                v = at("dist", b, j, t)
                if v is not None:
                    nxt = nxt + v
                for key, rec in (("Ap", X[b, t]), ("Bp", U0[b, t])):
                    v = at(key, b, j)
                    if v is not None:
                        nxt = nxt + v @ rec
                dX[b, j, t + 1] = nxt
                dU0[b, j, t] = du0
    return dict(dX=dX, dU0=dU0, failed=failed)


def plant_rollout(case, tan, b, j, X, U0):
    """dX [P+1, nx] of tangent j of loop b when no period has a plan: dx_{t+1} = Ap dx_t + dd_t + dAp x_t + dBp u0_t, in the
    order loop_jvp adds the terms."""
    Ap, Bp = _plant(case, b)
    P = U0.shape[1]
    pick = lambda v: None if v is None else v[b if v.shape[0] > 1 else 0, j]  # noqa: E731
    x0, dd, dA, dB = (pick(tan.get(k)) for k in ("x0", "dist", "Ap", "Bp"))
    out = np.zeros((P + 1, case["nx"]))
    if x0 is not None:
        out[0] = x0
    for t in range(P):
        nxt = Ap @ out[t] + Bp @ np.zeros(case["nu"])
        if dd is not None:
            nxt = nxt + (dd if dd.ndim == 1 else dd[t])
        if dA is not None:
            nxt = nxt + dA @ X[b, t]
        if dB is not None:
            nxt = nxt + dB @ U0[b, t]
        out[t + 1] = nxt
    return out


def pairing(g, tan):
    """[B, T]: <g, tangents> of loop_adjoint_np.loop_vjp's per-loop gradients with a full set of per-loop tangents; also the sum
    of the absolute values of the paired terms, the scale a duality on the device is held to."""
    gs = dict(x0=g["x0"], goal=g["goal"], targets=g["targets"], dist=g["states"][:, 1:], Ap=g["Ap"], Bp=g["Bp"])
    val = mag = 0.0
    for k, gk in gs.items():
        v = tan.get(k)
        if v is None:
            continue
        gk = gk[:, None]
        if v.ndim == gk.ndim - 1:  # constant in time: the gradient's period sum
            gk = gk.sum(axis=2)
        prod = gk * v
        axes = tuple(range(2, prod.ndim))
        val, mag = val + prod.sum(axis=axes), mag + np.abs(prod).sum(axis=axes)
    return val, mag


__all__ = ["loop_jvp", "plant_rollout", "pairing", "tangents", "tangent_shapes", "TANGENT_RTOL"]
