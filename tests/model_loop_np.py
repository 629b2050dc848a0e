"""Restatements of the closed loop of a shared model (test helper, NumPy + the C oracle; no GPU).

oracle_loop   the loop of include/mpcqp.h (mpcqp_model_periods_batch) with oracle.capi.build_solve_batch per period: solve at
              the current state, apply the first input (zero without a plan), step the plant, count. THE reference of the
              GPU tests.
warm_loop_np  the same loop with the kernel's warm period restated in NumPy on the whitened matrices M = G L^-T,
              w = L^-1 q: the kept set's multipliers, the drops, the slacks from scratch, the active-set loop, the
              from-scratch verification and the cold restart (steps 1 to 4 of the kernel's header comment). Dense linear
              algebra per step instead of the kernel's rank-one updates: it states WHAT the warm period computes."""
from __future__ import annotations

import numpy as np

from oracle import capi

import model_loop_cases as cases


def _flags(case) -> int:
    return capi.workload_flags(dict(wt=case["wt"], wx=case["wx"], goal=case["goal"], targets=case["targets"]))


def plant_step(case, x, u0, t):
    Ap, Bp = case["Ap"], case["Bp"]
    if Ap.ndim == 3:
        return np.einsum("bij,bj->bi", Ap, x) + np.einsum("bij,bj->bi", Bp, u0) + case["dist"][:, t]
    return x @ Ap.T + u0 @ Bp.T + case["dist"][:, t]


def oracle_loop(case, nperiods: int, t0: int = 0, x0=None):
    """-> dict(X [B, P+1, nx], U0 [B, P, nu], status [P, B], iters [P, B], lam [P, B, m], U [P, B, n], failed [B])."""
    c = case
    nx, nu, N, mk = c["nx"], c["nu"], c["N"], c["mk"]
    x = np.array(c["x0"] if x0 is None else x0, dtype=float)
    X, U0, ST, IT, LAM, UU = [x.copy()], [], [], [], [], []
    for t in range(t0, t0 + nperiods):
        goal = np.ascontiguousarray(cases.goal_at(c, t))
        tg = cases.targets_at(c, t)
        U, lam, st, it = capi.build_solve_batch(nx, nu, N, mk, _flags(c), c["wt"], 0.0 if c["wx"] is None else c["wx"], c["wu"],
                                                c["A"], c["B"], c["C"], c["D"], c["e"], x, goal,
                                                None if tg is None else np.ascontiguousarray(tg), tol=c["tol"])
        u0 = np.where((st == 0)[:, None], U[:, :nu], 0.0)
        x = plant_step(c, x, u0, t)
        X.append(x.copy())
        U0.append(u0)
        ST.append(st.copy())
        IT.append(it.copy())
        LAM.append(lam.copy())
        UU.append(np.where((st == 0)[:, None], U, 0.0))
    ST = np.array(ST)
    return dict(X=np.stack(X, 1), U0=np.stack(U0, 1), status=ST, iters=np.array(IT), lam=np.array(LAM), U=np.array(UU),
                failed=(ST != 0).sum(0))


# ------------------------------------------------------------------ the whitened problem of one loop and period
def condense_lti(case):
    """(L, M, Hx, Wx, Wg, Wt, e_rows) of the shared model: P = L L', M = G L^-T, h = e - Hx x0, w = Wx x0 - Wg goal - Wt targets."""
    c = case
    nx, nu, N, mk = c["nx"], c["nu"], c["N"], c["mk"]
    A, B = c["A"], c["B"]
    n, m = N * nu, N * mk
    Phi = [np.eye(nx)]
    Psi = [np.zeros((nx, n))]
    for k in range(N):
        P_next = A @ Psi[k]
        P_next[:, k * nu:(k + 1) * nu] += B
        Psi.append(P_next)
        Phi.append(A @ Phi[k])
    wt = c["wt"] or 0.0
    wx = c["wx"] or 0.0
    P = c["wu"] * np.eye(n) + wt * Psi[N].T @ Psi[N]
    for k in range(1, N):
        P += wx * Psi[k].T @ Psi[k]
    G, Hx = np.zeros((m, n)), np.zeros((m, nx))
    for k in range(N):
        rows = slice(k * mk, (k + 1) * mk)
        if c["C"] is not None:
            G[rows] += c["C"] @ Psi[k]
            Hx[rows] = c["C"] @ Phi[k]
        if c["D"] is not None:
            G[rows, k * nu:(k + 1) * nu] += c["D"]
    L = np.linalg.cholesky(P)
    Li = np.linalg.inv(L)
    Qx = wt * Psi[N].T @ Phi[N] + sum(wx * Psi[k].T @ Phi[k] for k in range(1, N))
    Qg = wt * Psi[N].T
    Qt = np.zeros((n, N * nx))
    for k in range(1, N):
        Qt[:, k * nx:(k + 1) * nx] = wx * Psi[k].T
    return dict(L=L, M=G @ Li.T, Hx=Hx, Wx=Li @ Qx, Wg=Li @ Qg, Wt=Li @ Qt, e=np.tile(c["e"], N), n=n, m=m)


def _multipliers(M, h, y_unc, act):
    MA = M[act]
    return -np.linalg.solve(MA @ MA.T, h[act] - MA @ y_unc)


def solve_period_np(M, w, h, tol, active=(), max_iter=None):
    """One period on the whitened problem min 1/2 |y|^2 + w.y, M y <= h. `active`: the kept set of a warm period (empty:
    cold). -> (y or None, active list, status, iterations). Status 0 only through the from-scratch verification."""
    m, n = M.shape
    max_iter = max_iter or 10 * (n + m) + 10
    tolh = tol * (1.0 + np.abs(h))
    norms = np.linalg.norm(M, axis=1)
    invn = np.where(norms > 0, 1.0 / np.where(norms > 0, norms, 1.0), 1.0)
    y_unc = -w
    act = list(active)
    iters = 0
    lam = np.zeros(0)
    # steps 1 and 2: multipliers of the equality-constrained problem on the kept set; the most negative one leaves
    while act:
        lam = _multipliers(M, h, y_unc, act)
        if lam.min() >= 0:
            break
        act.pop(int(np.argmin(lam)))
        iters += 1
    if not act:
        lam = np.zeros(0)
    for _round in range(4):
        while True:
            # step 3: y from the multipliers, slacks from scratch (0 on active rows)
            y = y_unc - (M[act].T @ lam if act else 0.0)
            s = h - M @ y
            s[act] = 0.0
            viol = (s < -tolh) & (h < 1e29)
            viol[act] = False
            if not viol.any():
                break
            p = int(np.argmin(np.where(viol, s * invn, np.inf)))
            up = 0.0
            while True:  # the step along row p: partial steps drop a row, the full step adds p
                if iters >= max_iter:
                    return None, act, 1, iters
                iters += 1
                if act:
                    MA = M[act]
                    r = np.linalg.solve(MA @ MA.T, MA @ M[p])
                    z = -M[p] + MA.T @ r
                else:
                    r = np.zeros(0)
                    z = -M[p]
                d2 = float(z @ z)
                can_move = len(act) < n and d2 * invn[p] ** 2 > 1e-14 and d2 > 0
                cand = r > 0
                t1, l = (np.inf, -1)
                if cand.any():
                    ratios = np.where(cand, lam / np.where(cand, r, 1.0), np.inf)
                    l = int(np.argmin(ratios))
                    t1 = ratios[l]
                sp = h[p] - M[p] @ (y_unc - (M[act].T @ lam if act else 0.0) - up * M[p])  # (p's own multiplier so far: up)
                t2 = -sp / d2 if can_move else np.inf
                t = min(t1, t2)
                if not np.isfinite(t):
                    return None, act, 2, iters
                lam = np.maximum(lam - t * r, 0.0)
                up += t
                if t2 <= t1:
                    act.append(p)
                    lam = np.append(lam, up)
                    break
                act.pop(l)
                lam = np.delete(lam, l)
        # step 4: accept only through the verification at the point the refined multipliers imply
        if act:
            lam = np.maximum(_multipliers(M, h, y_unc, act), 0.0)
        y = y_unc - (M[act].T @ lam if act else 0.0)
        fresh = h - M @ y
        bad = (fresh < -4.0 * tolh) & (h < 1e29)
        bad[act] = False
        if not bad.any():
            return y, act, 0, iters
    return None, act, 1, iters


def warm_loop_np(case, nperiods: int, warm: bool = True):
    """The loop with the warm period in NumPy -> dict(X, U0, status [P, B], iters [P, B], recold [B])."""
    c = case
    nu = c["nu"]
    md = condense_lti(c)
    Linv_T = np.linalg.inv(md["L"]).T
    x = np.array(c["x0"], dtype=float)
    Bn = x.shape[0]
    kept = [[] for _ in range(Bn)]
    X, U0, ST, IT = [x.copy()], [], [], []
    recold = np.zeros(Bn, dtype=np.int64)
    for t in range(nperiods):
        goal = np.broadcast_to(cases.goal_at(c, t), x.shape)
        tg = cases.targets_at(c, t)
        u0 = np.zeros((Bn, nu))
        st, it = np.zeros(Bn, dtype=np.int32), np.zeros(Bn, dtype=np.int32)
        for b in range(Bn):
            h = md["e"] - md["Hx"] @ x[b]
            w = md["Wx"] @ x[b] - md["Wg"] @ goal[b]
            if tg is not None:
                w = w - md["Wt"] @ (tg if tg.ndim == 1 else tg[b])
            y, act, s_, i_ = solve_period_np(md["M"], w, h, c["tol"], kept[b] if warm else ())
            if s_ != 0 and warm and kept[b]:
                # a stale state costs a cold restart, never a wrong plan
                recold[b] += 1
                y, act, s_, i2 = solve_period_np(md["M"], w, h, c["tol"])
                i_ += i2
            kept[b] = list(act) if s_ == 0 else []
            st[b], it[b] = s_, i_
            if s_ == 0:
                u0[b] = (Linv_T @ y)[:nu]
        x = plant_step(c, x, u0, t)
        X.append(x.copy())
        U0.append(u0)
        ST.append(st)
        IT.append(it)
    return dict(X=np.stack(X, 1), U0=np.stack(U0, 1), status=np.array(ST), iters=np.array(IT), recold=recold)
