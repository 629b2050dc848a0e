#!/usr/bin/env python3
"""CPU model (NumPy, no GPU) of the active set of the four-per-wavefront kernel (csrc/mpcqp_quad.hip): which trips a problem makes.

The kernel's dual active-set method with the operator explicit in the coordinates M = G L^-T: slots T (row a: T_a), the projector
H = I - M_A' T, selection of the violated row farthest from its hyperplane (s_i / |M_i|, compared on the high word with the row index
in the low five bits, as the kernel's key), tolerance tol (1 + |h_i|) with the C API's default tol = 1e-12, the step length from -M_p . z with the sum of squares near
dependence, the ratio test on the multipliers, and the deferred rank-one updates. A problem is condensed by oracle.capi.condense_one.
The refinement and the acceptance test behind the loop are not modelled: the counts are those of the first pass, which is the only
one in all but rare problems.

trips(problem) -> (iters, status, kinds): kinds has one letter per iteration,
    P  plain: a constraint selected in this trip takes the full step
    d  partial step: a multiplier blocks, its slot leaves (a drop), p is kept
    F  full step with a kept p (after one or more partial steps)
and ends, for a problem that does not solve, with L (iteration limit) or I (inconsistent). The kernel makes one trip of a wavefront
per iteration of each of its four rows that is still live: trip k of a wavefront is iteration k of its rows.

    python tools/quad_trip_model.py [batch]    -- the census of bench.py's headline batch (triple_integrator_batch)"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

DEP, DEP_FAST, INF = 1e-14, 1e-6, float("inf")
SOLVED, MAX_ITER, INFEASIBLE = 0, 1, 2
NV = 16


def _hi(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0] >> 32


def _ordered(x):
    b = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    h, l = b >> 32, b & 0xffffffff
    return ((~h) & 0xffffffff, (~l) & 0xffffffff) if h & 0x80000000 else (h | 0x80000000, l)


def operator(qp):
    """(M, s at the unconstrained optimum, h) of a condensed problem dict(P, q, G, h)"""
    L = np.linalg.cholesky(qp["P"])
    M = np.linalg.solve(L, qp["G"].T).T
    w = np.linalg.solve(L, qp["q"])
    return M, qp["h"] + M @ w, qp["h"]


def active_set(M, s, h, tol=1e-12, max_iter=None):
    """(iters, status, kinds) of the active-set loop on M (m x n), the slacks s at y0 and the bounds h"""
    m, n = M.shape
    max_iter = max_iter or 10 * (n + m) + 10  # (the C API's defaults: mpcqp_capi.hip)
    s = s.copy()
    nn = (M * M).sum(axis=1)
    invn = np.where(nn > 0, 1.0 / np.sqrt(np.where(nn > 0, nn, 1.0)), 1.0)
    sel = h < 1e29
    tolh = tol + tol * np.abs(h)
    T, H = np.zeros((NV, n)), np.eye(n)
    lam, occ, act, e = np.zeros(NV), np.zeros(NV, bool), np.zeros(NV, int), sel.copy()
    nq, p, needp, up, iters, kinds = 0, 0, True, 0.0, 0, ""
    zn, cT, cH = np.zeros(n), np.zeros(NV), np.zeros(n)
    while True:
        T += np.outer(cT, zn)
        H += np.outer(cH, zn)
        if needp:
            keys = [(((~_hi(s[i] * invn[i])) & 0xffffffe0) | i) for i in range(m) if e[i] and s[i] < -tolh[i]]
            if not keys:
                return iters, SOLVED, kinds
            p, up, needp = min(keys) & 31, 0.0, False
            kind = "P"
        else:
            kind = "F"
        mp = M[p]
        hd = H @ mp
        kd = M @ hd
        okf = kd[p] * invn[p] * invn[p] > DEP_FAST
        iv = 1.0 / kd[p] if kd[p] != 0 else INF
        inv, t2 = (iv if okf else -1.0), -s[p] * iv
        rd = T @ mp
        if not inv > 0:
            z2 = float(hd @ hd)
            ok2 = z2 * invn[p] * invn[p] > DEP and z2 > 0
            t2, inv = (-s[p] / z2 if z2 > 0 else INF), (1.0 / z2 if ok2 else 0.0)
        can_move = nq < n and inv > 0
        inv, t2 = (inv if can_move else 0.0), (t2 if can_move else INF)
        sl = int(np.flatnonzero(~occ)[0]) if not occ.all() else NV
        r = np.where(occ, rd, 0.0)
        with np.errstate(invalid="ignore"):  # (t2 = inf against r = 0)
            blk = (r > 0) & (lam < t2 * r)
        if iters >= max_iter:
            return iters, MAX_ITER, kinds + "L"
        iters += 1
        t1, lq = INF, 0
        if blk.any():
            cand = occ & (r > 0)
            ratio = np.where(cand, lam / np.where(cand, r, 1.0), INF)
            key = min((_ordered(ratio[a])[0], _ordered(ratio[a])[1] & 0xffffffe0 | a) for a in range(NV) if cand[a])
            lq = key[1] & 15
            t1 = ratio[lq]
        t = t1 if t1 < t2 else t2
        if not t < INF:
            return iters, INFEASIBLE, kinds + "I"
        full = t2 <= t1
        zn = hd
        cT = np.where(np.arange(NV) == sl, inv, -(r * inv)) if full else np.zeros(NV)
        cH = -(hd * inv) if full else np.zeros(n)
        s += t * kd
        lam = lam - t * r
        lam[occ & (lam < 0)] = 0.0
        up += t
        if full:
            lam[sl], act[sl], occ[sl], e[p] = up, p, True, False
            nq += 1
            needp = True
            kinds += kind
        else:  # the slot of the blocking multiplier leaves: T_a -= (T_a . T_l / T_l . T_l) T_l, H += T_l T_l' / T_l . T_l
            e[act[lq]] = sel[act[lq]]
            vv = T[lq].copy()
            tl = T @ vv
            zn, cT, cH = vv, np.where(np.arange(NV) == lq, -1.0, np.where(occ, -tl / tl[lq], 0.0)), vv / tl[lq]
            lam[lq], occ[lq] = 0.0, False
            nq -= 1
            kinds += "d"


def trips(problem, tol=1e-12, max_iter=None):
    import oracle.capi as OC

    return active_set(*operator(OC.condense_one(problem)), tol=tol, max_iter=max_iter)


def trips_of_workload(w, tol=1e-12, max_iter=None, count=None):
    """[(iters, status, kinds)] of the first `count` problems of a workload dict (qpmpc_amd/workloads.py)"""
    from qpmpc_amd.workloads import problem_from_workload

    return [trips(problem_from_workload(w, b), tol, max_iter) for b in range(len(w["x0"]) if count is None else count)]


def wavefronts(res):
    """the kinds of a launch by wavefront: [[kinds of row 0, .. row 3]] (a last wavefront with idle rows repeats the last problem)"""
    kinds = [k for _, _, k in res]
    kinds += [kinds[-1]] * (-len(kinds) % 4)
    return [kinds[i:i + 4] for i in range(0, len(kinds), 4)]


def main():
    from qpmpc_amd.workloads import triple_integrator_batch

    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    res = trips_of_workload(triple_integrator_batch(batch))
    it = np.array([r[0] for r in res])
    drops = [b for b, r in enumerate(res) if "d" in r[2]]
    print(f"{batch} problems: iterations mean {it.mean():.3f} max {it.max()}; problems that drop: {drops}")
    lens = np.array([max(len(k) for k in wf) for wf in wavefronts(res)])
    print("trips per wavefront (count):", dict(zip(*np.unique(lens, return_counts=True))))
    for b in drops:
        print(f"  problem {b} (wavefront {b // 4}): {res[b][2]}")


if __name__ == "__main__":
    main()
