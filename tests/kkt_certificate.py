"""Independent KKT certificate of one problem of a workload dict (plain helper module for the tests, no fixtures).

The verdict of a QP solve -- the C oracle's or a HIP kernel's -- is checked from scratch: the item is condensed by the NumPy
restatement of the reference build (oracle/condense_np.py) and the four KKT conditions of

    min 1/2 u'Pu + q'u   s.t.   G u <= h

are evaluated in extended precision (np.longdouble) at the returned plan U and multipliers lam. Each quantity is scaled the
way the oracle's acceptance rule scales it (mpc_oracle.c, end of oracle_gi_solve): rows by 1 + |h_i|, multipliers by
1 + max(lam). The primal half can also be formed without condensing, by the long-double roll-out of
qpmpc_amd/workloads.py:row_residuals -- ``certify(..., rollout=True)`` cross-checks the two.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np

from oracle.condense_np import condense
from qpmpc_amd.workloads import problem_from_workload, row_residuals, tight_ltv

# Acceptance bounds. PRIMAL is the oracle's bound on its active rows (1e-9 (1 + |h_i|)); DUAL its clamp of a weakly active row's
# multiplier (-1e-12 (1 + umax)), with room for a kernel that reports multipliers after one fewer refinement; COMPLEMENTARITY
# and STATIONARITY are the same 1e-9 relative to the problem's scale (a multiplier that was zeroed while clearly negative
# leaves |lam_i| |G_i| in the stationarity residual, orders of magnitude above these).
PRIMAL, DUAL, COMPLEMENTARITY, STATIONARITY = 1e-9, 1e-12, 1e-9, 1e-8


class Certificate(NamedTuple):
    primal: float           # max_i (G u - h)_i / (1 + |h_i|)            (<= 0: feasible)
    dual: float             # max_i -lam_i / (1 + max lam)               (<= 0: dual feasible)
    complementarity: float  # max_i |lam_i (h - G u)_i| / ((1 + max lam) (1 + |h_i|))
    stationarity: float     # max_j |P u + q + G' lam|_j / ((1 + max lam) (1 + max |G|) + max |q| + max |P| max |u|)
    ok: bool

    def __str__(self):
        return (f"primal {self.primal:.2e} dual {self.dual:.2e} complementarity {self.complementarity:.2e} "
                f"stationarity {self.stationarity:.2e} -> {'pass' if self.ok else 'FAIL'}")


_CACHE: Dict[tuple, tuple] = {}


def condensed(w: Dict, b: int):
    """(P, q, G, h) of item ``b`` by oracle/condense_np.py, as long doubles (memoised per workload dict and item)."""
    key = (id(w), b)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is w:
        return hit[1]
    cq = condense(problem_from_workload(w, b))
    LD = np.longdouble
    out = (cq.P.astype(LD), cq.q.astype(LD), cq.G.astype(LD), cq.h.astype(LD))
    if len(_CACHE) > 4096:
        _CACHE.clear()
    _CACHE[key] = (w, out)
    return out


def certify(w: Dict, b: int, U, lam, rollout: bool = False, active: Optional[np.ndarray] = None) -> Certificate:
    """KKT certificate of item ``b`` of workload ``w`` at plan ``U`` (n) and multipliers ``lam`` (m).

    ``lam=None``: only the primal half is certified (a launch that returns no multipliers); then ``active`` -- a boolean mask of
    the rows some other solve found active -- adds the check that those rows sit on their bounds. ``rollout``: the primal
    residual is also formed by the roll-out and the larger of the two is reported."""
    P, q, G, h = condensed(w, b)
    other = row_residuals(w, b, np.asarray(U, dtype=np.float64)) if rollout else None
    return certify_qp(P, q, G, h, U, lam, active=active, other_residual=other)


def certify_qp(P, q, G, h, U, lam, active: Optional[np.ndarray] = None, other_residual=None) -> Certificate:
    """certify() of a QP given as dense arrays (min 1/2 u'Pu + q'u s.t. G u <= h); ``other_residual``: G u - h formed some other
    way, the larger of the two is reported."""
    LD = np.longdouble
    P, q, G, h = (np.asarray(a).astype(LD) for a in (P, q, G, h))
    u = np.asarray(U, dtype=np.float64).reshape(-1).astype(LD)
    r = G @ u - h  # G u - h
    rows = LD(1) + np.abs(h)
    primal = r / rows
    if other_residual is not None:
        primal = np.maximum(primal, other_residual / rows)
    prim = float(primal.max()) if primal.size else 0.0
    if lam is None:
        on = 0.0
        if active is not None and np.any(active):
            on = float(np.abs(primal[np.asarray(active, dtype=bool)]).max())
        ok = bool(np.isfinite(u.astype(np.float64)).all()) and prim <= PRIMAL and on <= PRIMAL
        return Certificate(prim, 0.0, on, 0.0, ok)
    lm = np.asarray(lam, dtype=np.float64).reshape(-1).astype(LD)
    scale = LD(1) + max(LD(0), lm.max() if lm.size else LD(0))
    dual = float((-lm / scale).max()) if lm.size else 0.0
    comp = float((np.abs(lm * r) / (scale * rows)).max()) if lm.size else 0.0
    s = P @ u + q + G.T @ lm
    norm = scale * (LD(1) + (np.abs(G).max() if G.size else LD(0))) + np.abs(q).max() + np.abs(P).max() * np.abs(u).max()
    stat = float((np.abs(s) / norm).max())
    finite = bool(np.isfinite(u.astype(np.float64)).all() and np.isfinite(lm.astype(np.float64)).all())
    ok = finite and prim <= PRIMAL and dual <= DUAL and comp <= COMPLEMENTARITY and stat <= STATIONARITY
    return Certificate(prim, dual, comp, stat, ok)


def worst(certs) -> Certificate:
    """Element-wise worst of several certificates (the figures a campaign reports)."""
    certs = list(certs)
    if not certs:
        return Certificate(0.0, 0.0, 0.0, 0.0, True)
    return Certificate(max(c.primal for c in certs), max(c.dual for c in certs), max(c.complementarity for c in certs),
                       max(c.stationarity for c in certs), all(c.ok for c in certs))


def tight_narrow(seed: int, tight: float, rounds: int, batch: int):
    """The ``stress_tight narrow`` family (qpmpc_amd/workloads.py: tight_ltv): ``rounds`` workload dicts of ``batch`` problems."""
    rng = np.random.default_rng(seed)
    return [tight_ltv("narrow", rng, batch, tight) for _ in range(rounds)]
