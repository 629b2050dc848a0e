"""CPU: the oracle's SOLVED verdicts on the nearly fully active families (tools/stress_tight.py narrow, which every stress test
compares against) hold up under an independent KKT certificate (tests/kkt_certificate.py), and the oracle's clamp of negative
multipliers after refinement is bounded by its acceptance rule."""
import ctypes as C

import numpy as np
import pytest

import oracle
from kkt_certificate import certify, tight_narrow, worst


@pytest.mark.parametrize("tight", [0.5, 0.3, 0.15, 0.05])
def test_oracle_solutions_pass_the_kkt_certificate_on_tight_narrow_families(tight):
    """24 rounds of 32 problems per tightness (3072 in all): every item the oracle reports SOLVED passes the certificate -- primal
    feasibility, dual feasibility, complementarity and stationarity in long double, on the NumPy restatement of the build -- and its
    primal residual agrees with the roll-out of qpmpc_amd/workloads.py:row_residuals."""
    certs, solved = [], 0
    for w in tight_narrow(int(100 * tight) + 11, tight, 24, 32):
        U, lam, st, _ = oracle.solve_workload(w)
        for b in np.flatnonzero(st == 0):
            c = certify(w, int(b), U[b], lam[b], rollout=True)
            assert c.ok, (tight, int(b), str(c))
            certs.append(c)
        solved += int((st == 0).sum())
    assert solved >= (600 if tight >= 0.15 else 300)  # (the families are solvable, not only tight)
    print(f"STRESS_TIGHT {tight}: {solved} solved items, worst {worst(certs)}")


def test_certificate_rejects_a_wrong_active_set():
    """The certificate is no formality: the oracle's plan with one active row's multiplier zeroed fails stationarity, the plan
    moved off the bounds by 1e-6 fails primal feasibility, a negative multiplier fails dual feasibility."""
    (w,) = tight_narrow(61, 0.3, 1, 8)
    U, lam, st, _ = oracle.solve_workload(w)
    b = int(np.flatnonzero(st == 0)[0])
    assert certify(w, b, U[b], lam[b]).ok
    act = np.flatnonzero(lam[b] > 0)
    i = act[np.argmax(lam[b][act])]
    dropped = lam[b].copy()
    dropped[i] = 0.0
    assert not certify(w, b, U[b], dropped).ok
    assert not certify(w, b, U[b] + 1e-6 * np.sign(np.random.default_rng(0).standard_normal(U.shape[1])), lam[b]).ok
    negative = lam[b].copy()
    negative[i] = -1e-3
    assert certify(w, b, U[b], negative).dual > 0


def _clamp(u):
    lib = oracle.capi._load()
    u = np.ascontiguousarray(u, dtype=float)
    neg = lib.oracle_clamp_multipliers(C.c_int(len(u)), u.ctypes.data_as(C.c_void_p))
    return neg, u


def test_clamp_zeroes_rounding_level_multipliers_only():
    """oracle_clamp_multipliers (mpc_oracle.c), the rule oracle_gi_solve applies after refining the final active set and again in
    its acceptance check: a multiplier down to -1e-12 (1 + max u) is a weakly active row's and becomes 0; a clearly negative one
    stays negative and is counted, so the solve is refused instead of reported SOLVED with that active set."""
    neg, u = _clamp([3.0, -3e-12, 0.5])
    assert neg == 0 and u.tolist() == [3.0, 0.0, 0.5]
    neg, u = _clamp([3.0, -1e-3, 0.5])
    assert neg == 1 and u[1] == -1e-3
    neg, u = _clamp([1e8, -1e-3])  # (relative to the largest multiplier: -1e-11 (1 + 1e8) is beyond the bound)
    assert neg == 1 and u[1] == -1e-3
    neg, u = _clamp([-1e-13])  # (no positive multiplier: the bound is -1e-12)
    assert neg == 0 and u[0] == 0.0
    neg, u = _clamp([float("nan"), 1.0])
    assert neg == 1


def test_gi_solve_on_a_degenerate_vertex_returns_a_certified_point():
    """End to end through the clamp: three rows through one vertex of the plane, two of them nearly parallel (an ill-conditioned
    active set). The solve ends SOLVED at the vertex with every multiplier >= 0 and stationarity to 1e-9. (No QP found in random
    searches makes the refinement itself leave a clearly negative multiplier; the rule is pinned directly above.)"""
    eps = 1e-8
    P = np.eye(2)
    q = np.array([-1.0, -1.0])
    G = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, eps]])
    h = np.zeros(3)
    x, lam, st, _ = oracle.gi_solve(P, q, G, h)
    assert st == 0
    assert (lam >= 0).all()
    stat = np.abs(P @ x + q + G.T @ lam).max()
    assert stat <= 1e-9 and np.abs(x).max() <= 1e-12
