"""CPU tests: the inputs of tests/test_gpu_verdicts.py are what tests/verdict_cases.py claims. For every distinct case behind the
routes of tests/operand_layouts.py, on the C oracle:

  * the mixed batch is [0, 2, 0, 0, 0, 0, 2, 2, 0]; the row pair of items 1, 6 and 7 condensed in np.longdouble has G0 + G1 == 0
    exactly and h0 + h1 < 0 (infeasible by the Farkas vector (1, 1)); the plans of the six untouched items are bitwise those of
    the clean batch;
  * with a terminal weight of -50 every item is MPCQP_NOT_PD and min eig(P) < 0;
  * a limit k exists that leaves at least two items with a count <= k - 1 and two with a count >= k + 1;
  * at least three items have three or more multipliers above 1e-6 (1 + max lam): under max_iter = 1 they cannot be solved by a
    method that admits one row per iteration;
  * the oracle's own iteration limit follows the rule include/mpcqp.h states: a problem that takes `it` iterations is solved
    under max_iter >= it and MPCQP_MAX_ITER below;

and the shared-model and dense-QP batches: the six good items solved, the three bad ones MPCQP_INFEASIBLE."""

import numpy as np
import pytest

import oracle

import operand_layouts as OL
import verdict_cases as VC

CASES = [routes[0] for routes in VC.distinct_cases().values()]
_INTERIOR = {}


def _interior(route):
    if route not in _INTERIOR:
        _INTERIOR[route] = VC.interior(OL.route_case(route, 0)[1][1])
    return _INTERIOR[route]


def test_the_routes_share_seventeen_cases():
    groups = VC.distinct_cases()
    assert sorted(r for routes in groups.values() for r in routes) == sorted(OL.ROUTES)
    assert len(groups) == 17
    assert VC.GOOD == (0, 2, 3, 4, 5, 8) and VC.MIXED_STATUS.tolist() == [0, 2, 0, 0, 0, 0, 2, 2, 0]
    for route, r in OL.ROUTES.items():
        assert r["shape"][3] >= 2, route


@pytest.mark.parametrize("route", CASES)
def test_mixed_batch(route):
    _, (_, full) = OL.route_case(route, 0)
    Uc, _, stc = OL.oracle_on_full(route, 0)
    w, k = VC.mixed(full)
    U, _, st, _ = oracle.solve_workload(w)
    assert np.array_equal(st, VC.MIXED_STATUS), st
    for b in VC.INFEASIBLE:
        G0, G1, h0, h1 = VC.condensed_row_pair(w, b, k)
        assert G0.dtype == np.longdouble and np.abs(G0).max() > 0
        assert (G0 + G1 == 0).all() and h0 + h1 < 0, (b, h0, h1)
        cq = VC.condensed(w, b)  # (the oracle's own rows, in float64)
        mk = w["e"].shape[-1]
        assert (cq.G[k * mk] + cq.G[k * mk + 1] == 0).all() and cq.h[k * mk] + cq.h[k * mk + 1] < 0
    good = list(VC.GOOD)
    assert (stc == 0).all() and np.array_equal(U[good].view(np.uint8), Uc[good].view(np.uint8))
    for X in ("A", "B", "C", "D", "e", "x0", "goal", "targets"):  # (the untouched items' operands are the clean batch's)
        if full[X] is not None:
            assert np.array_equal(w[X][good], full[X][good]), X


@pytest.mark.parametrize("route", CASES)
def test_indefinite_batch(route):
    _, (_, full) = OL.route_case(route, 0)
    w = VC.indefinite(full)
    st = oracle.solve_workload(w)[2]
    assert (st == 3).all(), st
    for b in range(OL.BATCH):
        assert np.linalg.eigvalsh(VC.condensed(w, b).P).min() < 0, b
    assert full["wt"] > 0


@pytest.mark.parametrize("route", CASES)
def test_iteration_limit_inputs(route):
    _, (_, full) = OL.route_case(route, 0)
    _, lam, st = OL.oracle_on_full(route, 0)
    c = oracle.solve_workload(full)[3]
    a = VC.active_counts(lam)
    assert (st == 0).all() and (c >= a).all(), (c, a)
    k, below, above = VC.choose_limit(c)
    assert k is not None and below >= 2 and above >= 2, c
    assert (a >= 3).sum() >= 3, a
    free = _interior(route)
    assert np.array_equal(c == 0, free), (c, free)
    # the oracle's rule: solved under max_iter >= c[b] (same plan, same count), given up below it
    for limit in (k, 1):
        Ul, _, stl, cl = oracle.solve_workload(full, max_iter=limit)
        assert np.array_equal(stl, np.where(c <= limit, 0, 1)), (limit, c, stl)
        assert np.array_equal(cl[stl == 0], c[stl == 0])
        assert (stl[a >= limit + 2] == 1).all()
    assert ((a >= 3) & (stl == 1)).sum() >= 3


def test_interior_items():
    """how many items have a feasible unconstrained minimiser (iters must be 0 for them): one, item 1 of the case of "quad general,
    streamed". The GPU test's `iters == 0` check runs on that route alone; every other item of every case needs an iteration."""
    have = {route: np.flatnonzero(_interior(route)).tolist() for route in CASES}
    assert {r: v for r, v in have.items() if v} == {"quad general, streamed": [1]}, have


def test_boundary_limits():
    # items 2 and 8 took partial steps (c - a = 4 and 2): their counts, the larger gap first; never k itself
    c, a = [10, 4, 13, 12, 9, 3, 13, 6, 15], [10, 4, 9, 12, 9, 3, 13, 6, 13]
    assert VC.boundary_limits(c, a, 10) == [13, 15] and VC.boundary_limits(c, a, 13) == [15]
    assert VC.boundary_limits([5, 7, 7, 5, 11, 6, 9, 5, 7], [5, 7, 5, 5, 7, 6, 7, 5, 7], 6, most=2) == [11, 7]
    # no partial step anywhere: the median count, or its nearest neighbour when the median is k
    c = [6, 4, 1, 7, 6, 7, 9, 8, 6]
    assert VC.boundary_limits(c, c, 5) == [6] and VC.boundary_limits(c, c, 6) == [7]
    for k in range(1, 10):
        assert all(v in c and v != k for v in VC.boundary_limits(c, c, k))


def test_choose_limit():
    assert VC.choose_limit([0, 0, 1, 2, 2, 3, 5, 6, 7]) == (2, 3, 4)  # (k = 3 gives (5, 3): a tie, the smaller k is taken)
    assert VC.choose_limit([0, 0, 0, 0, 4, 4, 5, 6, 7]) == (1, 4, 5)
    assert VC.choose_limit([0, 1, 4, 4, 4, 4, 4, 6, 7]) == (2, 2, 7)
    assert VC.choose_limit([0, 0, 4, 4, 4, 4, 4, 9, 9])[0] in (1, 2, 3, 5, 6, 7, 8)
    assert VC.choose_limit([3] * 9) == (None, 0, 0)
    assert VC.choose_limit([0, 2, 2, 2, 2, 2, 2, 2, 4]) == (None, 0, 0)


@pytest.mark.parametrize("shape", OL.MODEL_SHAPES)
def test_shared_model_band(shape):
    w, full, k = VC.model_mixed(shape)
    assert w["C"].shape[0] == 1 and (w["C"][0, k, 1] == -w["C"][0, k, 0]).all() and (w["D"][0, k, 1] == -w["D"][0, k, 0]).all()
    st = oracle.solve_workload(full)[2]
    assert np.array_equal(st, VC.MIXED_STATUS), st
    stw = oracle.solve_workload(w)[2]
    assert np.array_equal(stw, st)
    for b in range(OL.BATCH):
        G0, G1, h0, h1 = VC.condensed_row_pair(full, b, k)
        assert (G0 + G1 == 0).all()
        assert (h0 + h1 == -2) if b in VC.INFEASIBLE else (h0 > 0 and h1 > 0), (b, h0, h1)  # (good items: u = 0 inside the band)
    lam = oracle.solve_workload(full)[1]
    assert ((lam > 1e-9).any(axis=1)[list(VC.GOOD)]).sum() >= 4


@pytest.mark.parametrize("n,m,f32,tol", VC.DENSE_SIZES)
def test_dense_mixed(n, m, f32, tol):
    P, q, G, h = VC.dense_mixed(n, m)
    if f32:
        P, q, G, h = (a.astype(np.float32).astype(np.float64) for a in (P, q, G, h))
    st = np.array([oracle.gi_solve(P[b], q[b], G[b], h[b])[2] for b in range(OL.BATCH)])
    assert np.array_equal(st, VC.MIXED_STATUS), st
    for b in VC.INFEASIBLE:
        assert (G[b, 0] + G[b, 1] == 0).all() and h[b, 0] + h[b, 1] == -2
