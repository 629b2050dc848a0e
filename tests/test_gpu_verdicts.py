"""GPU tests (-m gpu): the verdict contract of include/mpcqp.h on every forward route of tests/operand_layouts.py -- "status[b] and
iters[b] are written for every problem; U of a problem with status[b] != 0 is all zeros" -- and MpcqpSolveOpts.max_iter.

The other forward tests launch batches in which every problem is solvable and compare "solved or not". Here the code itself is
held (MPCQP_MAX_ITER 1, MPCQP_INFEASIBLE 2, MPCQP_NOT_PD 3), on batches where the items that fail share a wavefront with items
that run on, and the iteration limit is held to a bound that no kernel's own count enters. The inputs are those of
tests/verdict_cases.py (tests/test_verdict_cases_cpu.py shows on the C oracle that they are what they claim to be), launched
through Forward of tests/guarded_launch.py under the 0xFF fill: an output that was never written holds -1 or NaN.
No kernel's multipliers are read: every expectation comes from the oracle or from the same kernel's unlimited launch.

  test_mixed_batch         items 1, 6 and 7 infeasible among six solvable ones: status exactly [0, 2, 0, 0, 0, 0, 2, 2, 0]
  test_indefinite_hessian  a terminal weight of -50: MPCQP_NOT_PD for all nine, and nothing of it sticks in the workspace
  test_iteration_limit     max_iter = k (chosen from the route's own unlimited counts) and max_iter = 1
  test_shared_model_mixed, test_dense_qp_mixed: the mixed batch through mpcqp_solve_model_bounds_batch and mpcqp_solve_batch

With MPCQP_VERDICT_REPORT=<path> a complete run writes the per-route table of profiles/verdicts.txt."""
import os

import numpy as np
import pytest

import oracle

import operand_layouts as OL
import verdict_cases as VC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers and comparisons; needs torch)
from guarded_launch import Forward, ModelCase, QPs, against_oracle, equal_outputs  # noqa: E402
from guarded_launch import flags as _flags  # noqa: E402


F, F64, F32, I32, U8 = GL.F, GL.F64, GL.F32, GL.I32, GL.U8
MAX_ITER, INFEASIBLE, NOT_PD = 1, 2, 3
NARROW = ("narrow stage-wise", "narrow stage-wise, stage-wise entry")  # (their code 1 and 2 items go to the wide kernel)
ROUTES = list(OL.ROUTES)
GOOD = list(VC.GOOD)
BAD = list(VC.INFEASIBLE)

SEEN = {}  # route -> what the report prints


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MPCQP_VERDICT_REPORT")
    cols = ("mixed", "not_pd", "k", "below", "band", "above", "iters_k", "iters_1", "more", "band2", "partial", "interior")
    if path and list(SEEN) == ROUTES and all(all(c in SEEN[r] for c in cols) for r in ROUTES):  # (a partial run writes nothing)
        with open(path, "w") as fh:
            fh.write("tests/test_gpu_verdicts.py, 9 problems per launch, fill 0xFF. mixed: the codes of the batch with items 1, 6, 7\n"
                     "infeasible; not PD: the codes with a terminal weight of -50; k: the limit chosen from the route's unlimited counts\n"
                     "c; below / band / above: solved of items with c <= k - 1, c == k, c >= k + 1 under max_iter = k; largest iters\n"
                     "written by a launch under max_iter = k and under max_iter = 1 (over all items, solved or given up). partial: items\n"
                     "with c > a (a: rows active at the oracle's solution), which took a partial step; k2: the further limits, each the\n"
                     "count of such an item (or the median count); band2: solved of the items with c == k2, over those launches;\n"
                     "interior: items whose unconstrained minimiser is feasible (iters must be 0).\n\n")
            fh.write(f"{'route':40s} {'mixed':20s} {'not PD':7s} {'k':>3s} {'below':>6s} {'band':>6s} {'above':>6s} {'iters<=k':>9s} {'iters<=1':>9s} {'partial':>8s} {'band2':>6s} {'interior':>9s}  k2\n")
            for r in ROUTES:
                s = SEEN[r]
                fh.write(f"{r:40s} {s['mixed']:20s} {s['not_pd']:7s} {s['k']:3d} {s['below']:>6s} {s['band']:>6s} {s['above']:>6s} "
                         f"{s['iters_k']:9d} {s['iters_1']:9d} {s['partial']:8d} {s['band2']:>6s} {s['interior']:9d}  {s['more']}\n")


def _case(route, w):
    r = OL.ROUTES[route]
    case = Forward(w, dtype=F32 if r["f32"] else None, stagewise=r["stagewise"])
    assert case.B == OL.BATCH
    return case, _flags(r["flags"]), (1e-3 if r["f32"] else 1e-7)


def _written(out, what):
    """iters of every item is written (the fill reads -1) and is a count"""
    assert (out["iters"] >= 0).all(), (what, "iters", out["iters"])


def _no_plan(out, items, code, what):
    assert (out["status"][items] == code).all(), (what, out["status"])
    assert not np.isnan(out["U"]).any(), what
    assert (out["U"][items] == 0).all(), (what, "U of an item without a plan is not zeros", out["U"][items])
    _written(out, what)


# ---------------------------------------------------------------------------------------------- 1. mixed batches
@pytest.mark.parametrize("route", ROUTES)
def test_mixed_batch(route):
    """Items 1, 6 and 7 are infeasible (a row and its negative, both bounds -1), the other six are the clean batch's: return code 0
    (Launch.run), status exactly [0, 2, 0, 0, 0, 0, 2, 2, 0], U of the three exact zeros, iters of all nine written, and the six
    within the route's bound of the oracle on the same batch. A lane neighbour that is frozen must not disturb the ones that run on:
    item 1 has solvable neighbours at two and at four per wavefront, 6 and 7 fill a two-per-wavefront slot beside 4 and 5."""
    key, (_, full) = OL.route_case(route, 0)
    w, _ = VC.mixed(full)
    case, flags, tol = _case(route, w)
    out = case.run(F, flags)
    print(f"    {route}: status {out['status'].tolist()} iters {out['iters'].tolist()}")
    SEEN.setdefault(route, {})["mixed"] = "".join(str(int(s)) for s in out["status"])
    assert np.array_equal(out["status"], VC.MIXED_STATUS), out["status"]
    _no_plan(out, BAD, INFEASIBLE, route)
    ok = against_oracle(repr(key) + " mixed", w, out, tol)
    assert np.array_equal(np.flatnonzero(ok), GOOD)


# ---------------------------------------------------------------------------------------------- 2. indefinite Hessian
@pytest.mark.parametrize("route", ROUTES)
def test_indefinite_hessian(route):
    """The clean batch with MpcqpDims.w_terminal = -50: P is indefinite (the stage-wise kernels meet it as a Riccati stage that is
    not PD: P is PD exactly when every stage is), so every status is MPCQP_NOT_PD, U exact zeros, iters written. Then w_terminal is
    restored and the same arena, its workspace as the indefinite launch left it, gives the bits of a launch on a freshly filled
    one: nothing sticks."""
    _, (_, full) = OL.route_case(route, 0)
    case, flags, _ = _case(route, full)
    clean = case.run(F, flags)
    assert (clean["status"] == 0).all(), clean["status"]
    wt = case.dims.w_terminal
    assert wt > 0
    case.dims.w_terminal = VC.W_TERMINAL_INDEFINITE
    bad = case.run(F, flags)
    case.dims.w_terminal = wt
    print(f"    {route}: status {bad['status'].tolist()} iters {bad['iters'].tolist()}")
    SEEN.setdefault(route, {})["not_pd"] = "".join(sorted({str(int(s)) for s in bad["status"]}))
    _no_plan(bad, slice(None), NOT_PD, route)
    again = case.run(F, flags, keep=("ws",))
    equal_outputs(clean, again, route + ": after the indefinite launch, workspace kept")


# ---------------------------------------------------------------------------------------------- 3. the iteration limit
def _limited(route, case, flags, tol, Uo, limit, a):
    """one launch under max_iter = limit. Safety: every item reported solved is within the route's bound of the oracle, every
    other one is MPCQP_MAX_ITER with U exact zeros, iters written (iters = max_iter, the header's rule, but on the narrow
    stage-wise routes), no NaN. The limit is honoured: a method that admits one row per iteration cannot solve an item with
    limit + 2 or more rows active at the oracle's solution."""
    out = case.run(F, flags, max_iter=limit)
    st = out["status"]
    print(f"    {route}, max_iter {limit}: status {st.tolist()} iters {out['iters'].tolist()}")
    assert np.isin(st, (0, MAX_ITER)).all(), st
    _no_plan(out, st != 0, MAX_ITER, f"{route}, max_iter {limit}")
    if route not in NARROW:
        assert (out["iters"][st != 0] == limit).all(), (limit, out["iters"])
    if (st == 0).any():
        scale = np.maximum(1.0, np.abs(Uo).max(axis=1, keepdims=True))
        err = float((np.abs(out["U"].astype(np.float64) - Uo) / scale)[st == 0].max())
        assert err <= tol, (limit, err)
    must = a >= limit + 2
    assert (st[must] == MAX_ITER).all(), (f"max_iter {limit}: solved with {a.tolist()} rows active at the solution", st)
    return out


def _per_item(route, unl, out, c, limit):
    """under max_iter = limit every item is judged on its own count, whatever shares its wavefront: those with c <= limit are the
    unlimited launch's bitwise (status, iters, U, lam), those with c >= limit + 1 are MPCQP_MAX_ITER"""
    equal_outputs(unl, out, f"{route}: items with c <= {limit}", items=c <= limit)
    assert (out["status"][c <= limit] == 0).all()
    assert (out["status"][c >= limit + 1] == MAX_ITER).all(), (limit, c, out["status"])


@pytest.mark.parametrize("route", ROUTES)
def test_iteration_limit(route):
    """Every kernel counts what the oracle counts, one step of the dual active-set method (a row admitted, or a blocking row
    dropped), per problem, and admits one row per counted iteration: no route needs another unit. The unlimited launch solves all
    nine with counts c: c >= a, the rows active at the oracle's solution, and c == 0 for the items whose unconstrained minimiser
    is feasible by 1e-6 (iters feeds mpcqp_order_by_count; of the 17 cases only that of "quad general, streamed" has such an item,
    item 1: tests/test_verdict_cases_cpu.py::test_interior_items, and the report's last column but one).

    Launches under three kinds of limit, all safe and honouring the limit (_limited), and all judged item by item against the
    unlimited launch (_per_item: c <= limit bitwise its status, iters, U and lam -- the boundary c == limit included, the rule
    include/mpcqp.h states --, c >= limit + 1 MPCQP_MAX_ITER):
      k     splits c into at least two items on either side (verdict_cases.choose_limit);
      1     nearly every item is given up in its first trips, beside the few that need one step or none;
      k2    verdict_cases.boundary_limits: the count c[b] of each item with c[b] > a[b], up to four. Such an item took a partial
            step, and the trip that then removes the blocking row is not counted: the item has fallen behind the rows that share
            its wavefront, and under max_iter = c[b] it is solved only if the limit is compared with ITS count -- the wavefront's
            trip count is already past the limit when it takes its last step. A route with no such item gets the median count, so
            that every route has an item exactly on the boundary. The k2 launches are repeated on the batch sorted by falling
            count, where such an item sits beside the items most likely to be given up while it still runs: a given-up item
            must freeze without taking its lane neighbours with it.
    The two narrow stage-wise routes are held to safety and the limit only: their MPCQP_MAX_ITER items are solved again by the
    wide kernel and iters is then that kernel's count."""
    key, (_, full) = OL.route_case(route, 0)
    case, flags, tol = _case(route, full)
    unl = case.run(F, flags, max_iter=0)
    c = unl["iters"].astype(np.int64)
    print(f"    {route}: unlimited counts {c.tolist()}")
    assert (unl["status"] == 0).all(), unl["status"]
    against_oracle(repr(key), full, unl, tol)
    Uo, lamo, sto = GL.oracle_of(repr(key), full)
    a = VC.active_counts(lamo)
    assert (sto == 0).all()
    assert (c >= a).all(), (c, a)
    free = VC.interior(full)
    assert (c[free] == 0).all() and (c[a > 0] > 0).all(), (c, free)
    k, below, above = VC.choose_limit(c)
    assert k is not None and below >= 2 and above >= 2, c
    at_k = _limited(route, case, flags, tol, Uo, k, a)
    at_1 = _limited(route, case, flags, tol, Uo, 1, a)
    assert ((a >= 3) & (at_1["status"] == MAX_ITER)).sum() >= 3

    def solved(mask):
        return f"{int((at_k['status'][mask] == 0).sum())}/{int(mask.sum())}"

    more = VC.boundary_limits(c, a, k)
    assert more and all((c == k2).any() for k2 in more), (c, a, more)
    at_more = [_limited(route, case, flags, tol, Uo, k2, a) for k2 in more]
    hit = sum(int((out["status"][c == k2] == 0).sum()) for k2, out in zip(more, at_more))
    SEEN.setdefault(route, {}).update(k=k, below=solved(c <= k - 1), band=solved(c == k), above=solved(c >= k + 1),
                                      iters_k=int(at_k["iters"].max()), iters_1=int(at_1["iters"].max()), more=str(more),
                                      band2=f"{hit}/{sum(int((c == k2).sum()) for k2 in more)}", partial=int((c > a).sum()),
                                      interior=int(free.sum()))
    if route in NARROW:
        return
    _per_item(route, unl, at_k, c, k)
    _per_item(route, unl, at_1, c, 1)
    for k2, out in zip(more, at_more):
        _per_item(route, unl, out, c, k2)
    # the same nine problems sorted by falling count, so that an item that has fallen behind (c > a) shares its wavefront with
    # items that reach the limit while it still runs: they are given up beside it, and it must run on to its own count
    perm = np.argsort(-c, kind="stable")
    sorted_w = {name: (v[perm] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == OL.BATCH else v) for name, v in full.items()}
    case2, _, _ = _case(route, sorted_w)
    unl2 = case2.run(F, flags, max_iter=0)
    c2, a2 = unl2["iters"].astype(np.int64), a[perm]
    print(f"    {route}: sorted by count, unlimited counts {c2.tolist()}")
    assert (unl2["status"] == 0).all() and (c2 >= a2).all(), (unl2["status"], c2, a2)
    for k2 in VC.boundary_limits(c2, a2, None):
        _per_item(route + ", sorted by count", unl2, _limited(route, case2, flags, tol, Uo[perm], k2, a2), c2, k2)


# ---------------------------------------------------------------------------------------------- the shared-model export
@pytest.mark.parametrize("per_wave", ["OPT_TWO_PER_WAVE", "OPT_FOUR_PER_WAVE"])
@pytest.mark.parametrize("shape", OL.MODEL_SHAPES)
def test_shared_model_mixed(shape, per_wave):
    """mpcqp_solve_model_bounds_batch, two and four per wavefront: the model is shared, so every problem has the band (row 1 of step
    N // 2 the negative of row 0); e of the six good items keeps u = 0 feasible, e of items 1, 6 and 7 is -1, -1
    (verdict_cases.model_mixed). Set up as tests/test_gpu_operand_layouts.py::test_shared_model_solves (ModelCase, the model
    factored in the arena)."""
    nx, nu, N, mk = shape
    w, full, _ = VC.model_mixed(shape)
    for key, width in (("x0", nx), ("goal", nx), ("targets", N * nx), ("e", N * mk)):
        assert w[key].reshape(w[key].shape[0], -1).shape == (OL.BATCH, width)
    out = ModelCase(w, factor_in_arena=True).run(F, _flags([per_wave]))
    print(f"    model {shape} {per_wave}: status {out['status'].tolist()} iters {out['iters'].tolist()}")
    assert np.array_equal(out["status"], VC.MIXED_STATUS), out["status"]
    _no_plan(out, BAD, INFEASIBLE, f"model {shape}")
    ok = against_oracle(f"model mixed {shape}", full, out, 1e-7)
    assert np.array_equal(np.flatnonzero(ok), GOOD)


# ---------------------------------------------------------------------------------------------- the dense-QP export
@pytest.mark.parametrize("n,m,f32,tol", VC.DENSE_SIZES)
def test_dense_qp_mixed(n, m, f32, tol):
    """mpcqp_solve_batch at every size of tests/test_gpu_memory_discipline.py::test_dense_qp_solver (the small-problem kernel, the
    workgroup kernel and the workspace-resident solver), nine problems, the row pair written into G and h of items 1, 6 and 7."""
    P, q, G, h = VC.dense_mixed(n, m)
    assert len(q) == OL.BATCH
    out = QPs(P, q, G, h, dtype=F32 if f32 else F64, workspace=True).run(F, 0)
    print(f"    dense QP n {n} m {m}: status {out['status'].tolist()} iters {out['iters'].tolist()}")
    assert np.array_equal(out["status"], VC.MIXED_STATUS), out["status"]
    _no_plan(out, BAD, INFEASIBLE, f"dense QP {n} {m}")
    ref = GL.f32_view(dict(P=P, q=q, G=G, h=h)) if f32 else dict(P=P, q=q, G=G, h=h)
    for b in GOOD:
        xo, _, so, _ = oracle.gi_solve(ref["P"][b], ref["q"][b], ref["G"][b], ref["h"][b])
        assert so == 0
        err = float(np.abs(out["U"][b].astype(np.float64) - xo).max() / max(1.0, np.abs(xo).max()))
        assert err <= tol, (b, err)
