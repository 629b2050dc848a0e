"""CPU tests: the inputs of tests/test_gpu_degenerate.py are what tests/degenerate_cases.py claims. For every distinct case behind
the routes of tests/operand_layouts.py, for the shared-model and on-chip cases and for the dense QPs, on the C oracle and in
np.longdouble:

  (a) the oracle solves all nine items of every variant with status 0 and its result passes kkt_certificate.certify; a float32
      case is stated in float32-representable numbers throughout (operand_layouts.f32_view of it is a no-op);
  (b) touch and free: every touched row has slack >= 0 at the exact answer and slack <= 2 ulp of the storage type times
      (1 + |e|), in long double; the oracle's plan is within 1e-9 (scaled as against_oracle scales it) of the exact answer;
  (c) the oracle's iteration count on every item of every variant is at most n + m, a tenth of the default limit
      10 (n + m) + 10 of include/mpcqp.h: a kernel that breaks ties differently has tenfold room;
  (d) the variants are degenerate in fact. touch: every item has a touched row, and on every case with n <= 64 at least 6 of 9
      items have at least min(n, m) zero-slack rows (active plus touched), or take another iteration count than nominal
      (min(n, m), not n: "quad general, streamed" has m = 8 rows for n = 16 variables and "general stage-wise" 40 for 60, so no
      vertex of theirs is determined by n rows; with every step touched all m of their rows have zero slack). duplicate and
      band: the modified rows have a positive multiplier sum in the oracle's answer on at least 6 of 9 items;
  (e) free: the exact answer u0 has no active row -- in long double its gradient P u0 + q vanishes and every row is satisfied, so
      (u0, lam = 0) is the KKT point -- and the oracle reports 0 iterations on every item whose rows a float64 minimiser (NumPy's,
      not the oracle's) still satisfies within a twentieth of feas_tol (degenerate_cases.min_slack_f64 >= -5e-14: two float64
      evaluations of one slack differ by about as much as each is off, which leaves the oracle's a factor of twenty). Any float64
      minimiser is off by about cond(P) 2^-53 |u|, 1e-12 on the worst conditioned cases (those without a stage cost, and the
      dense one); there rows that sit on the exact minimiser are violated by more than feas_tol = 1e-12 at the oracle's own, and
      it admits one to eight of them before it returns u0 within 2e-12: item 8 of "quad lean", three of "quad general,
      streamed" and five of "dense HBM f64" (NumPy's slacks there: -1e-13 .. -4e-12). The plan is held to (b) there like
      everywhere else."""
import numpy as np
import pytest

import degenerate_cases as DC
import kkt_certificate as KC
import operand_layouts as OL
import verdict_cases as VC

LD = np.longdouble
CASES = [routes[0] for routes in VC.distinct_cases().values()]
OTHER = DC.other_cases()
DENSE = [(n, m, f32) for n, m, f32, _ in VC.DENSE_SIZES] + [(n, m, False) for n, m in DC.ONCHIP_QP_SIZES]


def _rel(U, ref):
    return float((np.abs(U - ref) / np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))).max())


def _conditions(what, name, v, f32, nominal, solved, n, m, slack_of, certify, f64_slack):
    """(a) .. (e) of one variant of one case. nominal, solved: (U, lam, status, iters) of the oracle on the nominal problems and
    on the variant; slack_of(U): long-double (e - row value) [B, m] of the variant at plan U; certify(b, U, lam): Certificate."""
    B = OL.BATCH
    U, lam, st, it = solved
    rows = v["rows"].reshape(B, m)
    print(f"    {what}, {name}: status {st.tolist()} iters {it.tolist()} (nominal {nominal[3].tolist()})")
    assert (st == 0).all(), st  # (a)
    bad = [(b, str(c)) for b in range(B) for c in [certify(b, U[b], lam[b])] if not c.ok]
    assert not bad, bad
    assert (it <= n + m).all(), (it, n + m)  # (c)
    if v["exact"] is not None:  # (b)
        s = slack_of(v["exact_ld"])
        bound = 2 * DC.ulp(f32) * (1 + np.abs(v["e"].reshape(B, m).astype(LD)))
        assert (s[rows] >= 0).all(), float(s[rows].min())
        assert (s[rows] <= bound[rows]).all(), float((s[rows] / bound[rows]).max())
        assert (s >= -KC.PRIMAL * bound / (2 * DC.ulp(f32))).all()  # (the other rows: the oracle's own bound on its active rows)
        err = _rel(U, v["exact"])
        assert err <= 1e-9, err
    if name == "touch":  # (d)
        assert rows.any(axis=1).all()
        if n <= 64:
            zero = ((lam > 0) | rows).sum(axis=1)
            degenerate = (zero >= min(n, m)) | (it != nominal[3])
            assert degenerate.sum() >= 6, (zero, it, nominal[3])
    if name in ("duplicate", "band"):
        assert ((lam * rows).sum(axis=1) > 0).sum() >= 6, (lam * rows).sum(axis=1)
    if name == "free":  # (e)
        assert (s >= 0).all() and rows.all()
        eligible = np.array([f64_slack(b) >= DC.FREE_SLACK for b in range(B)])
        print(f"    {what}, free: float64 minimiser within a twentieth of feas_tol on items {np.flatnonzero(eligible).tolist()}")
        assert (it[eligible] == 0).all() and (lam[eligible] == 0).all(), (it, eligible)


def _workload_conditions(what, key, full, name, steps, f32):
    nx, nu = full["A"].shape[-1], full["B"].shape[-1]
    B, N, mk = full["e"].shape
    n, m = N * nu, N * mk
    nominal = DC.nominal(key, full)
    v = dict(DC.case_variant(key, full, name, steps, f32))
    w = v["w"]
    v["e"] = w["e"]
    if f32:
        for X, a in OL.f32_view(w).items():
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, w[X]), (what, name, X, "not float32-representable")
    if name == "free":  # in long double: the gradient at u0 vanishes (relative to |q|)
        for b in range(B):
            P, q = DC.cost_ld(full, b)  # (the cost does not depend on e)
            g = P @ v["exact_ld"][b] + q
            assert float(np.abs(g).max()) <= 1e-13 * max(1.0, float(np.abs(q).max())), (b, float(np.abs(g).max()))
    _conditions(what, name, v, f32, nominal, DC.oracle_on(key, name, w), n, m,
                lambda U: w["e"].astype(LD).reshape(B, m) - DC.row_values(w, U).reshape(B, m),
                lambda b, U, lam: KC.certify(w, b, U, lam), lambda b: DC.min_slack_f64(w, b))


@pytest.mark.parametrize("name", DC.VARIANTS)
@pytest.mark.parametrize("route", CASES)
def test_route_case(route, name):
    r = OL.ROUTES[route]
    key, (_, full) = OL.route_case(route, 0)
    assert r["shape"][3] >= 2
    _workload_conditions(route, key, full, name, DC.TOUCH_STEPS[route], r["f32"])


def test_touch_steps_table():
    """every route with n <= 64 touches every step, the larger ones evenly spaced steps; routes that share a case share the
    steps; up() rounds outward in either storage type"""
    assert set(DC.TOUCH_STEPS) == set(OL.ROUTES)
    for routes in VC.distinct_cases().values():
        assert len({DC.TOUCH_STEPS[r] for r in routes}) == 1, routes
    for route, r in OL.ROUTES.items():
        nx, nu, N, mk = r["shape"]
        steps = DC.TOUCH_STEPS[route]
        assert (steps is None) == (N * nu <= 64), route
        if steps is not None:
            assert len(set(steps)) == len(steps) >= 4 and all(0 <= k < N for k in steps) and len(set(np.diff(steps))) == 1
    v = np.array([1, 1 + 2.0 ** -30, 1 + 2.0 ** -60, -1 - 2.0 ** -30, 0.1], dtype=LD) + LD(2) ** -62
    for f32 in (False, True):
        r = DC.up(v, f32)
        t = np.float32 if f32 else np.float64
        assert (r.astype(LD) >= v).all() and (r == r.astype(t)).all()
        assert (np.nextafter(r.astype(t), t(-np.inf)).astype(LD) < v).all()  # (the smallest such number)


def test_free_eligibility_is_not_empty():
    """the 0-iteration half of (e) holds on items chosen by a float64 minimiser's slacks: over the float64 cases with n <= 64 at
    least half of all items are chosen (few or none on the cases without a stage cost, "quad lean" and "quad general, streamed",
    whose cond(P) is 5e3 .. 4e4, and fewer as n grows) -- the check cannot silently become empty"""
    total, count = 0, 0
    for route in CASES:
        r = OL.ROUTES[route]
        if r["f32"] or r["shape"][1] * r["shape"][2] > 64:
            continue
        key, (_, full) = OL.route_case(route, 0)
        w = DC.case_variant(key, full, "free", DC.TOUCH_STEPS[route], False)["w"]
        eligible = sum(DC.min_slack_f64(w, b) >= DC.FREE_SLACK for b in range(OL.BATCH))
        print(f"    {route}: {eligible} of {OL.BATCH} items held to 0 iterations")
        total, count = total + eligible, count + OL.BATCH
    assert 2 * total >= count, (total, count)


@pytest.mark.parametrize("name", DC.VARIANTS)
@pytest.mark.parametrize("label", list(OTHER))
def test_other_case(label, name):
    """the shared-model cases (the model stays shared under duplicate and band: degenerate_cases.shared asserts it) and the
    on-chip kernel's nine general problems"""
    key, full = OTHER[label]
    _workload_conditions(label, key, full, name, None, False)
    if key[0] == "model":
        w = DC.shared(DC.case_variant(key, full, name)["w"])
        assert w["C"].shape[0] == 1 and w["e"].shape[0] == OL.BATCH


@pytest.mark.parametrize("name", DC.VARIANTS)
@pytest.mark.parametrize("n,m,f32", DENSE)
def test_dense_case(n, m, f32, name):
    v = dict(DC.dense_variant(n, m, f32, name))
    P, q, G, h = v["qp"]
    v["e"] = h
    nominal = DC.dense_oracle(("dense", n, m, f32), *DC.dense_nominal(n, m, f32))
    solved = DC.dense_oracle(("dense", n, m, f32, name), P, q, G, h)
    if f32:
        for a in (P, q, G, h):
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    if name == "free":
        for b in range(OL.BATCH):
            g = P[b].astype(LD) @ v["exact_ld"][b] + q[b].astype(LD)
            assert float(np.abs(g).max()) <= 1e-13 * max(1.0, float(np.abs(q[b]).max()))

    def f64_slack(b):
        return DC.min_slack_qp(P[b], q[b], G[b], h[b])

    _conditions(f"dense QP {n} {m}", name, v, f32, nominal, solved, n, m,
                lambda U: h.astype(LD) - np.einsum("bij,bj->bi", G.astype(LD), U.astype(LD)),
                lambda b, U, lam: KC.certify_qp(P[b], q[b], G[b], h[b], U, lam), f64_slack)
