"""CPU tests: the unit changes of tests/unit_changes.py are what they claim to be, so that a green tests/test_gpu_unit_changes.py
means something. For every distinct case behind the routes of tests/operand_layouts.py and every change of UC.CHANGES:

  (a) rescaling and then applying the inverse change returns the base problem's bits, and rescaling commutes bit for bit with the
      float32 rounding of operand_layouts.f32_view (every factor is a power of two);
  (b) every rescaled weight stays above the 1e-10 weight switch and every |e'| below the 1e29 padding sentinel;
  (c) the C oracle on the rescaled problem gives the base problem's statuses (all solved); its plan and multipliers mapped back
      are the base problem's bit for bit under the six scalar changes (with equal iteration counts) and within 1e-12 relative
      under `rows` and `mixed` (measured: <= 1e-13; the oracle's selection rule scales a row by 1 + |h|, so its path may differ).
      The (12, 4, 64, 16) shape costs about 18 s of oracle per solve and runs `cost+` and `rows` only;
  (d) the derivative laws of UC hold on the NumPy restatements of tests/*_np.py: the restatement on the rescaled problem, mapped
      back, is the restatement on the base problem to 1e-10 relative to the base result's largest entry."""
import numpy as np
import pytest

import oracle

import adjoint_model_np as AM
import adjoint_np as AN
import adjoint_stagewise_np as AS
import model_adjoint_np as MA
import operand_layouts as OL
import tangent_np as TN
import tangent_stagewise_np as TS
import unit_changes as UC
import verdict_cases as VC

CASES = [routes[0] for routes in VC.distinct_cases().values()]
DENSE_CHANGES = ("cost+", "rows")
SOLVES = [(route, change) for route in CASES for change in UC.CHANGES
          if OL.ROUTES[route]["shape"] != OL.DENSE or change in DENSE_CHANGES]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same_workload(a, b, what):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and _bits(v, b[k]), (what, k)
        else:
            assert v == b[k] and type(v) is type(b[k]), (what, k, v, b[k])


def test_the_changes():
    assert list(UC.CHANGES) == ["state+", "state-", "input+", "input-", "cost+", "cost-", "rows", "mixed"]
    assert UC.CHANGES["mixed"] == (-6, -8, -12, True) and UC.CHANGES["rows"] == (0, 0, 0, True)
    assert UC.SCALAR == ("state+", "state-", "input+", "input-", "cost+", "cost-")
    m = UC.maps_of("mixed", (OL.BATCH, 5, 3), 7)
    k = np.log2(m["r"])
    assert (k == np.round(k)).all() and k.min() >= -10 and k.max() <= 10 and len(np.unique(k)) > 10
    assert _bits(m["r"], UC.maps_of("rows", (OL.BATCH, 5, 3), 7)["r"]) and not _bits(m["r"], UC.maps_of("rows", (OL.BATCH, 5, 3), 8)["r"])
    assert len(CASES) == 17


def test_every_route_runs_at_least_five_changes():
    """the tables tests/test_gpu_unit_changes.py runs by: what is skipped, and where iteration counts may differ"""
    routes = list(OL.ROUTES)
    for route in routes:
        assert sum((route, c) not in UC.F32_SKIPS for c in UC.CHANGES) >= 5, route
    assert all(r in routes and c in UC.CHANGES and reason for (r, c), reason in UC.F32_SKIPS.items())
    assert all(OL.ROUTES[r]["f32"] and UC.CHANGES[c][1] != 0 for r, c in UC.F32_SKIPS) and len(UC.F32_SKIPS) == 4 * 3
    assert set(UC.F32_KERNELS) == {r for r in routes if OL.ROUTES[r]["f32"] and not r.startswith("promoted")}
    # an exemption from equal iteration counts is a case that runs, under a scalar change of the state or the input unit
    assert all(r in routes and c in UC.SCALAR and UC.CHANGES[c][2] == 0 and why for (r, c), why in UC.ITERS_MAY_DIFFER.items())
    assert not set(UC.ITERS_MAY_DIFFER) & set(UC.F32_SKIPS) and len(UC.ITERS_MAY_DIFFER) == 5 * 4 + 2


@pytest.mark.parametrize("change", UC.CHANGES)
@pytest.mark.parametrize("route", CASES)
def test_rescale_is_exact_and_stays_in_range(route, change):
    """(a) and (b)"""
    r = OL.ROUTES[route]
    _, (_, full) = OL.route_case(route, 0)
    scaled, maps = UC.rescale(full, change, r["seed"])
    _same_workload(UC.apply(scaled, UC.inverse(maps)), full, "rescale, then the inverse change")
    _same_workload(OL.f32_view(scaled), UC.apply(OL.f32_view(full), maps), "float32 rounding commutes")
    if r["f32"]:
        _same_workload(OL.f32_view(scaled), scaled, "a float32 case stays float32-representable")
    assert min(UC.weights(scaled)) > UC.WEIGHT_SWITCH, UC.weights(scaled)
    assert min(UC.weights(scaled)) >= 9.5e-9
    assert np.abs(scaled["e"]).max() < UC.SENTINEL and np.isfinite(scaled["e"]).all()
    for X in ("A", "B", "C", "D", "e", "x0", "goal", "targets"):
        if full[X] is not None:
            assert np.isfinite(scaled[X]).all() and ((scaled[X] == 0) == (full[X] == 0)).all(), X  # (nothing flushed to zero)
    if UC.CHANGES[change][3]:
        assert not (maps["r"] == maps["r"].flat[0]).all()


@pytest.mark.parametrize("route,change", SOLVES)
def test_oracle_maps_back(route, change):
    """(c)"""
    r = OL.ROUTES[route]
    _, (_, full) = OL.route_case(route, 0)
    U0, lam0, st0 = OL.oracle_on_full(route, 0)
    scaled, maps = UC.rescale(full, change, r["seed"])
    U, lam, st, it = oracle.solve_workload(scaled)
    assert (st0 == 0).all() and np.array_equal(st, st0), (st, st0)
    Ub, lb = UC.back_plan(U, maps), UC.back_multipliers(lam, maps)
    if change in UC.SCALAR:
        assert _bits(Ub, U0) and _bits(lb, lam0), (route, change, np.abs(Ub - U0).max(), np.abs(lb - lam0).max())
        if r["shape"] != OL.DENSE:  # (one more solve for the base counts: not at 18 s each)
            assert np.array_equal(it, oracle.solve_workload(full)[3])
    else:
        eu = float((np.abs(Ub - U0) / np.maximum(1.0, np.abs(U0).max(axis=1, keepdims=True))).max())
        el = float((np.abs(lb - lam0) / np.maximum(1.0, np.abs(lam0).max(axis=1, keepdims=True))).max())
        print(f"    {route}, {change}: plan {eu:.1e}, multipliers {el:.1e}")
        assert eu <= 1e-12 and el <= 1e-12, (route, change, eu, el)


# ---------------------------------------------------------------------------------------------- (d) the derivative laws
SHORT, LONG = (3, 2, 8, 2), (3, 2, 70, 2)
_BASE = {}


def _solved(name):
    """(full, U, lam, status) of a derivative case, solved once by the C oracle"""
    if name not in _BASE:
        full = OL.model_case(OL.MODEL_SHAPES[0], 0)[1] if name == "model" else OL.diff_case(name, 0)[1]
        _BASE[name] = (full,) + oracle.solve_workload(full)[:3]
    return _BASE[name]


def _close(got, want, what):
    got, want = np.asarray(got, dtype=float).ravel(), np.asarray(want, dtype=float).ravel()
    assert got.shape == want.shape, what
    if want.size:
        err, top = np.abs(got - want).max(), np.abs(want).max()
        assert err <= 1e-10 * top, (what, err, top)


LAWS = ["condensed", "model", "stagewise", "stagewise long", "shared model"]


@pytest.mark.parametrize("change", UC.CHANGES)
@pytest.mark.parametrize("kind", LAWS)
def test_gradient_law(kind, change):
    """adjoint_np.vjp, adjoint_model_np.model_vjp, adjoint_stagewise_np.stagewise_vjp (both horizons) and model_adjoint_np's
    NumpyModel.vjp: cotangents of the same scalar loss, gradients mapped back by UC.back_gradients"""
    name = "model" if kind == "shared model" else LONG if kind == "stagewise long" else SHORT
    full, U, lam, st = _solved(name)
    scaled, maps = UC.rescale(full, change, 77, shared_rows=kind == "shared model")
    Us, lams = U * maps["su"], lam * maps["sc"] / maps["r"].reshape(lam.shape)
    B, n = U.shape
    N, nx = int(full["N"]), full["x0"].shape[1]
    rng = np.random.default_rng(3)
    gU, gX = rng.standard_normal((B, n)), rng.standard_normal((B, (N + 1) * nx))
    gUs, gXs = UC.rescale_cotangents(gU, gX, maps)
    assert (st == 0).sum() >= 6 and (lam > 0).any(axis=1).sum() >= 5
    if kind == "shared model":
        base, other = MA.NumpyModel(full), MA.NumpyModel(scaled)
    for b in np.flatnonzero(st == 0):
        w1, w1s = AN.single(full, b), AN.single(scaled, b)
        if kind == "condensed":
            ref, got = AN.vjp(w1, lam[b], gU[b], gX[b]), AN.vjp(w1s, lams[b], gUs[b], gXs[b])
        elif kind == "model":
            ref, got = AM.model_vjp(w1, U[b], lam[b], gU[b], gX[b]), AM.model_vjp(w1s, Us[b], lams[b], gUs[b], gXs[b])
        elif kind == "shared model":
            ref, got = base.vjp(lam[b], gU[b], gX[b]), other.vjp(lams[b], gUs[b], gXs[b])
        else:
            ref = AS.stagewise_vjp(w1, lam[b], gU[b], gX[b], U[b])
            got = AS.stagewise_vjp(w1s, lams[b], gUs[b], gXs[b], Us[b])
            assert ref["status"] == 0 and got["status"] == 0
        back = UC.back_gradients({k: v for k, v in got.items() if k != "status"}, maps, b)
        assert set(back) >= {"x0"} and len(back) >= (6 if kind in ("model", "stagewise", "stagewise long") else 4)
        for key, v in back.items():
            _close(v, ref[key], (kind, change, b, key))


@pytest.mark.parametrize("change", UC.CHANGES)
@pytest.mark.parametrize("kind", ["condensed", "stagewise", "stagewise long", "shared model"])
def test_tangent_law(kind, change):
    """tangent_np.jvp, tangent_stagewise_np.stagewise_jvp (both horizons) and NumpyModel.jvp: tangents in the new units by
    UC.rescale_tangents, responses mapped back by UC.back_tangents"""
    name = "model" if kind == "shared model" else LONG if kind == "stagewise long" else SHORT
    full, U, lam, st = _solved(name)
    scaled, maps = UC.rescale(full, change, 77, shared_rows=kind == "shared model")
    lams = lam * maps["sc"] / maps["r"].reshape(lam.shape)
    rng = np.random.default_rng(4)
    if kind == "shared model":
        base, other = MA.NumpyModel(full), MA.NumpyModel(scaled)
    for b in np.flatnonzero(st == 0):
        w1, w1s = AN.single(full, b), AN.single(scaled, b)
        tan = TN.random_tangent(w1, rng)
        tans = UC.rescale_tangents(tan, maps, b)
        if kind == "condensed":
            ref, got = TN.jvp(w1, lam[b], tan), TN.jvp(w1s, lams[b], tans)
        elif kind == "shared model":
            ref, got = base.jvp(lam[b], tan), other.jvp(lams[b], tans)
        else:
            ref, got = TS.stagewise_jvp(w1, lam[b], tan), TS.stagewise_jvp(w1s, lams[b], tans)
        dU, dX = UC.back_tangents(got["U"], got["X"], maps)
        _close(dU, ref["U"], (kind, change, b, "dU"))
        _close(dX, ref["X"], (kind, change, b, "dX"))
