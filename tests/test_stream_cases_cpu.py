"""CPU tests: the inputs of tests/test_gpu_streams.py are worth launching. That test tells a launch that ran in stream order from
one that ran ahead of the copy queued in front of it by the plans it returns, so for every route of
stream_cases.ROUTES_UNDER_TEST the C oracle must, on the materialised problems (float32 routes: on the float32-rounded operands),

  * solve all nine B problems (A's matrices, bounds, goal and targets with x0_B),
  * find a binding row in at least six of them,
  * return plans that differ from A's, item by item, by at least ten times the bound the route's plans are held to:
    max |U_B - U_A| / max(1, max |U_A|) >= 1e-6 in float64, 1e-2 in float32;

the table covers every route of operand_layouts.ROUTES and the two on-chip routes for 17 .. 32 variables, the recorded t is the
first of stream_cases.TS that serves (routes that none serves say where their x0_B comes from instead), and the LDS sizes recorded
for the workgroup kernel are what the library says."""
import ctypes as C

import numpy as np
import pytest

import oracle

import operand_layouts as OL
import stream_cases as SC


def test_the_table_covers_every_route():
    assert set(SC.ROUTES_UNDER_TEST) == set(OL.ROUTES) | {SC.ON_CHIP_FUSED, SC.ON_CHIP_MODEL}
    assert len(SC.ROUTES_UNDER_TEST) == len(OL.ROUTES) + 2 == 26
    for name, r in OL.ROUTES.items():
        assert SC.ROUTES_UNDER_TEST[name] is r, name
    assert OL.pads_of(SC.LAYOUT) == OL.PADS and OL.PADS["x0"] > 0  # (a padded layout: x0 itself sits behind a padded stride)
    assert OL.LAYOUTS[SC.LAYOUT].get("x0", "b") == "b"
    assert "OPT_ON_CHIP_32" in SC.ROUTES_UNDER_TEST[SC.ON_CHIP_FUSED]["flags"]
    nx, nu, N, mk = SC.ROUTES_UNDER_TEST[SC.ON_CHIP_FUSED]["shape"]
    assert 17 <= N * nu <= 32 and N * mk <= 64 and N * nu == min(s[2] * s[1] for s, _, _ in SC.OC.SHAPES)
    nx, nu, N, mk = SC.ROUTES_UNDER_TEST[SC.ON_CHIP_MODEL]["shape"]
    assert 17 <= N * nu <= 32 and N * mk <= 64 and N * nu == min(s[2] * s[1] for s, _ in SC.MC.SHAPES)
    assert OL.model_pads(SC.MODEL_VARIANT)["x0"] > 0
    # every route says where its x0_B comes from, in exactly one way
    assert set(SC.T) | set(SC.SECOND_SEED) == set(SC.ROUTES_UNDER_TEST) and not set(SC.T) & set(SC.SECOND_SEED)
    for name, t in SC.T.items():
        assert t in SC.TS or t in SC.FINER, (name, t)


@pytest.mark.parametrize("route", list(SC.ROUTES_UNDER_TEST))
def test_x0_B_meets_the_conditions(route):
    a, b = SC.case_a(route)[0]["x0"], SC.x0_b(route)
    assert b.shape == a.shape == (OL.BATCH, SC.ROUTES_UNDER_TEST[route]["shape"][0])
    assert (np.abs(b - a).max(axis=1) > 0).all()
    if SC.ROUTES_UNDER_TEST[route]["f32"]:  # (what a float32 launch stores)
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64)) and np.array_equal(b, b.astype(np.float32).astype(np.float64))
    (_, full_a), (_, full_b) = SC.case_a(route), SC.case_b(route)
    for k in full_a:  # (only x0 differs)
        if k != "x0":
            assert full_a[k] is full_b[k] or np.array_equal(full_a[k], full_b[k]), k
    failed = SC.conditions(route)
    Ua, Ub = SC.reference(route, "A")[0], SC.reference(route, "B")[0]
    print(f"    {route}: x0_B from {'seed %d' % SC.SECOND_SEED[route] if route in SC.SECOND_SEED else 't = %g' % SC.T[route]}, "
          f"separation {SC.separation(Ua, Ub).min():.2e} .. {SC.separation(Ua, Ub).max():.2e} (needed {SC.SEPARATION * SC.bound(route):.0e})")
    assert not failed, failed


@pytest.mark.parametrize("route", list(SC.ROUTES_UNDER_TEST))
def test_the_recorded_t_is_the_first_that_serves(route):
    """every t of TS in front of the recorded one fails a condition; a route recorded outside TS fails them at all of TS"""
    recorded = SC.T.get(route)
    for t in SC.TS:
        if t == recorded:
            break
        assert SC.conditions(route, t), (route, t)
    if recorded in SC.FINER:
        # the value in front of it leaves a B problem infeasible, and then so does every larger one: the constraints are linear
        # in x0, so the t that keep a problem feasible are an interval around 0
        before = (SC.TS + SC.FINER)[len(SC.TS) + SC.FINER.index(recorded) - 1]
        assert any(f.startswith("B statuses") for f in SC.conditions(route, before)), (route, before)


@pytest.mark.parametrize("tag", list(SC.RECORDED))
def test_the_recorded_dense_plans_are_the_oracles(tag):
    """tests/golden/stream_dense_reference.npz, which the GPU tests read for the six dense HBM routes, against the oracle run here:
    statuses equal, plans within 1e-10 max(1, |u|) (the same C code on another machine; the routes are held to 1e-7 and 1e-3)"""
    name = SC.RECORDED[tag]
    for other in SC.DENSE:  # (every dense route reads one of the two records, and it is the record of its own problems)
        if SC.ROUTES_UNDER_TEST[other]["f32"] == (tag == "f32"):
            assert OL.route_case(other, SC.LAYOUT)[0] == OL.route_case(name, SC.LAYOUT)[0] and SC.T[other] == SC.T[name]
    for which in "AB":
        U, _, st = SC.reference(name, which)
        Ug, stg = SC.plan_reference(name, which)
        assert np.array_equal(st, stg) and Ug.shape == U.shape
        assert float((np.abs(Ug - U) / np.maximum(1.0, np.abs(U).max(axis=1, keepdims=True))).max()) <= 1e-10


SEARCHED = [r for r in SC.ROUTES_UNDER_TEST if r in SC.SECOND_SEED or (SC.T[r] in SC.FINER and r not in SC.DENSE)]


@pytest.mark.parametrize("route", SEARCHED)
def test_the_second_seed_is_the_first_that_serves_or_none_does(route):
    """the search behind the table, run again: a recorded second seed is the first of stream_cases.SEEDS whose x0 meets the
    conditions, and a route that went on to a finer t instead has no such seed among them (the dense HBM routes are not searched:
    stream_cases says why)"""
    assert SC.first_seed(route) == SC.SECOND_SEED.get(route)


def test_the_oracle_solves_the_sequences():
    """the stateful pairs run the problems of tests/test_gpu_memory_discipline.py: at least half solved, as its against_oracle asks"""
    from qpmpc_amd import _capi

    assert len(SC.SEQUENCES) == 2
    for name, seq in SC.SEQUENCES.items():
        w, B = OL.ltv(*seq["ltv"]), seq["ltv"][1]  # (the helper the GPU test states them with)
        st = oracle.solve_workload(w)[2]
        assert (st == 0).sum() * 2 >= B, (name, st)
        for step in (seq["first"], seq["second"]):
            assert all(hasattr(_capi, f) for f in step["flags"]) and (step["warm_start"] is None or hasattr(_capi, step["warm_start"]))
        assert seq["carried"] in ("ws", "warm") and (seq["carried"] == "warm") == seq["warm"]


def test_lds_shapes_are_one_instantiation_above_48_kib():
    pytest.importorskip("torch")
    from qpmpc_amd import _capi

    lib = _capi.load()
    assert len(SC.LDS_SHAPES) == 3 and len(set(SC.LDS_SHAPES.values())) == 3
    for shape, recorded in SC.LDS_SHAPES.items():
        nx, nu, N, mk = shape
        d, nbytes = _capi.Dims(nx, nu, N, mk, _capi.F64, 0, 1.0, 1.0, 0.1), C.c_size_t(0)
        assert lib.mpcqp_lds_bytes(C.byref(d), C.byref(nbytes)) == 0
        assert nbytes.value == recorded and SC.LDS_48K < recorded <= 160 * 1024, (shape, nbytes.value)
        assert N * nu > 32  # (dispatch_lds: one wavefront per problem up to n = 32 and m = 64, four beyond -- all three take four)
        w = SC.lds_case(shape)
        assert w["A"].shape[:2] == (OL.BATCH, N) and w["B"].shape[:2] == (OL.BATCH, N)  # (per step: the image mpcqp_lds_bytes prices)
        _, lam, st, _ = oracle.solve_workload(w)
        assert (st == 0).all() and (lam > 1e-9).any(axis=1).sum() >= SC.MIN_BINDING, (shape, st)
