"""GPU tests (-m gpu): every kernel on problems stated in other units. A unit change (tests/unit_changes.py: states times sx,
inputs times su, cost times sc, every constraint row times its own r, all powers of two) is a symmetry of the MPC problem, so
the plan of the rescaled problem is known exactly from the base problem's: U' = su U, X' = sx X, lam' = sc lam / r, equal
statuses. The kernels hold absolute constants (selection tolerances, refinement thresholds, padding sentinels, float32
acceptance constants, reciprocal estimates) whose effect depends on the units; every other test draws operands of size about 1
and measures against max(1, |want|), so a plan in small units that is 1e-4 relative off would pass them all.

Here every result is mapped back to BASE units before it is measured, against the reference of the BASE problem:

  test_forward_route_change  every route of tests/operand_layouts.py x every change, 9 problems per launch in the guarded arena
                             (fill 0xFF) as tests/test_gpu_operand_layouts.py::test_forward_route_layout launches them: return
                             code 0, the oracle's statuses (all solved), |U'/su - U_oracle| / max(1, |U_oracle|) within the
                             route's bound (1e-7 float64, 1e-3 float32); under the six scalar changes, where the oracle maps back
                             bit for bit, also the iteration counts of the same route's launch of the base problem (a difference
                             means an absolute constant decided something; UC.ITERS_MAY_DIFFER lists the documented ones); and
                             where the KKT certificate passes on the base launch it passes on the mapped-back plan and multipliers.
  test_shared_model_change   mpcqp_solve_model_bounds_batch, two and four per wavefront, the same assertions.
  test_vjp_change, test_jvp_change, test_shared_model_derivatives_change
                             solve_mpc_batch_diff (condensed, model gradients, adjoint="stagewise"), plan_jvp (condensed and
                             formulation="stagewise") and SharedModel.solve_diff / plan_jvp on rescaled problems, mapped back by
                             the derivative laws of tests/unit_changes.py, against the NumPy restatements on the BASE problem at
                             the C oracle's BASE plan and multipliers, 1e-8 max(1, |want|) in base units.

tests/test_unit_changes_cpu.py shows that the rescaling is exact, that the C oracle maps back (bit for bit under the scalar
changes) and that the derivative laws hold on the restatements. The four true float32 kernels skip the changes of the input
unit (UC.F32_SKIPS): their contract is an absolute bound in the caller's input units.

With MPCQP_UNITS_REPORT=<path> a complete run writes the per-route table of profiles/unit_changes.txt."""
import os

import numpy as np
import pytest

import adjoint_model_np as AM
import adjoint_np as AN
import adjoint_stagewise_np as AS
import kkt_certificate as KC
import model_adjoint_np as MA
import operand_layouts as OL
import tangent_np as TN
import unit_changes as UC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers and comparisons; needs torch)
from guarded_launch import Forward, ModelCase, close  # noqa: E402
from guarded_launch import flags as _flags  # noqa: E402


F, F64, F32, I32, U8 = GL.F, GL.F64, GL.F32, GL.I32, GL.U8
ROUTES, CHANGES = list(OL.ROUTES), list(UC.CHANGES)
SOME = ("state-", "input+", "cost-", "mixed")  # the changes the shared-model and derivative tests run

F32_SKIPS = UC.F32_SKIPS  # (route, change) -> why it is not run (tests/test_unit_changes_cpu.py checks the table)

SEEN = {}  # (route, change) -> (worst base-unit error, iteration counts equal to the base launch's, certificates held / passed on base)
PASSED = set()  # the (route, change) cases whose every assertion held


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MPCQP_UNITS_REPORT")
    complete = all((r, c) in PASSED or (r, c) in F32_SKIPS for r in ROUTES for c in CHANGES)
    if path and complete:  # (a partial run, -k, or one with a failed case writes nothing)
        with open(path, "w") as fh:
            fh.write("tests/test_gpu_unit_changes.py::test_forward_route_change, 9 problems per launch, fill 0xFF. Per route and change:\n"
                     "worst |U'/su - U_oracle| / max(1, |U_oracle|) in BASE units against the oracle on the base problem (bound: 1e-7\n"
                     "float64, 1e-3 float32), then '=' if every iteration count equals the base launch's, else the number of items\n"
                     "whose count differs (asserted equal under the six scalar changes unless listed in UC.ITERS_MAY_DIFFER), then\n"
                     "certificates held / passed on the base launch (float64 routes). '-': not run (UC.F32_SKIPS).\n\n")
            fh.write(f"{'route':40s}" + "".join(f" {c:>18s}" for c in CHANGES) + "\n")
            for r in ROUTES:
                cells = []
                for c in CHANGES:
                    if (r, c) not in SEEN:
                        cells.append("-")
                        continue
                    err, differ, held, base = SEEN[(r, c)]
                    cells.append(f"{err:.1e} {'=' if differ == 0 else differ} {held}/{base}")
                fh.write(f"{r:40s}" + "".join(f" {c:>18s}" for c in cells) + "\n")


def _base_error(Uback, Uo):
    """max |U'/su - U_oracle| / max(1, |U_oracle|), per-problem scale, in base units"""
    return float((np.abs(Uback - Uo) / np.maximum(1.0, np.abs(Uo).max(axis=1, keepdims=True))).max())


def _certified(full, U, lam):
    return np.array([KC.certify(full, b, U[b], lam[b]).ok for b in range(len(U))])


# ---------------------------------------------------------------------------------------------- forward: route x change
_BASE = {}


def _launch(route, full):
    r = OL.ROUTES[route]
    case = Forward(full, dtype=F32 if r["f32"] else None, stagewise=r["stagewise"])
    assert case.B == OL.BATCH
    return case.run(F, _flags(r["flags"]))


def _base_launch(route):
    """the route's launch of the BASE problem (materialised, packed), once: its iteration counts and KKT certificates"""
    if route not in _BASE:
        _, (_, full) = OL.route_case(route, 0)
        out = _launch(route, full)
        assert (out["status"] == 0).all(), out["status"]
        cert = np.zeros(OL.BATCH, dtype=bool)
        if not OL.ROUTES[route]["f32"]:  # (float32 multipliers do not reach the certificate's 1e-9)
            cert = _certified(full, out["U"].astype(np.float64), out["lam"].astype(np.float64))
        _BASE[route] = (out, cert)
    return _BASE[route]


FORWARD = [(route, change) for route in ROUTES for change in CHANGES]


@pytest.mark.parametrize("route,change", [pytest.param(r, c, id=f"{r}-{c}") for r, c in FORWARD])
def test_forward_route_change(route, change):
    """One launch of the rescaled problem through the route, judged in base units against the base problem's oracle, the route's
    base launch and its certificates (module docstring). The float32 dense kernels missed 1e-3 under `rows` (2.7e-3 .. 4.6e-3)
    while their feasibility tolerance had an absolute term, tol (1 + |h_i|); it is tol (|G_i| + |h_i|) now (row_tol,
    csrc/mpcqp_internal.h)."""
    if (route, change) in F32_SKIPS:
        pytest.skip(F32_SKIPS[(route, change)])
    r = OL.ROUTES[route]
    key, (_, full) = OL.route_case(route, 0)
    scaled, maps = UC.rescale(full, change, r["seed"])
    Uo, _, sto = GL.oracle_of(repr(key), full)
    assert (sto == 0).all(), sto
    base, cert = _base_launch(route)
    out = _launch(route, scaled)
    Uback = UC.back_plan(out["U"], maps)
    err = _base_error(Uback, Uo)
    differ = int((out["iters"] != base["iters"]).sum())
    held = 0
    if cert.any():
        lback = UC.back_multipliers(out["lam"], maps)
        again = _certified(full, Uback, lback)
        held = int((again & cert).sum())
    SEEN[(route, change)] = (err if np.isfinite(err) else float("nan"), differ, held, int(cert.sum()))
    print(f"    {route}, {change}: status {out['status'].tolist()}, base-unit error {err:.2e}, iters {out['iters'].tolist()} "
          f"(base {base['iters'].tolist()}), certificates {held} of {int(cert.sum())}")
    assert np.array_equal(out["status"], sto), (out["status"], sto)
    assert not np.isnan(out["U"]).any()
    assert err <= (1e-3 if r["f32"] else 1e-7), err
    if change in UC.SCALAR:
        if (route, change) in UC.ITERS_MAY_DIFFER:
            assert differ > 0, "a stale entry of UC.ITERS_MAY_DIFFER"
        else:
            assert differ == 0, (out["iters"], base["iters"])
    if cert.any():
        bad = [(b, str(KC.certify(full, b, Uback[b], lback[b]))) for b in np.flatnonzero(cert & ~again)]
        assert not bad, bad
    PASSED.add((route, change))


# ---------------------------------------------------------------------------------------------- shared-model solves
def _model_solves(shape, w):
    """mpcqp_factor_model + mpcqp_solve_model_bounds_batch of the shared-model workload `w` (A, B, C, D with a leading 1; x0, goal,
    targets, e per problem), two and four per wavefront, as tests/test_gpu_operand_layouts.py::test_shared_model_solves sets
    them up (packed, the model factored in the arena): {flags: out}"""
    nx, nu, N, mk = shape
    for key, width in (("x0", nx), ("goal", nx), ("targets", N * nx), ("e", N * mk)):
        assert w[key].reshape(w[key].shape[0], -1).shape == (OL.BATCH, width)  # (every operand per problem)
    case = ModelCase(w, factor_in_arena=True)
    return {_flags([name]): case.run(F, _flags([name])) for name in ("OPT_TWO_PER_WAVE", "OPT_FOUR_PER_WAVE")}


def _shared(full):
    """the materialised problems of a shared-model case with A, B, C, D stored once"""
    w = dict(full)
    for X in ("A", "B", "C", "D"):
        assert (full[X] == full[X][:1]).all(), X
        w[X] = np.ascontiguousarray(full[X][:1])
    return w


_MODEL_BASE = {}


@pytest.mark.parametrize("change", SOME)
@pytest.mark.parametrize("shape", OL.MODEL_SHAPES)
def test_shared_model_change(shape, change):
    """Variant 0 of OL.model_case (x0, goal, targets and e per problem). Every problem shares C and D, so every problem gets the
    row factors of item 0."""
    _, full = OL.model_case(shape, 0)
    seed = 3000 + shape[0]
    scaled, maps = UC.rescale(full, change, seed, shared_rows=True)
    Uo, _, sto = GL.oracle_of(f"model {shape} 0", full)
    assert (sto == 0).all(), sto
    if shape not in _MODEL_BASE:
        _MODEL_BASE[shape] = _model_solves(shape, _shared(full))
    for flags, out in _model_solves(shape, _shared(scaled)).items():
        base = _MODEL_BASE[shape][flags]
        assert (base["status"] == 0).all()
        Uback, lback = UC.back_plan(out["U"], maps), UC.back_multipliers(out["lam"], maps)
        err = _base_error(Uback, Uo)
        differ = int((out["iters"] != base["iters"]).sum())
        cert = _certified(full, base["U"], base["lam"])
        again = _certified(full, Uback, lback)
        print(f"    model {shape}, {change}, flags {flags:#x}: status {out['status'].tolist()}, base-unit error {err:.2e}, iters "
              f"{out['iters'].tolist()} (base {base['iters'].tolist()}), certificates {int((again & cert).sum())} of {int(cert.sum())}")
        assert np.array_equal(out["status"], sto), out["status"]
        assert err <= 1e-7, err
        if change in UC.SCALAR:
            assert differ == 0, (out["iters"], base["iters"])
        assert not (cert & ~again).any(), [str(KC.certify(full, b, Uback[b], lback[b])) for b in np.flatnonzero(cert & ~again)]


# ---------------------------------------------------------------------------------------------- derivatives, public API
SHORT, LONG = OL.DIFF_SHAPES
_DIFF = {}


def _diff_base(name):
    """(full, U, lam, status) of a derivative case in BASE units: the plan and multipliers are the C oracle's"""
    if name not in _DIFF:
        full = OL.model_case(OL.MODEL_SHAPES[0], 0)[1] if name == "model" else OL.diff_case(name, 0)[1]
        _DIFF[name] = (full,) + GL.forward_on_cpu(full)
    return _DIFF[name]


def _leaf(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev).clone().requires_grad_()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _forward_holds(plan, maps, U0, st0):
    """statuses of the base problem, and the plan mapped back within 1e-7 of the oracle's base plan"""
    st = _np(plan.status).astype(np.int32)
    assert np.array_equal(st, st0), (st, st0)
    ok = st0 == 0
    assert ok.sum() * 2 >= len(st0)
    assert _base_error(UC.back_plan(_np(plan.U).reshape(U0.shape), maps)[ok], U0[ok]) <= 1e-7
    return ok


VJP = [("condensed", SHORT), ("model", SHORT), ("stagewise", SHORT), ("stagewise", LONG)]


@pytest.mark.parametrize("change", SOME)
@pytest.mark.parametrize("kind,shape", VJP)
def test_vjp_change(kind, shape, change):
    """solve_mpc_batch_diff on the rescaled problem, the cotangents of the same scalar loss (gU / su, gX / sx): every gradient
    mapped back by UC.back_gradients against adjoint_np.vjp, adjoint_model_np.model_vjp or adjoint_stagewise_np.stagewise_vjp on
    the base problem. The cost weights are shared by the batch: their gradient is the sum over the solved problems."""
    from qpmpc_amd import solve_mpc_batch_diff
    from qpmpc_amd import workloads as W

    full, U0, lam0, st0 = _diff_base(shape)
    scaled, maps = UC.rescale(full, change, 5000)
    bp = W.to_batch_problem(scaled)
    dev = bp.device
    B, n = U0.shape
    N, nx = int(full["N"]), full["x0"].shape[1]
    rng = np.random.default_rng(3)
    gU, gX = rng.standard_normal((B, n)), rng.standard_normal((B, (N + 1) * nx))
    gUs, gXs = UC.rescale_cotangents(gU, gX, maps)
    leaves = {k: _leaf(scaled[k], dev) for k in ("x0", "goal", "targets", "e")}
    kw = dict(initial_state=leaves["x0"], goal_state=leaves["goal"], target_states=leaves["targets"], ineq_vector=leaves["e"])
    if kind != "condensed":
        leaves.update({k: _leaf(scaled[k], dev) for k in ("A", "B", "C", "D", "wt", "wx", "wu")})
        kw.update(transition_state_matrix=leaves["A"], transition_input_matrix=leaves["B"], ineq_state_matrix=leaves["C"],
                  ineq_input_matrix=leaves["D"], terminal_cost_weight=leaves["wt"], stage_state_cost_weight=leaves["wx"],
                  stage_input_cost_weight=leaves["wu"])
    U, X, plan = solve_mpc_batch_diff(bp, states=True, adjoint="stagewise" if kind == "stagewise" else "condensed", **kw)
    loss = (U.reshape(B, -1) * torch.as_tensor(gUs, device=dev)).sum() + (X.reshape(B, -1) * torch.as_tensor(gXs, device=dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    ok = _forward_holds(plan, maps, U0, st0)
    vst = _np(plan.vjp_status).astype(np.int32)
    assert np.array_equal(vst, st0), (vst, st0)
    per = [k for k in leaves if k not in ("wt", "wx", "wu")]
    got = UC.back_gradients({k: _np(leaves[k].grad).reshape(B, -1) for k in per}, maps)
    wsum = np.zeros(3)
    for b in np.flatnonzero(ok):
        w1 = AN.single(full, b)
        if kind == "stagewise":
            ref = AS.stagewise_vjp(w1, lam0[b], gU[b], gX[b], U0[b])
            assert ref["status"] == 0
        else:
            ref = AN.vjp(w1, lam0[b], gU[b], gX[b])
            if kind == "model":
                ref.update({k: v for k, v in AM.model_vjp(w1, U0[b], lam0[b], gU[b], gX[b]).items() if k not in ref})
        for k in per:
            close(got[k][b], ref[k], (kind, shape, change, b, k))
        if kind != "condensed":
            wsum += ref["w"]
    for b in np.flatnonzero(~ok):
        assert all((got[k][b] == 0).all() for k in per), (b, "an unsolved item's gradients are zeros")
    if kind != "condensed":
        gw = UC.back_gradients(dict(w=np.array([float(leaves[k].grad) for k in ("wt", "wx", "wu")])), maps)["w"]
        close(gw, wsum, (kind, shape, change, "cost weights"))


JVP = [("condensed", SHORT), ("stagewise", SHORT), ("stagewise", LONG)]


@pytest.mark.parametrize("change", SOME)
@pytest.mark.parametrize("formulation,shape", JVP)
def test_jvp_change(formulation, shape, change):
    """plan_jvp on the rescaled problem with three tangents per problem stated in the new units (UC.rescale_tangents): dU and dX
    mapped back against tangent_np.jvp on the base problem."""
    from qpmpc_amd import plan_jvp, solve_mpc_batch
    from qpmpc_amd import workloads as W

    full, U0, lam0, st0 = _diff_base(shape)
    scaled, maps = UC.rescale(full, change, 5000)
    bp = W.to_batch_problem(scaled)
    dev = bp.device
    nx, nu, N, mk = shape
    B, T = OL.BATCH, 3
    rng = np.random.default_rng(4)
    tan = GL._tangents(full, B, T, rng, False)
    tans = UC.rescale_tangents(tan, maps)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    t = {k: torch.as_tensor(v, device=dev) for k, v in tans.items()}
    dU, dX = plan_jvp(bp, plan, initial_state=t["x0"], goal_state=t["goal"], target_states=t["targets"],
                      ineq_vector=t["e"].reshape(B, T, N, mk), states=True, formulation=formulation)
    torch.cuda.synchronize()
    ok = _forward_holds(plan, maps, U0, st0)
    jst = _np(plan.jvp_status).astype(np.int32)
    assert np.array_equal(jst, st0), (jst, st0)
    dU, dX = UC.back_tangents(_np(dU).reshape(B, T, -1), _np(dX).reshape(B, T, -1), maps)
    for b in np.flatnonzero(ok):
        w1 = AN.single(full, b)
        for j in range(T):
            ref = TN.jvp(w1, lam0[b], {k: v[b, j] for k, v in tan.items()})
            close(dU[b, j], ref["U"], (formulation, shape, change, b, j, "dU"))
            close(dX[b, j], ref["X"], (formulation, shape, change, b, j, "dX"))
    assert (dU[~ok] == 0).all() and (dX[~ok] == 0).all()


@pytest.mark.parametrize("change", SOME)
def test_shared_model_derivatives_change(change):
    """SharedModel.solve_diff (backward: mpcqp_model_vjp_batch) and SharedModel.plan_jvp (mpcqp_model_jvp_batch) on the rescaled
    shared-model case (3, 1, 16, 2) -- OL.diff_case has no shared model --, against model_adjoint_np.NumpyModel of the BASE model."""
    from qpmpc_amd import SharedModel
    from qpmpc_amd import workloads as W

    full, U0, lam0, st0 = _diff_base("model")
    scaled, maps = UC.rescale(full, change, 3003, shared_rows=True)
    bp = W.to_batch_problem(_shared(scaled))
    dev = bp.device
    sm = SharedModel(bp)
    ref_model = MA.NumpyModel(full)
    B, n = U0.shape
    N, nx = int(full["N"]), full["x0"].shape[1]
    mk = full["e"].shape[-1]
    rng = np.random.default_rng(5)
    gU, gX = rng.standard_normal((B, n)), rng.standard_normal((B, (N + 1) * nx))
    gUs, gXs = UC.rescale_cotangents(gU, gX, maps)
    leaves = {k: _leaf(scaled[k], dev) for k in ("x0", "goal", "targets", "e")}
    U, X, plan = sm.solve_diff(leaves["x0"], leaves["goal"], leaves["targets"], ineq_vector=leaves["e"], states=True)
    loss = (U.reshape(B, -1) * torch.as_tensor(gUs, device=dev)).sum() + (X.reshape(B, -1) * torch.as_tensor(gXs, device=dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    ok = _forward_holds(plan, maps, U0, st0)
    assert ok.all() and (_np(plan.vjp_status) == 0).all()
    got = UC.back_gradients({k: _np(v.grad).reshape(B, -1) for k, v in leaves.items()}, maps)
    T = 3
    tan = GL._tangents(full, B, T, rng, False)
    t = {k: torch.as_tensor(v, device=dev) for k, v in UC.rescale_tangents(tan, maps).items()}
    dU, dX = sm.plan_jvp(plan, initial_state=t["x0"], goal_state=t["goal"], target_states=t["targets"],
                         ineq_vector=t["e"].reshape(B, T, N, mk), states=True)
    torch.cuda.synchronize()
    assert (_np(plan.jvp_status) == 0).all()
    dU, dX = UC.back_tangents(_np(dU).reshape(B, T, -1), _np(dX).reshape(B, T, -1), maps)
    for b in range(B):
        ref = ref_model.vjp(lam0[b], gU[b], gX[b])
        for k in leaves:
            close(got[k][b], ref[k], ("shared model", change, b, k))
        for j in range(T):
            rj = ref_model.jvp(lam0[b], {k: v[b, j] for k, v in tan.items()})
            close(dU[b, j], rj["U"], ("shared model", change, b, j, "dU"))
            close(dX[b, j], rj["X"], ("shared model", change, b, j, "dX"))
