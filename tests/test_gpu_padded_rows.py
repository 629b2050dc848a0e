"""GPU tests (-m gpu): the padded-row contract of include/mpcqp.h (MpcqpDims), route by route. A problem whose row count varies
per step is padded by the host to mk rows with C = D = 0 and e = 1e30, "an inequality that can never be active"; every solver
kernel keeps that promise on its own (a row whose bound is at least 1e29 is never a candidate, a zero row's norm is not divided
by), and MpcqpSolveOpts.warm_shift adds that stored ids which name a padded row are dropped.

tests/padded_rows.py holds the cases -- nine problems per route of tests/operand_layouts.py (and the on-chip routes for 17 .. 32
variables), padded in three placements: `tail` (what BatchMPCProblem.from_problems makes), `mixed` (a random quarter, a whole
step, the head of a step, a whole problem) and `rows` (a zero row in a shared, time-invariant constraint block) --, and
tests/test_padded_rows_cpu.py shows on the C oracle that they mean something: most items have a binding real row, and the
padding moves most plans by ten times the bound they are held to.

The reference is always the STRIPPED problem (padded rows deleted from the condensed G and h, oracle.capi.gi_solve), never the
padded one: statuses equal, U within the route's existing bound (1e-7 float64, 1e-3 float32, relative to max(1, |U|)), no NaN,
lam == 0 on every padded row, and for an item padded whole iters == 0 and the plan within the bound of -P^-1 q. Every launch
runs in the guarded arena of tests/guarded_launch.py under the all-0xFF fill. Multipliers on REAL rows are not
compared here (the verdict and parity tests hold statuses and plans; that is the existing contract)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import model_adjoint_np as MN
import operand_layouts as OL
import padded_rows as PR
from golden_util import load_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers and comparisons; needs torch)
from guarded_launch import Forward, ModelCase, QPs  # noqa: E402
from guarded_launch import flags as _flags  # noqa: E402

F, F32 = GL.F, GL.F32
B = PR.BATCH


def held(c, out, what):
    """the assertions of this file on the outputs of one launch of case `c`; returns the worst relative error of the plans"""
    Uo, lamo, sto, _ = PR.reference(c)
    assert (sto == 0).all()
    U = out["U"].astype(np.float64)
    err = float(PR.rel(U, Uo).max()) if not np.isnan(U).any() else float("nan")
    print(f"    {what}: status {out['status'].tolist()}, max rel err vs the stripped reference {err:.2e}")
    assert np.array_equal(out["status"], sto), (what, out["status"], sto)
    assert not np.isnan(U).any(), (what, "NaN in U")
    assert err <= c["bound"], (what, err)
    if "lam" in out and out["lam"] is not None:
        lam = out["lam"].reshape(B, -1)
        assert not np.isnan(lam).any(), (what, "NaN in lam")
        assert (lam[c["mask"]] == 0).all(), (what, "a padded row has a multiplier", np.argwhere((lam != 0) & c["mask"])[:4])
    for b in np.flatnonzero(c["mask"].all(axis=1)):  # an item padded whole is unconstrained
        assert out["iters"][b] == 0, (what, b, out["iters"][b])
        free = PR.unconstrained(c, b)
        assert np.abs(U[b] - free).max() <= c["bound"] * max(1.0, np.abs(free).max()), (what, b)
    return err


# ---------------------------------------------------------------------------------------------- 1. forward: route x placement
WORST = {}  # (route, placement) -> (items compared, statuses, worst relative error)
QP_MODE = "on-chip 32 QP mode"


@pytest.fixture(scope="module", autouse=True)
def _report():
    """With MPCQP_PADDED_REPORT=<path> the forward cases' worst errors are written there (profiles/padded_rows.md)."""
    yield
    path = os.environ.get("MPCQP_PADDED_REPORT")
    names = list(PR.ROUTES) + [f"{QP_MODE} {PR.ROUTES[n]['shape']}" for n in PR.ON_CHIP_FUSED]
    models = [(_model_name(shape, flag, bounds), shape, variant) for shape, variant in PR.MODEL_CASES
              for flag, bounds in _model_launches(shape, variant)]
    complete = (set(WORST) == {(n, p) for n in names for p in PR.PLACEMENTS}
                and set(MODEL_WORST) == {k + (p,) for k in models for p in PR.PLACEMENTS})
    if path and complete:  # (a partial run, -k, writes nothing)
        with open(path, "w") as fh:
            fh.write("# Padded rows: every forward route and shared-model solve against the stripped reference\n\n"
                     "`tests/test_gpu_padded_rows.py::test_forward_route_placement`, `::test_on_chip_qp_mode` and\n"
                     "`::test_shared_model_solves`, 9 problems per launch, fill 0xFF. Worst max |u - u_ref| / max(1, |u_ref|) against\n"
                     "the stripped reference of `tests/padded_rows.py` (padded rows deleted, `oracle.capi.gi_solve`); bound 1e-7 in\n"
                     "float64, 1e-3 in float32 against the float32-rounded operands. Statuses: MPCQP_* codes of the nine items\n"
                     "(0: solved). The stateful launches, the derivative exports and the Python layer are held to the same\n"
                     "reference by the other tests of that file.\n\n"
                     "## Forward routes (fused build and solve; the QP mode on the condensed problem)\n\n"
                     "| route | shape | placement | items | statuses | worst error |\n|---|---|---|---|---|---|\n")
            for n in names:
                shape = PR.ROUTES[n]["shape"] if n in PR.ROUTES else n[len(QP_MODE) + 1:]
                for p in PR.PLACEMENTS:
                    items, st, err = WORST[(n, p)]
                    fh.write(f"| {n} | {shape} | {p} | {items} | {' '.join(str(s) for s in st)} | {err:.2e} |\n")
            fh.write("\n## Shared-model solves, the padded rows in the model\n\n"
                     "`mixed` in the form a shared constraint block can express: step N // 2 padded whole and row 0 of step 0, the same\n"
                     "for every problem (a random quarter per problem and a problem padded whole cannot exist in a shared model).\n"
                     "Variant: `operand_layouts.MODEL_VARIANTS` (1: everything per problem, padded strides; 3: e shared).\n\n"
                     "| launch | shape | variant | placement | items | statuses | worst error |\n|---|---|---|---|---|---|---|\n")
            for name, shape, variant in models:
                for p in PR.PLACEMENTS:
                    items, st, err = MODEL_WORST[(name, shape, variant, p)]
                    fh.write(f"| {name} | {shape} | {variant} | {p} | {items} | {' '.join(str(s) for s in st)} | {err:.2e} |\n")


FORWARD = [(name, placement) for name in PR.ROUTES for placement in PR.PLACEMENTS]


@pytest.mark.parametrize("name,placement", FORWARD, ids=[f"{n}-{p}" for n, p in FORWARD])
def test_forward_route_placement(name, placement):
    """One launch of the padded case through the route (the flags and entry point of tests/test_gpu_operand_layouts.py; the
    on-chip routes flagged MPCQP_OPT_ON_CHIP_32 and without a workspace): return code 0, guards intact, operands unchanged
    (Launch.run), and held()."""
    r = PR.ROUTES[name]
    c = PR.case(name, placement)
    if name in PR.ON_CHIP_FUSED:
        case = Forward(c["w"], workspace=False)
    else:
        case = Forward(c["w"], dtype=F32 if r["f32"] else None, stagewise=r["stagewise"])
    assert case.B == B
    out = case.run(F, _flags(r["flags"]))
    WORST[(name, placement)] = (B, out["status"].tolist(), float(PR.rel(out["U"].astype(np.float64), PR.reference(c)[0]).max()))
    held(c, out, f"{name}, {placement}")


@pytest.mark.parametrize("placement", PR.PLACEMENTS)
@pytest.mark.parametrize("name", PR.ON_CHIP_FUSED)
def test_on_chip_qp_mode(name, placement):
    """mpcqp_solve_batch flagged MPCQP_OPT_ON_CHIP_32 (the QP mode of mpcqp_duo.hip) on the CONDENSED padded problems of the
    on-chip cases: zero rows of G with h = 1e30."""
    c = PR.case(name, placement)
    refs = GL.condense_refs(c["full"], B)
    P, q, G, h = (np.stack([getattr(cq, k) for cq in refs]) for k in ("P", "q", "G", "h"))
    assert not G[c["mask"]].any() and (h[c["mask"]] == PR.PAD).all()
    out = QPs(P, q, G, h).run(F, _flags(["OPT_ON_CHIP_32"]))
    what = f"{QP_MODE} {c['shape']}"
    WORST[(what, placement)] = (B, out["status"].tolist(), float(PR.rel(out["U"], PR.reference(c)[0]).max()))
    held(c, out, f"{what}, {placement}")


# ---------------------------------------------------------------------------------------------- 2. shared-model solves
MODEL_WORST = {}  # (launch, shape, variant, placement) -> (items compared, statuses, worst relative error)


def _model_launches(shape, variant):
    """(flag, with bounds of the launch's own) of the launches of a shared-model case"""
    shares_e = OL.MODEL_VARIANTS[variant]["e"] == "1"
    if shape[1] * shape[2] <= 16:
        launches = [(flag, True) for flag in ("OPT_TWO_PER_WAVE", "OPT_FOUR_PER_WAVE")]
        if shares_e:
            launches += [(flag, False) for flag in ("OPT_TWO_PER_WAVE", "OPT_FOUR_PER_WAVE", "OPT_ONE_PER_WAVE", "OPT_FORCE_LDS")]
        return launches
    return [(None, True), ("OPT_ON_CHIP_32", True)] + ([("OPT_ON_CHIP_32", False)] if shares_e else [])


def _model_name(shape, flag, bounds):
    kernel = "on-chip 32 MODEL mode" if shape[1] * shape[2] > 16 else "shared model"
    return f"{kernel}, {flag or 'no flag'}, " + ("bounds per launch" if bounds else "the model's e")


@pytest.mark.parametrize("placement", PR.PLACEMENTS)
@pytest.mark.parametrize("shape,variant", PR.MODEL_CASES)
def test_shared_model_solves(shape, variant, placement):
    """mpcqp_solve_model_bounds_batch (e per problem or shared, 1e30 on the padded rows) and mpcqp_solve_model_batch (the model's
    own e, where the variant shares it) with padded rows IN THE MODEL, in the three placements (`mixed` in the form a shared
    block can express: a step padded whole and the head row of a step). Up to 16 variables: two and four per wavefront, both
    exports; MPCQP_OPT_ONE_PER_WAVE and MPCQP_OPT_FORCE_LDS on the export without bounds (with bounds of their own the
    small-problem kernels serve the launch whatever those flags say). (3, 1, 24, 2): the MODEL mode of mpcqp_duo.hip, which
    the export with bounds takes with and without MPCQP_OPT_ON_CHIP_32 and the other one with it."""
    c = PR.model_case(shape, variant, placement)
    case = ModelCase(c["w"], OL.model_pads(variant))
    assert case.B == B
    for flag, bounds in _model_launches(shape, variant):
        out = case.run(F, _flags([flag] if flag else []), bounds=bounds)
        key = (_model_name(shape, flag, bounds), shape, variant, placement)
        MODEL_WORST[key] = (B, out["status"].tolist(), float(PR.rel(out["U"], PR.reference(c)[0]).max()))
        held(c, out, f"{key[0]} {shape} variant {variant}, {placement}")


# ---------------------------------------------------------------------------------------------- 3. stateful launches
def _reload(case, w):
    """the next runs of `case` load the operands of workload `w` (same shapes, same layout) instead of its own"""
    from qpmpc_amd import workloads as W

    bp = W.to_batch_problem(w)
    for name, attr in GL.OPS:
        t = getattr(bp, attr)
        if t is not None:
            spec = next(s for s in case.L.specs if s["name"] == "op_" + name)
            rows = t.reshape(t.shape[0], -1).contiguous()
            assert rows.shape == spec["rows"].shape and rows.dtype == spec["rows"].dtype
            spec["rows"] = rows


def _own_record_needs_no_iteration(c, cold, again, what):
    """shows that a warm launch CONSUMES the record (one that quietly ran cold would pass every comparison with the reference):
    started from the record of its own solution a launch needs no iteration -- the contract
    tests/test_gpu_warm_start.py::test_warm_start_from_own_solution_needs_no_iteration and
    ::test_stage_kernel_warm_start_same_plans_fewer_sweeps_less_time hold on unpadded problems --, where the cold launch, which
    begins from the empty set, iterated on every item that has a binding row"""
    binding = (PR.reference(c)[1] > 1e-9).any(axis=1)
    assert binding.sum() >= PR.MIN_ITEMS and (cold["iters"][binding] >= 1).all(), (what, cold["iters"], binding)
    assert (again["iters"] == 0).all(), (what, again["iters"])


def _stored_ids(out, kind):
    """per problem, the row ids of the warm record a launch left: "pair" (the operator, 16 x 16 doubles, then int32 ids, -1 for
    an empty slot) or "stagew" (int32 count, then the ids), as qpmpc_amd.batch.WarmState.active_set reads them"""
    rec = out["warm"].reshape(B, -1)
    if kind == "pair":
        ids = np.ascontiguousarray(rec[:, 16 * 16 * 8:]).view(np.int32)
        return [set(int(i) for i in row if i >= 0) for row in ids]
    ints = np.ascontiguousarray(rec).view(np.int32)
    return [set(int(i) for i in row[1:1 + max(0, int(row[0]))]) for row in ints]


def _record_names_real_rows(c, out, kind, what):
    """the record of a launch on case `c` holds every binding row of the stripped reference and no padded row"""
    lam = PR.reference(c)[1]
    for b, ids in enumerate(_stored_ids(out, kind)):
        assert set(np.flatnonzero(lam[b] > 1e-9)) <= ids, (what, b, "a binding row is not in the record")
        assert not any(c["mask"][b, i] for i in ids), (what, b, "the record names a padded row", sorted(ids))


@pytest.mark.parametrize("name", ["small", "pair generic"])
def test_small_kernel_warm_operator(name):
    """The small-problem kernel, a `tail` problem: a cold launch with a warm state, then MPCQP_WARM_OPERATOR on the same matrices
    and bounds with new initial states -- the warm launch held to the stripped reference of ITS problem."""
    from qpmpc_amd import _capi

    first, second = PR.warm_pair(name, "operator")
    case = Forward(first["w"], warm=True)
    cold = case.run(F)
    held(first, cold, f"{name}: cold launch with a warm state")
    again = case.run(F, warm_start=_capi.WARM_OPERATOR, keep=("warm",))
    held(first, again, f"{name}: MPCQP_WARM_OPERATOR on the same problem")
    _own_record_needs_no_iteration(first, cold, again, name)
    _reload(case, second["w"])
    held(second, case.run(F, warm_start=_capi.WARM_OPERATOR, keep=("warm",)), f"{name}: MPCQP_WARM_OPERATOR, new x0")


@pytest.mark.parametrize("name", ["small", "pair generic"])
def test_small_kernel_warm_active_set_shifted_onto_padding(name):
    """The small-problem kernel: a cold launch, then MPCQP_WARM_ACTIVE_SET with warm_shift = mk on a second `tail` problem. Most
    stored ids, moved down by mk, name a padded row of the second problem (tests/test_padded_rows_cpu.py::test_warm_pairs):
    the header says they are dropped."""
    from qpmpc_amd import _capi

    first, second = PR.warm_pair(name, "active_set")
    mk = first["shape"][3]
    case = Forward(first["w"], warm=True)
    cold = case.run(F)
    held(first, cold, f"{name}: cold launch with a warm state")
    _record_names_real_rows(first, cold, "pair", f"{name}: the cold launch's record")
    _reload(case, second["w"])
    warm = case.run(F, warm_start=_capi.WARM_ACTIVE_SET, keep=("warm",), warm_shift=mk)
    held(second, warm, f"{name}: MPCQP_WARM_ACTIVE_SET, warm_shift {mk}")
    _record_names_real_rows(second, warm, "pair", f"{name}: the warm launch's record")


def test_narrow_stagewise_keep_then_reuse_factor_with_a_warm_start():
    """mpcqp_stage.hip at (3, 1, 24, 2), a `tail` problem: MPCQP_OPT_KEEP_FACTOR with a warm state, then MPCQP_OPT_REUSE_FACTOR
    and a warm start from the record on the same matrices with new initial states."""
    from qpmpc_amd import _capi

    first, second = PR.warm_pair("narrow", "operator")
    case = Forward(first["w"], warm=True)
    cold = case.run(F, _capi.OPT_KEEP_FACTOR)
    held(first, cold, "narrow: KEEP_FACTOR")
    again = case.run(F, _capi.OPT_REUSE_FACTOR, warm_start=_capi.WARM_OPERATOR, keep=("ws", "warm"))
    held(first, again, "narrow: REUSE_FACTOR, warm start on the same problem")
    _own_record_needs_no_iteration(first, cold, again, "narrow")
    _reload(case, second["w"])
    held(second, case.run(F, _capi.OPT_REUSE_FACTOR, warm_start=_capi.WARM_OPERATOR, keep=("ws", "warm")),
         "narrow: REUSE_FACTOR, warm start, new x0")


def test_wide_stagewise_active_set_record_shifted_onto_padding():
    """mpcqp_stagew.hip at (6, 2, 20, 3): a cold launch writes the active rows' ids, then MPCQP_WARM_ACTIVE_SET with
    warm_shift = mk on a second `tail` problem, where most of the moved ids name padded rows."""
    from qpmpc_amd import _capi

    first, second = PR.warm_pair("wide", "active_set")
    mk = first["shape"][3]
    case = Forward(first["w"], warm=True)
    cold = case.run(F)
    held(first, cold, "wide: cold launch with a warm state")
    _record_names_real_rows(first, cold, "stagew", "wide: the cold launch's record")
    _reload(case, second["w"])
    warm = case.run(F, warm_start=_capi.WARM_ACTIVE_SET, keep=("warm",), warm_shift=mk)
    held(second, warm, f"wide: MPCQP_WARM_ACTIVE_SET, warm_shift {mk}")
    _record_names_real_rows(second, warm, "stagew", "wide: the warm launch's record")


def test_pairing_order_on_a_mixed_batch():
    """A pairing order on the `mixed` batch of the lean pair kernel. What a problem's bits may depend on, by mpcqp_pair.hip: the
    half of the wavefront it sits in (the halves sum in different orders) and its PARTNER -- the refinement step after the
    iterations is taken by the whole wavefront when either half's active residuals ask for it ("in both halves", at
    REFTOL = 1e-11), so a problem next to another partner may be refined where it was not; the header promises plans equal to
    rounding for that. An order that moves whole wavefronts -- pairs (0, 1) <-> (2, 3), (4, 5) <-> (6, 7), the unconstrained
    problem 7 with them -- keeps every problem's half and partner: every output is bitwise the natural order's. The reversal
    keeps the halves (i and 8 - i have the same parity) and changes the partners: statuses and iteration counts equal, plans
    equal to 1e-9 (guarded_launch.same_plans)."""
    c = PR.case("pair lean", "mixed")
    natural = Forward(c["w"]).run(F)
    held(c, natural, "pair lean, mixed, natural order")
    moved = Forward(c["w"], order=[2, 3, 0, 1, 6, 7, 4, 5, 8]).run(F)
    held(c, moved, "pair lean, mixed, wavefronts exchanged")
    GL.equal_outputs(natural, moved, "a pairing order that moves whole wavefronts")
    reversed_ = Forward(c["w"], order=np.arange(B)[::-1].copy()).run(F)
    held(c, reversed_, "pair lean, mixed, reversed order")
    GL.same_plans(natural, reversed_, "a pairing order that changes the partners")
    assert np.array_equal(natural["iters"], reversed_["iters"])


# ---------------------------------------------------------------------------------------------- 4. derivative exports
_DIFF = {}


def _diff(shape):
    """(case, (w, full, U, lam, status)) of a derivative case: plan and multipliers are the STRIPPED reference's, so the active
    set the exports see has no padded row in it"""
    if shape not in _DIFF:
        c = PR.diff_case(shape)
        U, lam, st, _ = PR.reference(c)
        _DIFF[shape] = (c, (c["w"], c["full"], U, lam, st.astype(np.int32)))
    return _DIFF[shape]


@pytest.mark.parametrize("kind,shape", [("condensed", (3, 2, 8, 2)), ("model", (3, 2, 8, 2)), ("stagewise", (3, 2, 70, 2))])
def test_plan_vjp_on_a_tail_case(kind, shape):
    """mpcqp_plan_vjp_batch / _vjp_model_batch / _vjp_stagewise_batch: every gradient against the NumPy restatement on the
    materialised (padded) problem at 1e-8 (guarded_launch.plan_vjp), and the gradients with respect to e, C and D
    exactly 0 on the padded rows."""
    nx, nu, N, mk = shape
    c, case = _diff(shape)
    g, vst = GL.plan_vjp(kind, shape, case, 0, "padded tail")
    assert (vst == 0).all()
    assert (g["e"][c["mask"]] == 0).all()
    for X in ("C", "D"):
        if X in g:
            assert (g[X].reshape(B, N * mk, -1)[c["mask"]] == 0).all(), X


@pytest.mark.parametrize("model,stagewise,shape", [(False, False, (3, 2, 8, 2)), (True, False, (3, 2, 8, 2)),
                                                  (False, True, (3, 2, 70, 2)), (True, True, (3, 2, 70, 2))])
def test_plan_jvp_on_a_tail_case(model, stagewise, shape):
    """mpcqp_plan_jvp_batch / _jvp_model_batch / _jvp_stagewise_batch / _jvp_model_stagewise_batch: three random tangents
    against the NumPy restatement at 1e-8 (guarded_launch.plan_jvp); then tangents that are non-zero only on padded
    rows of e (and of C and D): dU = dX = 0."""
    nx, nu, N, mk = shape
    c, case = _diff(shape)
    GL.plan_jvp(model, stagewise, shape, case, 0, "padded tail")
    tan = GL._tangents(c["full"], B, 3, np.random.default_rng(6), model)
    for X in ("x0", "goal", "targets", "A", "B", "w"):
        if X in tan:
            tan[X][...] = 0.0
    for X in ("e", "C", "D"):
        if X in tan:
            rows = tan[X].reshape(B, 3, N * mk, -1)
            rows[np.broadcast_to(~c["mask"][:, None, :], rows.shape[:3])] = 0.0
            assert np.abs(rows).max() > 0
    dU, dX, vst = GL.plan_jvp(model, stagewise, shape, case, 0, "padded tail, tangents on padded rows only", tan=tan)
    assert (vst == 0).all() and (dU == 0).all() and (dX == 0).all()


def test_shared_model_derivatives_with_padded_rows_in_the_model():
    """mpcqp_model_vjp_batch and mpcqp_model_jvp_batch at (3, 2, 8, 2), the `tail` rows in the shared model: against
    tests/model_adjoint_np.py at 1e-8 with the stripped reference's multipliers; g_e exactly 0 on padded rows, and a tangent
    on padded rows of e alone gives dU = dX = 0."""
    from qpmpc_amd import SharedModel, model_diff
    from qpmpc_amd import workloads as W

    c = PR.model_case(PR.MODEL_DIFF_SHAPE, PR.DIFF_VARIANT)
    nx, nu, N, mk = c["shape"]
    U, lam, st, _ = PR.reference(c)
    assert (st == 0).all()
    ref = MN.NumpyModel(c["w"])
    sm = SharedModel(W.to_batch_problem(c["w"]))
    dev = sm.template.device
    plan = SimpleNamespace(U=torch.as_tensor(U, device=dev), multipliers=torch.as_tensor(lam, device=dev),
                           status=torch.as_tensor(st.astype(np.int32), device=dev))
    rng = np.random.default_rng(7)
    gU, gX = rng.standard_normal((B, N * nu)), rng.standard_normal((B, (N + 1) * nx))
    g = model_diff.model_vjp(sm, plan, torch.as_tensor(gU, device=dev), torch.as_tensor(gX, device=dev), {"goal", "targets", "e"})
    torch.cuda.synchronize()
    g = dict(zip(("x0", "goal", "targets", "e"), [v.reshape(B, -1).cpu().numpy() for v in g]))
    assert (plan.vjp_status.cpu().numpy() == 0).all()
    tan = dict(x0=rng.standard_normal((B, 3, nx)), goal=rng.standard_normal((B, 3, nx)),
               targets=rng.standard_normal((B, 3, N * nx)), e=rng.standard_normal((B, 3, N, mk)))
    only = dict(e=tan["e"].copy())
    only["e"].reshape(B, 3, N * mk)[np.broadcast_to(~c["mask"][:, None, :], (B, 3, N * mk))] = 0.0
    names = dict(x0="initial_state", goal="goal_state", targets="target_states", e="ineq_vector")
    runs = []
    for t in (tan, only):
        dU, dX = model_diff.model_jvp(sm, plan, states=True, **{names[k]: torch.as_tensor(v, device=dev) for k, v in t.items()})
        torch.cuda.synchronize()
        assert (plan.jvp_status.cpu().numpy() == 0).all()
        runs.append((dU.reshape(B, 3, -1).cpu().numpy(), dX.reshape(B, 3, -1).cpu().numpy()))
    for b in range(B):
        want = ref.vjp(lam[b], gU[b], gX[b])
        for key in ("x0", "goal", "targets", "e"):
            GL.close(g[key][b], want[key], (b, key))
        for t in range(3):
            rj = ref.jvp(lam[b], {k: v[b, t] for k, v in tan.items()})
            GL.close(runs[0][0][b, t], rj["U"], (b, t, "dU"))
            GL.close(runs[0][1][b, t], rj["X"], (b, t, "dX"))
    assert (g["e"][c["mask"]] == 0).all()
    assert np.abs(only["e"]).max() > 0 and (runs[1][0] == 0).all() and (runs[1][1] == 0).all()


# ---------------------------------------------------------------------------------------------- 5. the Python layer
def test_solve_mpc_on_the_ragged_fixture():
    """solve_mpc on tests/golden/random_ltv_ragged.npz (per-step lists of 1, 2, 3, 4, 1, 2, 3 rows, recorded from the reference):
    the plan equals the recorded U_star at 1e-6, and the multipliers it returns are those of the real rows -- lam[valid_rows] of
    the padded launch it stands for, none of them on a padded row."""
    from qpmpc_amd import BatchMPCProblem, solve_mpc, solve_mpc_batch

    problem, z = load_case("random_ltv_ragged")
    plan = solve_mpc(problem, solver="hip_gi")
    assert not plan.is_empty
    Ustar = np.asarray(z["U_star"]).ravel()
    assert np.abs(plan.inputs.ravel() - Ustar).max() <= 1e-6 * max(1.0, np.abs(Ustar).max())
    bp = BatchMPCProblem.from_problems([problem])
    batch = solve_mpc_batch(bp, return_multipliers=True)
    torch.cuda.synchronize()
    lam = batch.multipliers[0].cpu().numpy()
    padded = np.ones(lam.shape, dtype=bool)
    padded[bp.valid_rows] = False
    assert padded.any() and (lam[padded] == 0).all() and not np.isnan(lam).any()
    got = np.asarray(plan.qpsol.z)
    assert got.shape == (len(bp.valid_rows),) == (z["out_G"].shape[0],)
    assert np.array_equal(got, lam[bp.valid_rows])


def _plan_out(plan):
    torch.cuda.synchronize()
    return dict(U=plan.U.cpu().numpy(), lam=plan.multipliers.cpu().numpy(), status=plan.status.cpu().numpy(),
                iters=plan.iters.cpu().numpy())


def test_ragged_batches_through_the_python_layer():
    """BatchMPCProblem.from_problems on ragged host problems (tests/test_padded_rows_cpu.py: it makes the `tail` case), through
    solve_mpc_batch -- the default route, MPCQP_OPT_FORCE_CONDENSED, formulation="stagewise" -- and the same batch through
    BatchMPCQP(...).solve(flags=MPCQP_OPT_ON_CHIP_32), at (12, 2, 16, 4) (condensed: 32 variables, 64 rows); all held to the
    stripped reference."""
    from qpmpc_amd import BatchMPCProblem, BatchMPCQP, _capi, solve_mpc_batch

    c = PR.case(PR.RAGGED[0], "tail")
    bp = BatchMPCProblem.from_problems(PR.ragged_problems(c))
    assert np.array_equal(bp.valid_rows, np.flatnonzero(~c["mask"][0]))
    for what, kw in (("default route", {}), ("FORCE_CONDENSED", dict(flags=_capi.OPT_FORCE_CONDENSED)),
                     ("stagewise", dict(formulation="stagewise"))):
        held(c, _plan_out(solve_mpc_batch(bp, return_multipliers=True, **kw)), f"from_problems {c['shape']}, {what}")
    x, lam, status, iters = BatchMPCQP(bp).solve(return_multipliers=True, flags=_capi.OPT_ON_CHIP_32)  # (n = 32, m = 64)
    torch.cuda.synchronize()
    held(c, dict(U=x.cpu().numpy(), lam=lam.cpu().numpy(), status=status.cpu().numpy(), iters=iters.cpu().numpy()),
         f"from_problems {c['shape']}, BatchMPCQP.solve on chip")
