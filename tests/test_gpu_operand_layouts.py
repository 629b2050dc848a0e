"""GPU tests (-m gpu): the operand addressing of include/mpcqp.h, kernel by kernel. Every operand is read as
ptr + b*batch_stride + k*step_stride, and A, B, C, D, e may each on their own be per problem or shared, per step or
time-invariant, packed or behind a batch stride wider than their block; goal and targets shared or per problem. That arithmetic
is restated in every kernel file, and several launch decisions hang on the layout (the strides the quad builds hoist, the LDS
image of mpcqp_pair.hip, the fused constraint layout of mpcqp_stagew.hip, fits_on_chip in route()).

tests/operand_layouts.py holds the layouts (LAYOUTS: every operand in every form, no two moving together; the odd-numbered ones
padded by a different amount per operand, PADS), the generator and the routes; tests/test_operand_layouts_cpu.py shows that
every case has nine solvable problems of which at least six have a binding row, and that any two blocks of an operand differ.

Each launch has its operands in the guarded arena of tests/guarded_launch.py in the STORED layout and runs once under
the all-0xFF fill: padding and guards hold NaN, so a read into the padding poisons the plan and an overrun is named. The
reference always sees the MATERIALISED problems ([B, N, ...] operands), so the oracle's own stride handling is not what vouches
for a kernel's. Bounds are those of tests/test_gpu_memory_discipline.py: 1e-7 relative for float64 plans, 1e-3 for float32 ones
against the oracle on the float32-rounded operands, 1e-8 (close()) for derivatives, 1e-12 for condensed matrices.

Which kernel a forced route reaches does not depend on the layout at these shapes, by the dispatch code as it stands: quad_applies,
quad4_applies, quad_general (lean or general build), w64_eligible, stage_supported, stagew_supported and stageg_supported read
dimensions, pointers and flags, never strides. Strides enter in four places. pair_eligible sizes the pair kernel's LDS image by
the step strides: a few hundred doubles at (3, 1, 16, 2) and (4, 2, 8, 2) against its 64 KiB, whatever the layout. mid_supported
counts the operands' blocks: most with everything per step, which is what test_mid_size_fused_kernel launches at this shape.
MPCQP_OPT_FORCE_LDS sizes the workgroup kernel's image by A's and B's step strides and REFUSES (MPCQP_ETOOLARGE) what does
not fit, it does not go elsewhere: a return code other than 0 fails the case. route()'s fits_on_chip with the launch's own
strides is reached only where w64_eligible already holds. Inside a kernel the layout does pick code: the strides the quad
builds hoist, and the fused constraint layout of mpcqp_stagew.hip on the layouts whose C and D are both time-invariant
(OL.coverage()). A layout that a route did refuse would be skipped with the code that refuses it (SKIPS); none is today."""
import ctypes as C
import os

import numpy as np
import pytest

import operand_layouts as OL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers and comparisons; needs torch)
from guarded_launch import Forward, Launch, ModelCase, against_oracle, plan_jvp, plan_vjp  # noqa: E402
from guarded_launch import flags as _flags  # noqa: E402

F, F64, F32, I32, U8 = GL.F, GL.F64, GL.F32, GL.I32, GL.U8
ELAYOUT = -4
NL = len(OL.LAYOUTS)

# (route, layout) -> the code that refuses it. A skip is never silent, and no route may skip more than a third of the layouts.
SKIPS = {}


# ---------------------------------------------------------------------------------------------- forward: route x layout
WORST = {}  # route -> [layouts run, layouts skipped, worst relative error against the oracle]


@pytest.fixture(scope="module", autouse=True)
def _report():
    """With MPCQP_LAYOUT_REPORT=<path> the forward cases' worst errors per route are written there (profiles/operand_layouts.txt)."""
    yield
    path = os.environ.get("MPCQP_LAYOUT_REPORT")
    complete = list(WORST) == list(OL.ROUTES) and all(ran + skipped == NL for ran, skipped, _ in WORST.values())
    if path and complete:  # (a partial run, -k, writes nothing)
        with open(path, "w") as fh:
            fh.write("tests/test_gpu_operand_layouts.py::test_forward_route_layout, 9 problems per launch, fill 0xFF.\n"
                     "Worst max |u - u_oracle| / max(1, |u_oracle|) over the layouts of tests/operand_layouts.py, oracle on the\n"
                     "materialised problems (bound: 1e-7 float64, 1e-3 float32 against the float32-rounded operands).\n\n")
            fh.write(f"{'route':44s} {'shape':18s} {'run':>4s} {'skipped':>8s} {'worst error':>12s}\n")
            for route, (ran, skipped, err) in WORST.items():
                fh.write(f"{route:44s} {str(OL.ROUTES[route]['shape']):18s} {ran:4d} {skipped:8d} {err:12.2e}\n")


FORWARD = [(route, i) for route in OL.ROUTES for i in range(NL)]


def test_no_route_skips_more_than_a_third():
    for route in OL.ROUTES:
        assert sum((route, i) in SKIPS for i in range(NL)) * 3 <= NL, route
    assert all(key in FORWARD and reason for key, reason in SKIPS.items())


@pytest.mark.parametrize("route,layout", FORWARD, ids=[f"{r}-{i}" for r, i in FORWARD])
def test_forward_route_layout(route, layout):
    """One launch of layout `layout` through the route: return code 0, guards intact and operands unchanged (Launch.run), every
    status the oracle's (all solved), the plan within the route's bound of the oracle on the materialised problems."""
    r = OL.ROUTES[route]
    tally = WORST.setdefault(route, [0, 0, 0.0])
    if (route, layout) in SKIPS:
        tally[1] += 1
        pytest.skip(SKIPS[(route, layout)])
    key, (w, full) = OL.route_case(route, layout)
    case = Forward(w, dtype=F32 if r["f32"] else None, stagewise=r["stagewise"], pad=OL.pads_of(layout))
    assert case.B == OL.BATCH
    out = case.run(F, _flags(r["flags"]))
    Uo, _, sto = GL.oracle_of(repr(key), full)
    assert (sto == 0).all(), sto
    scale = np.maximum(1.0, np.abs(Uo).max(axis=1, keepdims=True))
    err = float((np.abs(out["U"].astype(np.float64) - Uo) / scale).max())
    tally[0] += 1
    tally[2] = max(tally[2], err) if np.isfinite(err) else float("nan")
    print(f"    {route}, layout {layout} {OL.LAYOUTS[layout]}: status {out['status'].tolist()}, max rel err {err:.2e}")
    assert np.array_equal(out["status"], sto), (out["status"], sto)
    against_oracle(repr(key), full, out, 1e-3 if r["f32"] else 1e-7)


# ---------------------------------------------------------------------------------------------- shared-model solves
@pytest.mark.parametrize("variant", range(len(OL.MODEL_VARIANTS)))
@pytest.mark.parametrize("shape", OL.MODEL_SHAPES)
def test_shared_model_solves(shape, variant):
    """mpcqp_solve_model_batch and _bounds_batch, two and four per wavefront, 9 problems that share A, B, C, D (per step): x0, goal,
    targets and (for the bounds export) e per problem or shared, packed and padded, against the oracle on the materialised
    problems at 1e-7. The export without bounds takes e from the model, so it runs where the variant shares e. The model is
    factored in the arena before every solve (ModelCase, factor_in_arena)."""
    from qpmpc_amd import _capi

    v = OL.MODEL_VARIANTS[variant]
    nx, nu, N, mk = shape
    w, full = OL.model_case(shape, variant)
    B = OL.BATCH
    for key, width in (("x0", nx), ("goal", nx), ("targets", N * nx), ("e", N * mk)):
        assert w[key].reshape(w[key].shape[0], -1).shape == (B if v[key] == "b" else 1, width)
    case = ModelCase(w, OL.model_pads(variant), factor_in_arena=True)
    assert case.B == B
    ran = 0
    for flags in (_capi.OPT_TWO_PER_WAVE, _capi.OPT_FOUR_PER_WAVE):
        for bounds in (True, False):
            if not bounds and v["e"] == "b":
                continue  # (without the bounds operand every problem has the model's e)
            out = case.run(F, flags, bounds)
            ok = against_oracle(f"model {shape} {variant}", full, out, 1e-7)
            assert ok.all() and (out["status"] == 0).all(), out["status"]
            ran += 1
    assert ran >= 2


# ---------------------------------------------------------------------------------------------- derivative exports
DIFF_LAYOUTS = OL.DIFF_LAYOUTS


_DIFF = {}


def _diff_case(shape, layout):
    """(w, full, U, lam, status) of a derivative case: the plan and multipliers are the CPU oracle's on the materialised problems"""
    if (shape, layout) not in _DIFF:
        w, full = OL.diff_case(shape, layout)
        _DIFF[(shape, layout)] = (w, full) + GL.forward_on_cpu(full)
    return _DIFF[(shape, layout)]


VJP = [(kind, shape, i) for i in DIFF_LAYOUTS for kind, shape in
       (("condensed", (3, 2, 8, 2)), ("model", (3, 2, 8, 2)), ("stagewise", (3, 2, 8, 2)), ("stagewise", (3, 2, 70, 2)))]


@pytest.mark.parametrize("kind,shape,layout", VJP)
def test_plan_vjp_layouts(kind, shape, layout):
    """mpcqp_plan_vjp_batch / _vjp_model_batch / _vjp_stagewise_batch as tests/test_gpu_memory_discipline.py::test_plan_vjp_exports
    sets them up, the operands in the stored, padded layout; every gradient per problem against the NumPy restatement on the
    materialised problem (the sum over a shared operand is the caller's)."""
    plan_vjp(kind, shape, _diff_case(shape, layout), OL.pads_of(layout), layout)


JVP = [(model, sw, shape, i) for i in DIFF_LAYOUTS for model, sw, shape in
       ((False, False, (3, 2, 8, 2)), (True, False, (3, 2, 8, 2)), (False, True, (3, 2, 8, 2)), (True, True, (3, 2, 8, 2)),
        (False, True, (3, 2, 70, 2)), (True, True, (3, 2, 70, 2)))]


@pytest.mark.parametrize("model,stagewise,shape,layout", JVP)
def test_plan_jvp_layouts(model, stagewise, shape, layout):
    """mpcqp_plan_jvp_batch / _jvp_stagewise_batch / _jvp_model_batch / _jvp_model_stagewise_batch as
    tests/test_gpu_memory_discipline.py::test_plan_jvp_exports sets them up, three tangents, the operands in the stored, padded
    layout; dU and dX per problem against the NumPy restatement on the materialised problem."""
    plan_jvp(model, stagewise, shape, _diff_case(shape, layout), OL.pads_of(layout), layout)


# ---------------------------------------------------------------------------------------------- condensing, vectors, roll-out
@pytest.mark.parametrize("layout", DIFF_LAYOUTS)
def test_condense_update_vectors_and_rollout_layouts(layout):
    """mpcqp_condense_batch, mpcqp_update_vectors_batch and mpcqp_rollout_batch at (4, 2, 10, 3), the operands in the stored, padded
    layout, against oracle/condense_np.py and a NumPy roll-out on the materialised problems at 1e-12 relative (the bounds of
    test_condense_and_its_phases and test_update_vectors_and_rollout)."""
    from qpmpc_amd import workloads as W

    _, lib, stream = GL._api()
    w, full = OL.condense_case(layout)
    bp = W.to_batch_problem(w)
    B, n, m, N, nx = bp.batch_size, bp.nb_variables, bp.nb_constraints, bp.nb_timesteps, bp.state_dim
    assert B == OL.BATCH
    dims, nbytes = bp.dims(), C.c_size_t(0)
    assert lib.mpcqp_workspace_bytes(C.byref(dims), B, 0, C.byref(nbytes)) == 0
    refs = GL.condense_refs(full, B)
    Uin = np.random.default_rng(5).standard_normal((B, n))
    pad = OL.pads_of(layout)
    L = Launch()
    GL.add_problem(L, bp, pad)
    sizes = dict(P=n * n, q=n, G=m * n, h=m, Phi=(N + 1) * nx * nx, Psi=(N + 1) * nx * n)
    for key, count in sizes.items():
        L.add(key, "out", F64, B * count)
    L.add("Phi_in", "in", F64, data=np.stack([np.vstack([c.Phi, c.phi_last]) for c in refs]))
    L.add("Psi_in", "in", F64, data=np.stack([np.vstack([c.Psi, c.psi_last]) for c in refs]))
    L.add("Uin", "in", F64, data=Uin)
    L.add("q2", "out", F64, B * n)
    L.add("h2", "out", F64, B * m)
    L.add("X", "out", F64, B * (N + 1) * nx)
    L.add("ws", "scratch", U8, nbytes.value)
    L.build()
    cp = GL.arena_problem(L, bp, pad)

    def condense():
        return lib.mpcqp_condense_batch(C.byref(dims), C.byref(cp), B, L.ptr("P"), L.ptr("q"), L.ptr("G"), L.ptr("h"), L.ptr("Phi"),
                                        L.ptr("Psi"), L.ptr("ws"), nbytes.value, stream())

    def update():
        return lib.mpcqp_update_vectors_batch(C.byref(dims), C.byref(cp), L.ptr("Phi_in"), sizes["Phi"], L.ptr("Psi_in"),
                                              sizes["Psi"], B, L.ptr("q2"), L.ptr("h2"), stream())

    def rollout():
        return lib.mpcqp_rollout_batch(C.byref(dims), C.byref(cp.A), C.byref(cp.B), C.byref(cp.x0), L.ptr("Uin"), B, L.ptr("X"),
                                       stream())

    cond, upd, roll = L.run(F, condense), L.run(F, update), L.run(F, rollout)
    for b, cq in enumerate(refs):
        for key, want in (("P", cq.P), ("q", cq.q), ("G", cq.G), ("h", cq.h), ("Phi", np.vstack([cq.Phi, cq.phi_last])),
                          ("Psi", np.vstack([cq.Psi, cq.psi_last]))):
            got = cond[key].reshape(B, -1)[b].reshape(want.shape)
            assert GL._rel(got, want) <= 1e-12, (layout, b, key, GL._rel(got, want))
        assert GL._rel(upd["q2"].reshape(B, n)[b], cq.q) <= 1e-12 and GL._rel(upd["h2"].reshape(B, m)[b], cq.h) <= 1e-12, (layout, b)
        x = full["x0"][b]
        want = [x]
        for k in range(N):
            x = full["A"][b, k] @ x + full["B"][b, k] @ Uin[b].reshape(N, -1)[k]
            want.append(x)
        assert GL._rel(roll["X"].reshape(B, -1)[b], np.concatenate(want)) <= 1e-12, (layout, b)


# ---------------------------------------------------------------------------------------------- MPCQP_ELAYOUT
def _extents(nx, nu, N, mk):
    return dict(A=N * nx * nx, B=N * nx * nu, C=N * mk * nx, D=N * mk * nu, e=N * mk, x0=nx, goal=nx, targets=N * nx)


@pytest.mark.parametrize("export", ["build_solve", "stagewise_solve", "plan_vjp"])
def test_short_and_negative_batch_strides_are_refused(export):
    """include/mpcqp.h: a non-zero batch stride smaller than a problem's extent, or a negative one, is MPCQP_ELAYOUT before anything
    is launched. Every operand in turn gets extent - 1, then -extent, then (the matrices) a negative step stride; every output
    buffer and the workspace still hold the fill. The well-formed call next to them returns 0."""
    from qpmpc_amd import _capi, autodiff
    from qpmpc_amd import workloads as W

    _, lib, stream = GL._api()
    shape = (3, 2, 8, 2)
    nx, nu, N, mk = shape
    everything = dict(A="bn", B="bn", C="bn", D="bn", e="bn", goal="b", targets="b")
    w, full = OL.make(shape, "cd", True, everything, 7000, 0.5)
    bp = W.to_batch_problem(w)
    B, n, m = OL.BATCH, N * nu, N * mk
    L = Launch()
    GL.add_problem(L, bp)
    nbytes = C.c_size_t(0)
    o = _capi.SolveOpts()
    if export == "plan_vjp":
        U, lam, status = GL.forward_on_cpu(full)
        dims = autodiff._vjp_dims(bp)
        assert lib.mpcqp_plan_vjp_workspace_bytes(C.byref(dims), B, C.byref(nbytes)) == 0
        L.add("lam", "in", F64, data=lam)
        L.add("gU", "in", F64, data=np.ones((B, n)))
        L.add("status_in", "in", I32, data=torch.as_tensor(status))
        outs = dict(g_x0=nx, g_goal=nx, g_targets=N * nx, g_e=m)
        for key, count in outs.items():
            L.add(key, "out", F64, B * count)
        L.add("vjp_status", "out", I32, B)
    else:
        dims = bp.dims()
        if export == "stagewise_solve":
            assert lib.mpcqp_stagewise_workspace_bytes(C.byref(dims), B, 0, C.byref(nbytes)) == 0
        else:
            assert lib.mpcqp_workspace_bytes(C.byref(dims), B, 1, C.byref(nbytes)) == 0
        L.add("U", "out", F64, B * n)
        L.add("lam", "out", F64, B * m)
        L.add("status", "out", I32, B)
        L.add("iters", "out", I32, B)
    L.add("ws", "scratch", U8, nbytes.value)
    L.build()

    def call_with(cp):
        if export == "plan_vjp":
            return lib.mpcqp_plan_vjp_batch(C.byref(dims), C.byref(cp), B, L.ptr("lam"), L.ptr("status_in"), L.ptr("gU"), None,
                                            L.ptr("g_x0"), L.ptr("g_goal"), L.ptr("g_targets"), L.ptr("g_e"), L.ptr("vjp_status"),
                                            L.ptr("ws"), nbytes.value, stream())
        tail = (L.ptr("U"), L.ptr("lam"), L.ptr("status"), L.ptr("iters"), L.ptr("ws"), nbytes.value, stream())
        if export == "stagewise_solve":
            return lib.mpcqp_stagewise_solve_batch(C.byref(dims), C.byref(cp), B, C.byref(o), 0, *tail)
        return lib.mpcqp_build_solve_batch(C.byref(dims), C.byref(cp), B, C.byref(o), *tail)

    tried = 0
    for name, extent in _extents(*shape).items():
        bad = [("batch_stride", extent - 1), ("batch_stride", -extent)]
        if name in OL.MATS:
            bad.append(("step_stride", -(extent // N)))
        for field, value in bad:
            cp = GL.arena_problem(L, bp)
            op = getattr(cp, name)
            assert op.ptr and op.batch_stride == extent
            setattr(op, field, value)
            rcs = []

            def refused():
                rcs.append(call_with(cp))
                return 0

            out = L.run(F, refused)
            assert rcs == [ELAYOUT], (export, name, field, value, rcs)
            for key, buf in out.items():
                assert GL.holds(buf, F), (export, name, field, value, key, "was written by a refused call")
            tried += 1
    assert tried == 8 * 2 + 5
    good = L.run(F, lambda: call_with(GL.arena_problem(L, bp)))
    assert not GL.holds(good["g_x0" if export == "plan_vjp" else "U"], F)
    assert b"batch stride" in lib.mpcqp_error_string(ELAYOUT)
