"""CPU tests: the inputs of tests/test_gpu_operand_layouts.py are worth launching. For every (route, layout) pair of the GPU test

  * the C oracle solves all 9 materialised problems and at least 6 of them have a multiplier above 1e-9 -- a row must bind, or
    C, D and e cannot change the plan and a kernel that misreads them passes;
  * the oracle on the stored (reduced) operands and on the materialised ones agrees in status and in U to 1e-9: both dicts
    state the same problems;
  * any two blocks of an operand the layout keeps per problem or per step differ by more than 1e-3 somewhere: a kernel that
    reads the wrong block reads different numbers;
  * the reference can be trusted at the bound the case is held to: the float64 oracle solves the condensed QP, so its own
    error is of the order cond(P) * 2.2e-16, which must stay below a tenth of the bound (1e-7 in float64, 1e-3 in float32);

the same for the inputs of the derivative, shared-model and condensing tests; and the layout list has the coverage its docstring
claims. The refusals of check_problem() (MPCQP_ELAYOUT) are reached here too: they come before any launch."""
import itertools

import numpy as np
import pytest

import oracle

import operand_layouts as OL


def test_layout_list_coverage():
    assert len(OL.LAYOUTS) >= 12
    cyc = OL.LAYOUTS[:12]
    assert len({tuple(sorted(l.items())) for l in OL.LAYOUTS}) == len(OL.LAYOUTS), "a layout is listed twice"
    for X in OL.MATS:  # every operand takes every form three times in the cyclic part
        assert sorted(l[X] for l in cyc) == sorted(OL.OPTS * 3), X
    for X, Y in itertools.combinations(OL.MATS, 2):  # no two operands move together: a pair takes more than four combinations
        assert len({(l[X], l[Y]) for l in cyc}) > 4, (X, Y)
    for X in ("goal", "targets"):
        assert {l[X] for l in OL.LAYOUTS} == {"b", "1"}
    assert {(l["goal"], l["targets"]) for l in cyc} == set(itertools.product("b1", "b1"))
    for what, have in OL.coverage().items():
        assert have, what
    # the fused constraint layout of mpcqp_stagew.hip with e per step and the two arguments of fits_on_chip, packed and padded
    ti = OL.time_invariant
    assert any(ti(l["C"]) and ti(l["D"]) and l["e"] == "bn" for l in OL.LAYOUTS)
    assert any(ti(l["A"]) and not ti(l["B"]) and l["A"][0] == "b" and l["B"][0] == "b" for l in OL.LAYOUTS)
    assert OL.pads_of(0) == 0 and OL.pads_of(1) == OL.PADS and len(set(OL.PADS.values())) >= 6
    assert any(v % 2 for v in OL.PADS.values()) and 0 in OL.PADS.values()  # (odd amounts break every alignment; one operand packed)
    # the derivative tests' four layouts: two packed, two padded
    assert [bool(OL.pads_of(i)) for i in OL.DIFF_LAYOUTS] == [False, True, True, True, False, True]
    # every operand meets a padded batch stride somewhere: non-zero padding on an odd-numbered layout that keeps it per problem
    for X in OL.MATS + ("goal", "targets"):
        if X != "D":  # (D stays packed among padded operands)
            assert OL.PADS[X] > 0 and any(i % 2 and l[X][0] == "b" for i, l in enumerate(OL.LAYOUTS)), X
            assert any(OL.pads_of(i) and OL.LAYOUTS[i][X][0] == "b" for i in OL.DIFF_LAYOUTS), X
    assert OL.PADS["x0"] > 0
    for X in OL.MODEL_PADS:  # shared-model solves: x0, goal, targets, e each per problem and shared, packed and padded
        assert OL.MODEL_PADS[X] > 0
        seen = {(v[X], bool(i % 2)) for i, v in enumerate(OL.MODEL_VARIANTS)}
        assert {("b", False), ("b", True), ("1", False), ("1", True)} <= seen, (X, seen)


def test_stored_shapes_follow_the_layout():
    nx, nu, N, mk = 4, 2, 8, 3
    blocks = dict(A=(nx, nx), B=(nx, nu), C=(mk, nx), D=(mk, nu), e=(mk,))
    for i, lay in enumerate(OL.LAYOUTS):
        w, full = OL.make((nx, nu, N, mk), "cd", True, i, 1000 + i, 0.2)
        for X in OL.MATS:
            want = (OL.BATCH if lay[X][0] == "b" else 1, N if lay[X][1] == "n" else 1) + blocks[X]
            assert w[X].shape == want and full[X].shape == (OL.BATCH, N) + blocks[X], (i, X)
            assert np.array_equal(np.broadcast_to(w[X], full[X].shape), full[X])
        for X, width in (("goal", nx), ("targets", N * nx)):
            assert w[X].shape == (OL.BATCH if lay[X] == "b" else 1, width) and full[X].shape == (OL.BATCH, width)
        # u = 0 is feasible for every problem on the materialised operands
        for b in range(OL.BATCH):
            x = full["x0"][b]
            for k in range(N):
                assert (full["C"][b, k] @ x <= full["e"][b, k] - 0.2 * 0.05 + 1e-12).all(), (i, b, k)
                x = full["A"][b, k] @ x
    w, full = OL.make((3, 1, 16, 2), "c", False, 5, 1, 0.2)
    assert w["D"] is None and full["D"] is None and w["targets"] is None and w["wx"] is None and w["C"] is not None
    w, full = OL.make((3, 1, 16, 2), "d", True, 5, 1, 0.2)
    assert w["C"] is None and full["C"] is None and w["D"] is not None and (w["e"] > 0).all()


def _blocks_differ(a, per_problem, per_step):
    """any two blocks along the axes the layout keeps differ by more than 1e-3 somewhere"""
    flat = a.reshape(a.shape[0] * a.shape[1], -1) if a.ndim > 2 else a
    assert flat.shape[0] == (OL.BATCH if per_problem else 1) * (a.shape[1] if (per_step and a.ndim > 2) else 1)
    gap = np.abs(flat[:, None, :] - flat[None, :, :]).max(axis=2)
    gap[np.diag_indices(len(flat))] = np.inf
    return float(gap.min()) > 1e-3


CASES = [(route, i) for route in OL.ROUTES for i in range(len(OL.LAYOUTS))]


_VERDICT = {}  # routes of equal shape, rows, cost, margin, seed and dtype share their problems: those are judged once


@pytest.mark.parametrize("route,layout", CASES, ids=[f"{r}-{i}" for r, i in CASES])
def test_inputs_of_the_gpu_test(route, layout):
    r = OL.ROUTES[route]
    key, (w, full) = OL.route_case(route, layout)
    assert r["shape"] == (w["A"].shape[-1], w["B"].shape[-1], int(w["N"]), w["e"].shape[-1])
    if key not in _VERDICT:
        try:
            _check_inputs(r, OL.LAYOUTS[layout], w, full, OL.oracle_on_full(route, layout))
            _VERDICT[key] = None
        except AssertionError as exn:
            _VERDICT[key] = exn
    if _VERDICT[key] is not None:
        raise _VERDICT[key]


def _check_inputs(r, lay, w, full, solved):
    from oracle import condense_np
    from qpmpc_amd.workloads import problem_from_workload

    U, lam, status = solved
    # (the derivative exports take unsolved items too -- zeros and their status --: their long case may hold some)
    assert (status == 0).all() or (r.get("unsolved_ok") and (status == 0).sum() >= 6), status
    bound = int(((lam > 1e-9).any(axis=1) & (status == 0)).sum())
    assert bound >= 6, f"only {bound} of {OL.BATCH} problems have a binding row"
    if lay.get("x0", "b") == "b" and (status == 0).all():  # (a workload dict takes its batch size from x0: one with a shared x0 states one problem)
        Uw, _, stw, _ = oracle.solve_workload(w)
        assert np.array_equal(stw, status)
        assert float(np.abs(Uw - U).max()) <= 1e-9, float(np.abs(Uw - U).max())
    for X in OL.MATS:
        if w[X] is not None and lay[X] != "11":
            assert _blocks_differ(w[X], lay[X][0] == "b", lay[X][1] == "n"), X
    for X in ("x0", "goal", "targets"):
        if w[X] is not None and lay.get(X, "b") == "b":
            assert _blocks_differ(w[X], True, False), X
    if r.get("tol") is None:
        return  # (the condensing cases are held to NumPy restatements of products, not to a solve)
    n = r["shape"][1] * r["shape"][2]
    for b in (range(OL.BATCH) if n <= 100 else (0, OL.BATCH // 2, OL.BATCH - 1)):  # (P depends on A, B and the weights only)
        cond = float(np.linalg.cond(condense_np.condense(problem_from_workload(full, b)).P))
        assert cond * 2.2e-16 <= r.get("tol", 1e-3 if r["f32"] else 1e-7) / 10, (b, cond)


OTHER = ([("diff", shape, i) for shape in OL.DIFF_SHAPES for i in OL.DIFF_LAYOUTS] + [("condense", OL.CONDENSE_SHAPE, i) for i in OL.DIFF_LAYOUTS]
         + [("model", shape, v) for shape in OL.MODEL_SHAPES for v in range(len(OL.MODEL_VARIANTS))])


@pytest.mark.parametrize("kind,shape,index", OTHER)
def test_inputs_of_the_other_gpu_tests(kind, shape, index):
    """the derivative, condensing and shared-model cases: the same conditions as the forward ones; cond(P) * 2.2e-16 below a tenth
    of the bound where the reference solves with P (the oracle at 1e-7, the derivatives' NumPy restatements at 1e-8)"""
    if kind == "model":
        (w, full), lay = OL.model_case(shape, index), OL.model_layout(index)
    else:
        (w, full), lay = (OL.diff_case(shape, index) if kind == "diff" else OL.condense_case(index)), OL.LAYOUTS[index]
    _check_inputs(dict(shape=shape, f32=False, tol=dict(model=1e-7, diff=1e-8, condense=None)[kind], unsolved_ok=kind == "diff"), lay, w, full, oracle.solve_workload(full)[:3])


def test_short_and_negative_strides_are_refused_before_any_launch():
    """check_problem() of mpcqp_capi.hip, reached without a GPU (dummy addresses, an empty batch for the well-formed call): a
    negative stride, a step stride that is not the block and a non-zero batch stride below a problem's extent are
    MPCQP_ELAYOUT; the packed strides, wider batch strides and 0 are taken."""
    import ctypes as C

    pytest.importorskip("torch")
    from qpmpc_amd import _capi

    lib = _capi.load()
    nx, nu, N, mk = 3, 2, 8, 2
    d = _capi.Dims(nx, nu, N, mk, _capi.F64, 0, 1.0, 1.0, 0.1)
    blocks = dict(A=nx * nx, B=nx * nu, C=mk * nx, D=mk * nu, e=mk, x0=nx, goal=nx, targets=N * nx)

    def rc(**strides):
        p = _capi.Problem()
        for name, block in blocks.items():
            step = block if name in OL.MATS else 0
            bs, ks = strides.get(name, ((N * block if step else block), step))
            setattr(p, name, _capi.Operand(8, bs, ks))
        return lib.mpcqp_build_solve_batch(C.byref(d), C.byref(p), 0, None, 8, None, 8, None, None, 0, None)

    ELAYOUT = -4
    assert rc() == 0
    for name, block in blocks.items():
        per_step = name in OL.MATS
        extent = N * block if per_step else block
        assert rc(**{name: (extent - 1, block if per_step else 0)}) == ELAYOUT, name
        assert rc(**{name: (-extent, block if per_step else 0)}) == ELAYOUT, name
        assert rc(**{name: (extent + 5, block if per_step else 0)}) == 0, name
        assert rc(**{name: (0, block if per_step else 0)}) == 0, name
        if per_step:
            assert rc(**{name: (extent, -block)}) == ELAYOUT and rc(**{name: (extent, block + 1)}) == ELAYOUT, name
            assert rc(**{name: (block, 0)}) == 0 and rc(**{name: (block - 1, 0)}) == ELAYOUT, name  # (time-invariant: one block)
    assert b"batch stride" in lib.mpcqp_error_string(ELAYOUT)
    # mpcqp_update_vectors_batch needs no A and B and makes the same check of the operands it is given
    p = _capi.Problem()
    for name in ("C", "e", "x0", "goal", "targets"):
        setattr(p, name, _capi.Operand(8, 0, 0))

    def update():
        return lib.mpcqp_update_vectors_batch(C.byref(d), C.byref(p), 8, 0, 8, 0, 0, 8, 8, None)

    assert update() == 0
    p.goal.batch_stride = nx - 1
    assert update() == ELAYOUT
    p.goal.batch_stride, p.e.batch_stride = nx, -mk
    assert update() == ELAYOUT
