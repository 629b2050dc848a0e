"""CPU tests: the inputs of tests/test_gpu_padded_rows.py are worth launching. For every case of tests/padded_rows.py, on the C oracle,

  * every item of the stripped reference (padded rows deleted from G and h) is solved;
  * the C oracle on the PADDED workload agrees with the stripped reference to 1e-10 relative (measured: at most 7e-13), and its
    multipliers on padded rows are exactly 0 -- the padding convention means to the oracle what the header says;
  * at least 6 of 9 items have a binding real row (a multiplier above 1e-9);
  * the padding matters: in at least 6 of 9 items the plan differs from the plan of the same problem with its rows left in place
    by at least ten times the bound the route is held to (1e-7 float64, 1e-3 float32) -- a kernel that ignored the padding, or
    padded the wrong row, would miss the bound (only items whose unpadded problem the oracle solves too are counted);
  * cond(P) * 2.2e-16 is at most a tenth of the bound for every item (the reference can be trusted there), as
    tests/test_operand_layouts_cpu.py asks;
  * `mixed`: item B - 2, padded whole, has no active row and 0 iterations;
  * warm pairs: in at least 6 of 9 items an active row id of the first problem, minus mk, names a padded row of the second.

A case that cannot meet the conditions has another draw or padded row (padded_rows.CHOICE), never a looser condition; the search
that found it is run again here."""
import numpy as np
import pytest

import operand_layouts as OL
import padded_rows as PR

CASES = [(name, placement) for name in PR.ROUTES for placement in PR.PLACEMENTS]
_VERDICT = {}  # routes of equal problems share a case: judged once


def _check(c):
    nx, nu, N, mk = c["shape"]
    B, m = PR.BATCH, N * mk
    assert c["mask"].shape == (B, m) and c["mask"].any() and c["full"]["e"].shape == (B, N, mk)
    e = np.asarray(c["full"]["e"]).reshape(B, m)
    assert (e[c["mask"]] >= 1e29).all() and (np.abs(e[~c["mask"]]) < 1e3).all()
    for X in ("C", "D"):
        if c["full"][X] is not None:
            a = np.asarray(c["full"][X]).reshape(B, m, -1)
            assert not a[c["mask"]].any() and (np.abs(a[~c["mask"]]).max(axis=1) > 0).all(), X
            assert np.array_equal(np.broadcast_to(c["w"][X], c["full"][X].shape), c["full"][X]), X
    cd = PR.conditions(c)
    print(f"    {c['shape']} {c['placement']}: binding {cd['binding']}, moved {cd['moved']}, padded oracle vs stripped "
          f"{cd['padded agrees']:.1e}, cond(P) {cd['cond']:.1e}")
    assert (cd["status"] == 0).all(), cd["status"]
    assert (cd["padded status"] == 0).all() and cd["padded agrees"] <= 1e-10, (cd["padded status"], cd["padded agrees"])
    assert cd["padded lam"] == 0.0
    assert cd["binding"] >= PR.MIN_ITEMS, f"only {cd['binding']} of {B} items have a binding real row"
    assert cd["moved"] >= PR.MIN_ITEMS, f"the padding moves only {cd['moved']} of {B} plans by {PR.SEPARATION} x the bound"
    assert cd["cond"] * 2.2e-16 <= c["bound"] / 10, cd["cond"]
    assert PR.serves(cd)
    U, lam, st, it = PR.reference(c)
    assert not lam[c["mask"]].any()
    if c["placement"] == "mixed":
        assert c["mask"].reshape(B, N, mk)[:, N // 2].all() and c["mask"][:, 0].all()  # a whole step, the head row of a step
    if c["placement"] == "mixed" and not c.get("shared"):
        assert c["mask"][B - 2].all() and not lam[B - 2].any() and it[B - 2] == 0
        assert PR.rel(U[B - 2:B - 1], PR.unconstrained(c, B - 2)[None])[0] == 0.0


@pytest.mark.parametrize("name,placement", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_inputs_of_the_forward_test(name, placement):
    key = PR.case_key(name, placement)
    c = PR.case(name, placement)
    assert c["shape"] == PR.ROUTES[name]["shape"] and c["placement"] == placement
    if key not in _VERDICT:
        try:
            _check(c)
            _VERDICT[key] = None
        except AssertionError as exn:
            _VERDICT[key] = exn
    if _VERDICT[key] is not None:
        raise _VERDICT[key]


def test_placements():
    B, N, mk = 9, 7, 3
    t = PR.tail(B, N, mk)
    for k in range(N):  # what BatchMPCProblem.from_problems makes of steps with 1 + k % mk rows
        assert not t[:, k, :k % mk + 1].any() and t[:, k, k % mk + 1:].all()
    x = PR.mixed(B, N, mk, np.random.default_rng(0))
    assert x[:, N // 2].all() and x[:, 0, 0].all() and x[B - 2].all()
    others = np.delete(x, B - 2, axis=0).reshape(B - 1, -1)
    assert (others.sum(axis=1) >= N * mk // 4).all() and not others.all(axis=1).any()
    assert len({row.tobytes() for row in others}) == B - 1  # (a quarter of the rows per problem: no two problems alike)
    r = PR.rows(B, N, mk)
    assert r[:, :, mk // 2].all() and r.sum() == B * N
    assert PR.PAD == 1e30
    pytest.importorskip("torch")
    from qpmpc_amd import batch

    assert batch.PAD_BOUND == PR.PAD


def test_recorded_choices_are_the_first_that_serve():
    """every entry of CHOICE: the route's own draw with row mk // 2 does not serve, and the recorded pair is the first of
    candidates() that does"""
    names = {PR.case_key(n, p): (n, p) for n, p in CASES}
    assert set(PR.CHOICE) <= set(names)
    for key, choice in PR.CHOICE.items():
        name, placement = names[key]
        assert choice != (PR.DRAW, None)
        assert PR.first_choice(name, placement) == choice, (name, placement)


@pytest.mark.parametrize("name", PR.RAGGED)
def test_from_problems_makes_the_tail_placement(name):
    """the ragged host problems of a `tail` case, padded by BatchMPCProblem.from_problems, are the case's operands element for
    element, and valid_rows names its real rows"""
    torch = pytest.importorskip("torch")
    from qpmpc_amd import BatchMPCProblem

    c = PR.case(name, "tail")
    bp = BatchMPCProblem.from_problems(PR.ragged_problems(c), device=torch.device("cpu"))
    for key, attr in (("A", "A"), ("B", "B"), ("C", "C"), ("D", "D"), ("e", "e"), ("x0", "initial_state"), ("goal", "goal_state"),
                      ("targets", "target_states")):
        assert np.array_equal(getattr(bp, attr).numpy().reshape(c["full"][key].shape), c["full"][key]), key
    assert all(np.array_equal(bp.valid_rows, np.flatnonzero(~c["mask"][b])) for b in range(PR.BATCH))


OTHER = ([("model", shape, variant, placement) for shape, variant in PR.MODEL_CASES for placement in PR.PLACEMENTS]
         + [("model", PR.MODEL_DIFF_SHAPE, PR.DIFF_VARIANT, "tail")] + [("diff", shape, None, "tail") for shape in OL.DIFF_SHAPES])


def test_recorded_model_choices_are_the_first_that_serve():
    assert set(PR.MODEL_CHOICE) <= {(s, v, p) for _, s, v, p in OTHER}
    for key, j in PR.MODEL_CHOICE.items():
        assert j > 0 and PR.first_model_choice(*key) == j, key


@pytest.mark.parametrize("kind,shape,variant,placement", OTHER)
def test_inputs_of_the_model_and_derivative_tests(kind, shape, variant, placement):
    """the shared-model cases in all three placements (`mixed` in its shareable form: one mask for every problem) and the
    derivative cases: the same conditions as the forward ones"""
    c = PR.model_case(shape, variant, placement) if kind == "model" else PR.diff_case(shape)
    assert c["placement"] == placement
    _check(c)
    if kind == "model":  # the matrices stay shared, e per problem or shared as the variant says
        assert (c["mask"] == c["mask"][:1]).all()
        w = c["w"]
        assert all(w[X].shape[0] == 1 for X in ("A", "B", "C", "D"))
        per_problem = variant != PR.DIFF_VARIANT and OL.MODEL_VARIANTS[variant]["e"] == "b"
        assert w["e"].shape[0] == (PR.BATCH if per_problem else 1)
        assert (w["e"].reshape(w["e"].shape[0], -1)[:, c["mask"][0]] == PR.PAD).all()


@pytest.mark.parametrize("name", list(PR.WARM_SHAPES))
def test_warm_pairs(name):
    shape = PR.WARM_SHAPES[name][0]
    mk = shape[3]
    assert PR.first_warm_t(name) == PR.WARM_T[name]
    for kind in ("operator", "active_set"):
        first, second = PR.warm_pair(name, kind)
        assert np.array_equal(first["mask"], second["mask"])
        for c in (first, second):
            U, lam, st, it = PR.reference(c)
            assert (st == 0).all(), (name, kind, st)
            assert int((lam > 1e-9).any(axis=1).sum()) >= PR.MIN_ITEMS
        assert (PR.rel(PR.reference(second)[0], PR.reference(first)[0]) >= PR.SEPARATION * 1e-7).sum() >= PR.MIN_ITEMS
        if kind == "operator":
            for X in ("A", "B", "C", "D", "e"):
                assert first["full"][X] is second["full"][X] or np.array_equal(first["full"][X], second["full"][X])
            assert np.abs(first["full"]["x0"] - second["full"]["x0"]).max() > 1e-3
        else:
            hit = PR.shifted_onto_padding(first, second, mk)
            print(f"    {name}: a stored id - mk names a padded row in {int(hit.sum())} of {PR.BATCH} items")
            assert hit.sum() >= PR.MIN_ITEMS
