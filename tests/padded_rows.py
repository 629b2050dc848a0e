"""Padded inequality rows (test helper, NumPy only, no GPU): the cases of tests/test_gpu_padded_rows.py.

include/mpcqp.h (MpcqpDims): a problem whose row count varies per step is padded by the host to mk rows with C = D = 0 and
e = 1e30, "an inequality that can never be active". BatchMPCProblem.from_problems makes such rows, solve_mpc and MPCQP strip
them again, and every solver kernel keeps the promise on its own (a row whose bound is at least 1e29 is never a candidate; a
zero row's norm is not divided by). tests/test_padded_rows_cpu.py holds the cases below, on the C oracle, to the conditions that
make a green GPU test mean something.

A case is nine problems of operand_layouts.make at the shape, rows, stage cost, margin, dtype and dynamics of a route, drawn with
seed = the route's seed + DRAW, on which a mask of rows (a placement, drawn with the route's seed + MASK) is turned into padding:

  tail   what from_problems makes: step k keeps rows 0 .. k % mk, the rows behind them are padding; everything per problem, per step.
  mixed  the same layout: a random quarter of each problem's rows, step N // 2 whole, row 0 of step 0 (the head of a step) and
         problem B - 2 whole (an unconstrained problem between constrained lane neighbours).
  rows   C and D shared and time-invariant, e per problem and per step: ONE row index padded at every step, i.e. a zero row in the
         shared block of the fused constraint layout of mpcqp_stagew.hip.

The reference of a case is the STRIPPED problem, never the padded one: each materialised problem is condensed by
oracle/condense_np.py, the padded rows of G and h are deleted and oracle.capi.gi_solve solves what is left; its multipliers are
scattered back to m rows with zeros on the padding. Float32 routes reference the float32-rounded operands.

The shared-model cases (model_case) carry the padding IN THE MODEL, in the same three placements; there `mixed` keeps the parts a
shared C / D block can express -- a step padded whole and the head row of a step, the same mask for every problem. Only its
per-problem parts (the random quarter, the problem padded whole) cannot exist in a shared model: C and D are one block for all
problems, and the header promises nothing for a non-zero row with e = 1e30.

Where the route's own draw cannot meet the conditions (CHOICE) the case takes the first (draw offset, padded row) of
candidates() that does, the way stream_cases searches; the CPU test runs that search again."""
from __future__ import annotations

import numpy as np

import operand_layouts as OL

PAD = 1e30  # qpmpc_amd.batch.PAD_BOUND
BATCH = OL.BATCH
PLACEMENTS = ("tail", "mixed", "rows")
DRAW, MASK = 77, 99
BOUND = {False: 1e-7, True: 1e-3}  # by route["f32"]: the bounds of tests/test_gpu_operand_layouts.py
MIN_ITEMS = 6  # of 9: items with a binding real row, items whose plan the padding moves
SEPARATION = 10.0

ON_CHIP_FUSED = ("on-chip 32 fused (3, 1, 24, 2)", "on-chip 32 fused (4, 2, 16, 4)")
ROUTES = dict(OL.ROUTES)
ROUTES[ON_CHIP_FUSED[0]] = OL.route((3, 1, 24, 2), flags=["OPT_ON_CHIP_32"])
ROUTES[ON_CHIP_FUSED[1]] = OL.route((4, 2, 16, 4), flags=["OPT_ON_CHIP_32"])

_PER_STEP = dict(A="bn", B="bn", C="bn", D="bn", e="bn", goal="b", targets="b")
_SHARED_ROWS = dict(_PER_STEP, C="11", D="11")


# ---------------------------------------------------------------------------------------------- placements: (B, N, mk, rng) -> mask
def tail(B, N, mk, rng=None, row=None):
    mask = np.zeros((B, N, mk), dtype=bool)
    for k in range(N):
        mask[:, k, k % mk + 1:] = True
    return mask


def mixed(B, N, mk, rng, row=None):
    m = N * mk
    mask = np.zeros((B, m), dtype=bool)
    for b in range(B):
        mask[b, rng.permutation(m)[:max(1, m // 4)]] = True
    mask = mask.reshape(B, N, mk)
    mask[:, N // 2] = True
    mask[:, 0, 0] = True
    mask[B - 2] = True
    return mask


def rows(B, N, mk, rng=None, row=None):
    mask = np.zeros((B, N, mk), dtype=bool)
    mask[:, :, mk // 2 if row is None else row] = True
    return mask


MASKS = dict(tail=tail, mixed=mixed, rows=rows)


def pad_rows(w, mask):
    """a copy of workload `w` (operands stored [1|B, 1|N, ...]) with the rows of `mask` [B, N, mk] turned into padding; a shared
    block takes the rows that are padded in EVERY problem (step) it serves, and e must then be per problem and per step"""
    out = dict(w)
    for X in ("C", "D"):
        if w[X] is not None:
            a = np.array(w[X], dtype=np.float64)
            mk_ = mask
            if a.shape[0] == 1:
                assert (mask == mask[:1]).all()
                mk_ = mk_[:1]
            if a.shape[1] == 1:
                assert (mask == mask[:, :1]).all()
                mk_ = mk_[:, :1]
            a[mk_] = 0.0
            out[X] = a
    e = np.array(w["e"], dtype=np.float64)
    assert e.shape == mask.shape
    e[mask] = PAD
    out["e"] = e
    return out


# ---------------------------------------------------------------------------------------------- cases
# (case key) -> (draw offset, padded row of the "rows" placement): the first of candidates() that meets the conditions, where
# (DRAW, mk // 2) does not. tests/test_padded_rows_cpu.py::test_recorded_choices_are_the_first_that_serve runs the search again.
CHOICE = {
    # the lean (3, 1, 16, 2) shape with state rows only: with one of its two rows per step padded, the route's own draw binds in 3
    # of 9 items whichever row goes
    ((3, 1, 16, 2), "c", False, 0.2, 24000, False, False, "rows"): (DRAW + 2000, None),
}


def candidates(mk, placement):
    """the (draw offset, padded row) pairs tried, in this order"""
    for j in range(40):
        for row in ([mk // 2] + [i for i in range(mk) if i != mk // 2] if placement == "rows" else [None]):
            yield DRAW + 1000 * j, row


def case_key(name, placement):
    r = ROUTES[name]
    return (r["shape"], r["rows"], r["stage"], r["margin"], r["seed"], r["contractive"], r["f32"], placement)


_CASES = {}


def build_case(r, placement, draw, row):
    nx, nu, N, mk = r["shape"]
    lay = _SHARED_ROWS if placement == "rows" else _PER_STEP
    w0, full0 = OL.make(r["shape"], r["rows"], r["stage"], lay, r["seed"] + draw, r["margin"], r["contractive"])
    mask = MASKS[placement](BATCH, N, mk, np.random.default_rng(r["seed"] + MASK), row)
    w, full = pad_rows(w0, mask), pad_rows(full0, mask)
    if r["f32"]:
        w, full, full0 = OL.f32_view(w), OL.f32_view(full), OL.f32_view(full0)
    return dict(route=r, placement=placement, shape=r["shape"], w=w, full=full, unpadded=full0, mask=mask.reshape(BATCH, N * mk),
                bound=BOUND[r["f32"]], draw=draw, row=row)


def case(name, placement):
    """the case of route `name` in placement `placement`, made once (routes of equal problems share it): w (stored operands),
    full (materialised), unpadded (the same problems with their rows left in place), mask [B, m] (True: padding), bound"""
    key = case_key(name, placement)
    if key not in _CASES:
        draw, row = CHOICE.get(key, (DRAW, None))
        _CASES[key] = build_case(ROUTES[name], placement, draw, row)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------- reference
def stripped(full, mask):
    """(U, lam, status, iters) of the stripped problems of a materialised workload: condense, delete the padded rows, gi_solve;
    lam is scattered back to m rows with zeros on the padding"""
    from oracle import capi, condense_np
    from qpmpc_amd.workloads import problem_from_workload

    B, m = mask.shape
    U, lam, st, it = [], np.zeros((B, m)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        cq = condense_np.condense(problem_from_workload(full, b))
        keep = ~mask[b]
        assert cq.G.shape[0] == m and (cq.h[mask[b]] >= 1e29).all() and not cq.G[mask[b]].any()
        if keep.any():
            x, l, st[b], it[b] = capi.gi_solve(cq.P, cq.q, cq.G[keep], cq.h[keep])
            lam[b, keep] = l
        else:
            x = -np.linalg.solve(cq.P, cq.q)
        U.append(x)
    return np.array(U), lam, st, it


_REF = {}


def reference(c):
    """stripped() of a case, solved once"""
    if id(c) not in _REF:
        _REF[id(c)] = (c, stripped(c["full"], c["mask"]))
    return _REF[id(c)][1]


def unconstrained(c, b):
    """-P^-1 q of item b"""
    from oracle import condense_np
    from qpmpc_amd.workloads import problem_from_workload

    cq = condense_np.condense(problem_from_workload(c["full"], b))
    return -np.linalg.solve(cq.P, cq.q)


def rel(U, Uref):
    """per item: max |U - Uref| / max(1, max |Uref|)"""
    return np.abs(np.asarray(U, dtype=np.float64) - Uref).max(axis=1) / np.maximum(1.0, np.abs(Uref).max(axis=1))


def conditions(c, with_cond=True):
    """the measured conditions of a case (see tests/test_padded_rows_cpu.py)"""
    import oracle
    from oracle import condense_np
    from qpmpc_amd.workloads import problem_from_workload

    U, lam, st, it = reference(c)
    out = dict(status=st, iters=it, binding=int(((lam > 1e-9).any(axis=1) & (st == 0)).sum()))
    Up, lamp, stp, _ = oracle.solve_workload(c["full"])
    out["padded status"] = stp
    out["padded agrees"] = float(rel(Up, U).max()) if (st == 0).all() and (stp == 0).all() else np.inf
    out["padded lam"] = float(np.abs(lamp[c["mask"]]).max()) if c["mask"].any() else 0.0
    U0, _, st0, _ = oracle.solve_workload(c["unpadded"])
    # (a difference between two PLANS: an item whose unpadded problem the oracle does not solve is not counted)
    out["moved"] = int(((rel(U0, U) >= SEPARATION * c["bound"]) & (st0 == 0) & (st == 0)).sum())
    if with_cond:  # (every item: A and B are per problem here, so P is)
        out["cond"] = max(float(np.linalg.cond(condense_np.condense(problem_from_workload(c["full"], b)).P)) for b in range(BATCH))
    return out


def serves(cd):
    return bool((cd["status"] == 0).all() and (cd["padded status"] == 0).all() and cd["binding"] >= MIN_ITEMS
                and cd["moved"] >= MIN_ITEMS and cd["padded agrees"] <= 1e-10 and cd["padded lam"] == 0.0)


def first_choice(name, placement, most=None):
    """the first (draw offset, row) of candidates() whose case serves; None if none of the first `most` does"""
    r = ROUTES[name]
    for i, (draw, row) in enumerate(candidates(r["shape"][3], placement)):
        if most is not None and i >= most:
            return None
        if serves(conditions(build_case(r, placement, draw, row), with_cond=False)):
            return draw, (None if row == r["shape"][3] // 2 or row is None else row)
    return None


# ---------------------------------------------------------------------------------------------- the other tests' inputs
# shared-model solves: the shapes of operand_layouts.MODEL_SHAPES (the small-problem kernels) and (3, 1, 24, 2) (the MODEL mode of
# mpcqp_duo.hip); variant 1 (everything per problem, padded strides: the export with bounds) and 3 (e shared: both exports)
MODEL_CASES = tuple((shape, variant) for shape in OL.MODEL_SHAPES + ((3, 1, 24, 2),) for variant in (1, 3))
DIFF_VARIANT = "diff"
MODEL_DIFF_SHAPE = OL.DIFF_SHAPES[0]


def shared_mixed(B, N, mk, rng=None, row=None):
    """the parts of `mixed` that a shared constraint block can express (the same mask for every problem): step N // 2 padded
    whole and row 0 of step 0. A random quarter per problem and a problem padded whole cannot exist in a shared model: its C
    and D are one block for all problems, and the header promises nothing for a non-zero row with e = 1e30."""
    mask = np.zeros((B, N, mk), dtype=bool)
    mask[:, N // 2] = True
    mask[:, 0, 0] = True
    return mask


MODEL_MASKS = dict(tail=tail, mixed=shared_mixed, rows=rows)
# (shape, variant, placement) -> j: the case is drawn with seed base + 1000 j, the first j = 0, 1, ... at which it meets the
# conditions (first_model_choice(); tests/test_padded_rows_cpu.py runs the search again). Not listed: j = 0.
MODEL_CHOICE = {
    # `mixed` pads only mk + 1 of the N mk rows: at j = 0 too few of the nine plans rest on one of them
    ((3, 1, 16, 2), 1, "mixed"): 2,
    ((3, 1, 24, 2), 3, "mixed"): 3,
    ((3, 2, 8, 2), "diff", "tail"): 1,  # (at j = 0 the padding moves five of the nine plans)
}


def build_model_case(shape, variant, placement, j):
    nx, nu, N, mk = shape
    if variant == DIFF_VARIANT:  # the shared-model derivative exports: e shared, everything else per problem
        lay, seed = dict(OL.model_layout(3), x0="b", goal="b", targets="b"), 3900 + shape[0] + DRAW
    else:
        lay, seed = OL.model_layout(variant), 3000 + 10 * variant + shape[0] + DRAW
    w0, full0 = OL.make(shape, "cd", True, lay, seed + 1000 * j, 0.2)
    mask = MODEL_MASKS[placement](BATCH, N, mk)
    full = pad_rows(full0, mask)
    w = dict(w0)
    w["C"], w["D"] = full["C"][:1].copy(), full["D"][:1].copy()
    w["e"] = np.array(w0["e"], dtype=np.float64)
    w["e"][mask[:w["e"].shape[0]]] = PAD
    return dict(shape=shape, w=w, full=full, unpadded=full0, mask=mask.reshape(BATCH, N * mk), bound=1e-7,
                route=dict(f32=False, shape=shape), placement=placement, shared=True)


_MODEL = {}


def model_case(shape, variant, placement="tail"):
    """a shared-model case (operand_layouts.model_case: A, B, C, D shared and per step) with padded rows IN THE MODEL, in the
    placement `tail`, `rows` or `mixed` (its shareable form, shared_mixed): the mask is the same for every problem, so that C
    and D stay shared; e holds 1e30 on the padded rows, per problem or shared. Made once."""
    key = (shape, variant, placement)
    if key not in _MODEL:
        _MODEL[key] = build_model_case(shape, variant, placement, MODEL_CHOICE.get(key, 0))
    return _MODEL[key]


def first_model_choice(shape, variant, placement, most=40):
    for j in range(most):
        if serves(conditions(build_model_case(shape, variant, placement, j), with_cond=False)):
            return j
    return None


def diff_case(shape):
    """a derivative case (operand_layouts.diff_case, everything per problem and per step) in the `tail` placement"""
    nx, nu, N, mk = shape
    long = N > 40
    w0, full0 = OL.make(shape, "cd", True, _PER_STEP, (15000 if long else 5000 + N) + DRAW, 0.5, contractive=long)
    mask = tail(BATCH, N, mk)
    return dict(shape=shape, w=pad_rows(w0, mask), full=pad_rows(full0, mask), unpadded=full0, mask=mask.reshape(BATCH, N * mk),
                bound=1e-8, route=dict(f32=False, shape=shape), placement="tail")


# ragged host problems: (12, 2, 16, 4), the Python layer's batch (condensed: 32 variables, 64 rows), and (3, 1, 24, 2); both `tail`
RAGGED = ("mid-size fused", ON_CHIP_FUSED[0])


def ragged_problems(c):
    """the problems of a `tail` case as host MPCProblems with per-step LISTS of different heights (step k: 1 + k % mk rows), the
    reference's own way of stating them; BatchMPCProblem.from_problems pads them back to the case's operands"""
    from qpmpc_amd import MPCProblem

    nx, nu, N, mk = c["shape"]
    u = c["unpadded"]
    out = []
    for b in range(BATCH):
        keep = [k % mk + 1 for k in range(N)]
        assert all(not c["mask"][b, k * mk:k * mk + keep[k]].any() and c["mask"][b, k * mk + keep[k]:(k + 1) * mk].all() for k in range(N))
        p = MPCProblem([u["A"][b, k] for k in range(N)], [u["B"][b, k] for k in range(N)],
                       None if u["C"] is None else [u["C"][b, k, :keep[k]] for k in range(N)],
                       None if u["D"] is None else [u["D"][b, k, :keep[k]] for k in range(N)],
                       [u["e"][b, k, :keep[k]] for k in range(N)], N, u["wt"], u["wx"], u["wu"], initial_state=u["x0"][b],
                       goal_state=None if u["goal"] is None else u["goal"][b])
        if u["targets"] is not None:
            p.update_target_states(u["targets"][b])
        out.append(p)
    return out


# warm pairs: two `tail` problems of one shape. "operator": the second has the first's matrices and bounds and another x0 (the
# contract of MPCQP_WARM_OPERATOR); "active_set": the second is another draw altogether (MPCQP_WARM_ACTIVE_SET: everything may
# have changed), and the first's active row ids, moved down by warm_shift = mk, must land on padded rows of the second.
WARM_SHAPES = {  # name -> (shape, rows, stage, margin, seed)
    "small": ((3, 1, 16, 2), "c", False, 0.2, 24000),
    "pair generic": ((4, 2, 8, 2), "cd", True, 0.2, 1000),
    "narrow": ((3, 1, 24, 2), "cd", True, 0.2, 1000),
    "wide": ((6, 2, 20, 3), "cd", True, 0.2, 1000),
}
WARM_TS = (1.0, 0.5, 0.25) + tuple(0.25 * 0.75 ** k for k in range(1, 9))


def _warm_first(name):
    shape, rws, stage, margin, seed = WARM_SHAPES[name]
    r = OL.route(shape, rws, stage, margin=margin, seed=seed)
    return r, build_case(r, "tail", DRAW, None)


def warm_pair(name, kind, t=None):
    """(first, second) cases of a warm pair. kind "operator": x0 of the second is x0 + t (roll(x0, 1) - x0) with t the first of
    WARM_TS at which the stripped reference solves all nine (WARM_T); kind "active_set": the draw one seed further."""
    r, first = _warm_first(name)
    if kind == "active_set":
        return first, build_case(r, "tail", DRAW + 1, None)
    t = WARM_T[name] if t is None else t
    second = dict(first)
    for key in ("w", "full", "unpadded"):
        d = dict(first[key])
        d["x0"] = d["x0"] + t * (np.roll(d["x0"], 1, axis=0) - d["x0"])
        second[key] = d
    return first, second


WARM_T = {"small": WARM_TS[-1], "pair generic": 1.0, "narrow": 1.0, "wide": 1.0}  # (state rows only: step 0 bounds C_0 x0 itself)


def first_warm_t(name):
    for t in WARM_TS:
        _, second = warm_pair(name, "operator", t)
        if (stripped(second["full"], second["mask"])[2] == 0).all():
            return t
    return None


def shifted_onto_padding(first, second, shift):
    """per item: does an active row id of the first problem's stripped reference, minus `shift`, name a padded row of the second?"""
    lam = reference(first)[1]
    hit = np.zeros(BATCH, dtype=bool)
    for b in range(BATCH):
        ids = np.flatnonzero(lam[b] > 1e-9) - shift
        ids = ids[ids >= 0]
        hit[b] = bool(second["mask"][b, ids].any())
    return hit
