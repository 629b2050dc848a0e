"""Operand layouts for the addressing contract of include/mpcqp.h (test helper, NumPy only, no GPU).

Every operand of a problem is addressed as ptr + b*batch_stride + k*step_stride, and each of A, B, C, D, e may on its own be

    "bn"  per problem, per step          "b1"  per problem, time-invariant (step_stride 0)
    "1n"  shared (batch_stride 0), per step   "11"  shared and time-invariant,

goal and targets "b" (per problem) or "1" (shared); so may x0 in the shared-model exports. LAYOUTS is a fixed list of such
assignments, PADS the batch-stride padding of the odd-numbered ones, make() the workload generator, ROUTES the forward launches
tests/test_gpu_operand_layouts.py runs each layout through, and diff_case / model_case / condense_case the inputs of its other
tests; tests/test_operand_layouts_cpu.py holds all of these inputs to the conditions that make a green GPU test mean something
(every problem solved, most with a binding row, blocks that differ, a reference that can be trusted at the bound).

The cyclic part of the list: layout i gives operand X the form OPTS[(i*s_X + o_X + t_X[i // 4]) % 4]. Without t the formula
has period 4 (every s is odd), so twelve layouts would be four, three times over, and operands of equal s would move in
lockstep; the per-cycle shifts t_X (none in the first cycle) make the twelve distinct and give every pair of operands more
than four joint forms, while each block of four still gives every operand every form once (every form three times in all)."""
from __future__ import annotations

import numpy as np

OPTS = ("bn", "b1", "1n", "11")
MATS = ("A", "B", "C", "D", "e")
_CYCLE = dict(A=(1, 0, (0, 0, 0)), B=(1, 1, (0, 1, 2)), C=(3, 2, (0, 1, 1)), D=(1, 3, (0, 2, 3)), e=(3, 1, (0, 2, 0)))  # (s, o, t)
BATCH = 9  # a ragged last wavefront at four and at two problems per wavefront, and more than one wavefront


def _cyclic(i: int) -> dict:
    lay = {X: OPTS[(i * s + o + t[i // 4]) % 4] for X, (s, o, t) in _CYCLE.items()}
    lay["goal"] = "b1"[i % 2]
    lay["targets"] = "b1"[(i // 2) % 2]
    return lay


def _by_hand(A, B, C, D, e, goal, targets) -> dict:
    return dict(A=A, B=B, C=C, D=D, e=e, goal=goal, targets=targets)


# appended by hand, so that the properties coverage() names hold whatever the cyclic part happens to contain: the fused constraint
# layout of mpcqp_stagew.hip (C and D both time-invariant) with e per step, shared and per problem; A LTI with B per step and
# the reverse (the two arguments of fits_on_chip), here with everything per problem
LAYOUTS = [_cyclic(i) for i in range(12)] + [
    _by_hand("bn", "b1", "11", "b1", "bn", "1", "b"),
    _by_hand("b1", "bn", "b1", "11", "1n", "b", "1"),
]

# elements past the packed batch stride, a different amount per operand, odd ones among them (they break every alignment); D stays
# packed among padded operands. Layout 13 is the odd-numbered one whose goal is per problem.
PADS = dict(A=2, B=3, C=7, D=0, e=5, x0=1, goal=6, targets=9)


def pads_of(i: int):
    """batch-stride padding (elements per operand) of layout i: the odd-numbered ones are padded, the even ones packed"""
    return dict(PADS) if i % 2 else 0


def time_invariant(form: str) -> bool:
    return form[1] == "1"


def coverage(layouts=None) -> dict:
    """the properties the list must have, each as the list of layouts that have it"""
    L = LAYOUTS if layouts is None else layouts
    ti = time_invariant
    return {
        "C and D time-invariant, e per step": [i for i, l in enumerate(L) if ti(l["C"]) and ti(l["D"]) and not ti(l["e"])],
        "exactly one of C, D time-invariant": [i for i, l in enumerate(L) if ti(l["C"]) != ti(l["D"])],
        "A time-invariant, B per step": [i for i, l in enumerate(L) if ti(l["A"]) and not ti(l["B"])],
        "A per step, B time-invariant": [i for i, l in enumerate(L) if not ti(l["A"]) and ti(l["B"])],
    }


def _reduce(a, form, how="slice"):
    """[B, N, ...] to the stored shape [1|B, 1|N, ...] of `form`: the first block of a shared axis, or the maximum over it"""
    if form[0] == "1":
        a = a[:1] if how == "slice" else a.max(axis=0, keepdims=True)
    if form[1] == "1":
        a = a[:, :1] if how == "slice" else a.max(axis=1, keepdims=True)
    return np.ascontiguousarray(a)


def make(shape, rows, stage, layout, seed, margin, contractive=False):
    """(w, full): BATCH problems of qpmpc_amd.workloads.random_ltv in layout `layout` (an index into LAYOUTS or a dict). `w` is
    the workload dict with every operand in its stored shape [1|B, 1|N, ...] (goal, targets [1|B, ...]); `full` states the same
    problems with every operand materialised to [B, N, ...] and [B, ...]. rows "c" / "d" / "cd": state rows, an input box or both;
    stage: with a stage cost. e is recomputed on the materialised operands so that u = 0 stays feasible for every problem:
    e[b, k] = C[b, k] x_free[b, k] + margin (0.05 + 0.5 |N(0, 1)|), reduced by max over the axes the layout shares for e.
    contractive: every drawn A block is replaced by 0.98 times its orthogonal QR factor and B is divided by sqrt(nx), the
    dynamics of BASELINE config 5 (qpmpc_amd.workloads.synthetic_ltv_batch) -- see LONG below."""
    from qpmpc_amd.workloads import random_ltv

    nx, nu, N, mk = shape
    lay = LAYOUTS[layout] if isinstance(layout, int) else layout
    rng = np.random.default_rng(seed)
    drawn = random_ltv(rng, BATCH, nx, nu, N, mk, margin)
    if contractive:
        drawn["A"] = 0.98 * np.linalg.qr(drawn["A"])[0]
        drawn["B"] = drawn["B"] / np.sqrt(nx)
    w = dict(drawn)
    full = dict(drawn)
    for X in ("A", "B", "C", "D"):
        w[X] = _reduce(drawn[X], lay[X])
        full[X] = np.ascontiguousarray(np.broadcast_to(w[X], drawn[X].shape))
    for X, width in (("x0", nx), ("goal", nx), ("targets", N * nx)):  # (x0 is per problem unless the layout says otherwise)
        w[X] = np.ascontiguousarray(drawn[X][:1] if lay.get(X, "b") == "1" else drawn[X])
        full[X] = np.ascontiguousarray(np.broadcast_to(w[X], (BATCH, width)))
    slack = margin * (0.05 + 0.5 * np.abs(rng.standard_normal((BATCH, N, mk))))
    if rows == "d":
        e = slack
    else:
        e = np.empty((BATCH, N, mk))
        for b in range(BATCH):
            x = full["x0"][b].copy()
            for k in range(N):
                e[b, k] = full["C"][b, k] @ x + slack[b, k]
                x = full["A"][b, k] @ x
    w["e"] = _reduce(e, lay["e"], "max")
    full["e"] = np.ascontiguousarray(np.broadcast_to(w["e"], e.shape))
    for d in (w, full):
        if rows == "c":
            d["D"] = None
        elif rows == "d":
            d["C"] = None
        if not stage:
            d["wx"] = d["targets"] = None
    return w, full


def ltv(seed, B, nx, nu, N, mk, tight=1.0, rows="cd", stage=True):
    """qpmpc_amd.workloads.random_ltv; rows "c" / "d" / "cd": state rows, an input box or both; stage: with a stage cost (the
    workloads of tests/test_gpu_memory_discipline.py, here so that a CPU test can state the same problems)"""
    from qpmpc_amd.workloads import random_ltv

    rng = np.random.default_rng(seed)
    w = random_ltv(rng, B, nx, nu, N, mk, tight)
    if rows == "c":
        w["D"] = None
    elif rows == "d":
        w["C"] = None
        w["e"] = tight * (0.05 + 0.5 * np.abs(rng.standard_normal(w["e"].shape)))
    if not stage:
        w["wx"] = w["targets"] = None
    return w


# ---------------------------------------------------------------------------------------------- the forward launches
# name -> (shape (nx, nu, N, mk), rows, stage cost, MpcqpSolveOpts flag names, float32, stage-wise entry point, margin, seed base):
# the routes, flags and smallest shapes of tests/test_gpu_memory_discipline.py, whose docstrings say why each is the smallest
# that reaches its kernel. Layout i of a route is make(shape, rows, stage, i, seed base + i, margin); margin and seed base are
# tuned on the CPU oracle (tests/test_operand_layouts_cpu.py: every problem solved, at least 6 of 9 with a binding row).
def route(shape, rows="cd", stage=True, flags=(), f32=False, stagewise=False, margin=0.2, seed=1000, contractive=False):
    return dict(shape=shape, rows=rows, stage=stage, flags=tuple(flags), f32=f32, stagewise=stagewise, margin=margin, seed=seed,
                contractive=contractive)


_route = route


# The long horizons (the float32 wide stage-wise kernel at n > 160 and the dense HBM path at BASELINE config 5's shape, that of
# tests/test_gpu_memory_discipline.py::test_dense_hbm_path) draw CONTRACTIVE dynamics. random_ltv's A = I + 0.08 N(0, 1) has a
# spectral radius of ~1.3 at nx = 12: held time-invariant over 48 steps it gives the condensed Hessian a condition number of
# 1e12 .. 1e16 (1e5 per step-varying A), and over 64 steps the oracle calls two of nine problems infeasible whatever the seed.
# The float64 oracle's own error, ~ cond(P) * 2.2e-16, is then far above the bounds these routes are held to, and the float32
# dense path (which squares the conditioning) misses 1e-3 on every layout for the same reason: no verdict on a kernel's
# addressing could be read off such a case. With config 5's own dynamics cond(P) stays below 1e5 in every layout
# (tests/test_operand_layouts_cpu.py holds every case to cond(P) * 2.2e-16 <= a tenth of its bound).
LONG = dict(contractive=True)
DENSE = (12, 4, 64, 16)

ROUTES = {
    "quad lean": _route((3, 1, 16, 2), "c", False, ["OPT_FOUR_PER_WAVE"], seed=24000),
    "quad general, registers": _route((6, 2, 8, 2), "cd", True, ["OPT_FOUR_PER_WAVE"]),
    "quad general, streamed": _route((12, 4, 4, 2), "c", False, ["OPT_FOUR_PER_WAVE"], seed=2000),
    "quadg (3, 1, 16, 4)": _route((3, 1, 16, 4), flags=["OPT_FOUR_PER_WAVE"]),
    "quadg (8, 4, 4, 8)": _route((8, 4, 4, 8), flags=["OPT_FOUR_PER_WAVE"]),
    "pair lean": _route((3, 1, 16, 2), "c", False, ["OPT_TWO_PER_WAVE"], seed=24000),
    "pair generic": _route((4, 2, 8, 2), "cd", True, ["OPT_TWO_PER_WAVE"]),
    "one per wavefront": _route((4, 2, 8, 3), flags=["OPT_ONE_PER_WAVE"]),
    "workgroup (LDS)": _route((4, 2, 10, 3), flags=["OPT_FORCE_LDS"]),
    "mid-size fused": _route((12, 2, 16, 4), flags=["OPT_FORCE_CONDENSED"]),
    "narrow stage-wise": _route((3, 1, 24, 2)),
    "narrow stage-wise, stage-wise entry": _route((3, 1, 24, 2), stagewise=True),
    "wide stage-wise f64": _route((6, 2, 20, 3)),
    "wide stage-wise f64, stage-wise entry": _route((6, 2, 20, 3), flags=["OPT_STAGE_WIDE"], stagewise=True),
    "wide stage-wise f32": _route((12, 4, 48, 4), f32=True, **LONG),
    "general stage-wise": _route((20, 6, 10, 4)),
    "dense HBM f64": _route(DENSE, flags=["OPT_FORCE_CONDENSED"], **LONG),
    "dense HBM f64, G in the workspace": _route(DENSE, flags=["OPT_FORCE_CONDENSED", "OPT_FORCE_GWS"], **LONG),
    "dense HBM f64, dense G": _route(DENSE, flags=["OPT_FORCE_CONDENSED", "OPT_FORCE_DENSE_G"], **LONG),
    "dense HBM f32": _route(DENSE, flags=["OPT_FORCE_CONDENSED"], f32=True, **LONG),
    "dense HBM f32, G in the workspace": _route(DENSE, flags=["OPT_FORCE_CONDENSED", "OPT_FORCE_GWS"], f32=True, **LONG),
    "dense HBM f32, dense G": _route(DENSE, flags=["OPT_FORCE_CONDENSED", "OPT_FORCE_DENSE_G"], f32=True, **LONG),
    "promoted f32 (3, 1, 16, 2)": _route((3, 1, 16, 2), f32=True, seed=2000),
    "promoted f32 (6, 2, 20, 3)": _route((6, 2, 20, 3), f32=True),
}


def f32_view(w):
    """the operands a float32 launch sees (float32 storage), as float64 arrays for the references"""
    return {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in w.items()}


_MADE = {}


def route_case(route: str, layout: int):
    """(w, full) of layout `layout` of route `route`, made once (routes of equal shape, rows, cost, margin and seed share them);
    a float32 route gets the float32-rounded operands, which is what its launch stores"""
    r = ROUTES[route]
    key = (r["shape"], r["rows"], r["stage"], r["margin"], r["seed"], r["contractive"], layout, r["f32"])
    if key not in _MADE:
        w, full = make(r["shape"], r["rows"], r["stage"], layout, r["seed"] + layout, r["margin"], r["contractive"])
        _MADE[key] = (f32_view(w), f32_view(full)) if r["f32"] else (w, full)
    return key, _MADE[key]


_SOLVED = {}


def oracle_on_full(route: str, layout: int):
    """(U, lam, status) of the C oracle on the MATERIALISED problems of a case, solved once"""
    import oracle

    key, (_, full) = route_case(route, layout)
    if key not in _SOLVED:
        _SOLVED[key] = oracle.solve_workload(full)[:3]
    return _SOLVED[key]


# ---------------------------------------------------------------------------------------------- the other tests' inputs
# derivative and condensing exports: two packed, four padded, so that every operand but D meets a padded batch stride (1: e, 13: goal)
DIFF_LAYOUTS = (0, 1, 3, 5, 10, 13)
DIFF_SHAPES = ((3, 2, 8, 2), (3, 2, 70, 2))
CONDENSE_SHAPE = (4, 2, 10, 3)


def diff_case(shape, layout):
    """(w, full) of a derivative case; the long horizon draws contractive dynamics for the reason LONG gives: held time-invariant
    over 70 steps, random_ltv's A takes cond(P) to 1e9 .. 1e13, and the NumPy restatements (dense solves with P) are then
    1e-7 .. 1e-3 off on single items, far above the 1e-8 the exports are held to"""
    if shape[2] > 40:  # (seed base tuned like those of ROUTES: 630 blocks of e with two entries each must all differ)
        return make(shape, "cd", True, layout, 15000 + layout, 0.5, contractive=True)
    return make(shape, "cd", True, layout, 5000 + layout + shape[2], 0.5)


def condense_case(layout):
    return make(CONDENSE_SHAPE, "cd", True, layout, 6000 + layout, 0.2)


# shared-model solves: x0, goal, targets and e each shared or per problem; the odd-numbered variants padded
MODEL_VARIANTS = [dict(x0="b", goal="b", targets="b", e="b"), dict(x0="b", goal="b", targets="b", e="b"),
                  dict(x0="1", goal="b", targets="1", e="b"), dict(x0="b", goal="1", targets="1", e="1"),
                  dict(x0="b", goal="b", targets="1", e="1"), dict(x0="1", goal="1", targets="b", e="b"),
                  dict(x0="b", goal="1", targets="b", e="1"), dict(x0="b", goal="b", targets="1", e="1")]
MODEL_PADS = dict(x0=1, goal=4, targets=9, e=5)
MODEL_SHAPES = ((3, 1, 16, 2), (4, 2, 8, 3))


def model_pads(variant):
    return dict(MODEL_PADS) if variant % 2 else dict.fromkeys(MODEL_PADS, 0)


def model_layout(variant):
    v = MODEL_VARIANTS[variant]
    return dict(A="1n", B="1n", C="1n", D="1n", e=v["e"] + "n", x0=v["x0"], goal=v["goal"], targets=v["targets"])


def model_case(shape, variant):
    """(w, full) of a shared-model case: A, B, C, D shared and per step"""
    return make(shape, "cd", True, model_layout(variant), 3000 + 10 * variant + shape[0], 0.2)
