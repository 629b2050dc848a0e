"""Inputs of the stream-contract tests (tests/test_gpu_streams.py); test helper, NumPy only, no GPU. tests/test_stream_cases_cpu.py
holds these inputs, on the C oracle, to the conditions that make a green GPU test mean something.

The GPU tests tell a launch that ran in stream order from one that ran ahead of (or without) the work queued before it by the
DATA it saw: every route has two sets of initial states, x0_A (what the arena loads) and x0_B (copied over x0_A on the stream,
right before the launch). Matrices, bounds, goal and targets are those of A. A launch, or a graph replay, that read x0 before
the copy landed returns A's plans; the conditions below make A's and B's plans differ, item by item, by at least ten times the
bound the plans are held to.

ROUTES_UNDER_TEST: every route of operand_layouts.ROUTES at layout 1 (a padded layout: strides are in play) and the two on-chip
routes for 17 .. 32 variables, at the smallest shape of onchip32_cases.SHAPES (nine problems of operand_layouts.make in layout 1,
flagged MPCQP_OPT_ON_CHIP_32) and of onchip32_model_cases.SHAPES (variant 1: everything per problem, padded; bounds per problem).

x0_B = x0_A + t (roll(x0_A, 1, axis=0) - x0_A) with t the first of TS at which, on the oracle (float32 routes: on the
float32-rounded operands, x0_B included),

  * all nine B problems are solved (e stays A's, so a B problem may well be infeasible),
  * at least six of the nine have a binding row (a multiplier above 1e-9),
  * for every item max |U_B - U_A| / max(1, max |U_A|) >= 10 x the route's bound (1e-7 float64, 1e-3 float32).

T records that t per route. operand_layouts.make draws the bounds e around the free response of x0_A (e_k = C_k x_k + a slack of
0.01 .. 0.3), which another x0 far from x0_A breaks -- with state rows only, step 0 bounds C_0 x0 itself, whatever the inputs
do --, so eleven routes meet the conditions at none of TS. Five of them get x0_B from a second seed of operand_layouts.make
(SECOND_SEED: the first of SEEDS = 90000 .. 90399 whose x0 meets the conditions, first_seed()). For the lean (3, 1, 16, 2) pair,
quadg (3, 1, 16, 4) and the mid-size kernel none of SEEDS serves (tests/test_stream_cases_cpu.py runs the search again), and t
goes on down the finer sequence FINER = 0.25 (3/4)^k, k = 1, 2, ... to the first that serves: the t that keep a B problem
feasible are an interval around 0, and the CPU test shows the value in front of the recorded one infeasible. The six dense HBM
routes (DENSE: two sets of problems) go down FINER too, WITHOUT a seed search: a try is an oracle solve of nine problems of 256
variables and 1024 rows, 400 of them are half an hour, and a draw of x0 is as far from x0_A as t = 1, where all nine problems
are infeasible (at 0.5 and 0.25: eight). The conditions themselves are the same for every route."""
from __future__ import annotations

import functools
import os

import numpy as np

import onchip32_cases as OC
import onchip32_model_cases as MC
import operand_layouts as OL

LAYOUT = 1
TS = (1.0, 0.5, 0.25)
BOUND = {False: 1e-7, True: 1e-3}  # by route["f32"]: the bounds of tests/test_gpu_operand_layouts.py
SEPARATION = 10.0
MIN_BINDING = 6

ON_CHIP_FUSED, ON_CHIP_MODEL = "on-chip 32 fused", "on-chip 32 shared model"
ON_CHIP_FUSED_SHAPE, ON_CHIP_FUSED_KIND, _ = OC.SHAPES[0]
ON_CHIP_MODEL_SHAPE, MODEL_VARIANT = MC.SHAPES[0][0], 1
assert ON_CHIP_FUSED_KIND == "lean" and OL.MODEL_VARIANTS[MODEL_VARIANT] == dict(x0="b", goal="b", targets="b", e="b")

# name -> the route: the dicts of operand_layouts.ROUTES; the fused on-chip route stated the same way (lean: state rows, terminal
# cost only); the shared-model route has no flags (bounds per problem past 16 variables: only the on-chip kernel serves them)
ROUTES_UNDER_TEST = dict(OL.ROUTES)
ROUTES_UNDER_TEST[ON_CHIP_FUSED] = OL.route(ON_CHIP_FUSED_SHAPE, "c", False, ["OPT_ON_CHIP_32"], seed=OC.LAYOUT_SEED,
                                             margin=OC.LAYOUT_MARGIN)
ROUTES_UNDER_TEST[ON_CHIP_MODEL] = dict(shape=ON_CHIP_MODEL_SHAPE, f32=False, model=True, variant=MODEL_VARIANT)

FINER = tuple(0.25 * 0.75 ** k for k in range(1, 17))
DENSE = ("dense HBM f64", "dense HBM f64, G in the workspace", "dense HBM f64, dense G", "dense HBM f32",
          "dense HBM f32, G in the workspace", "dense HBM f32, dense G")
# route -> t (see above)
T = {
    "quad lean": FINER[1], "pair lean": FINER[1],  # (the same problems)
    "quad general, registers": 1.0,
    "quadg (3, 1, 16, 4)": FINER[7],
    "quadg (8, 4, 4, 8)": 0.25,
    "pair generic": 1.0,
    "one per wavefront": 0.25,
    "mid-size fused": FINER[4],
    "wide stage-wise f64": 0.5, "wide stage-wise f64, stage-wise entry": 0.5,
    "wide stage-wise f32": 1.0,
    "general stage-wise": 1.0,
    **dict.fromkeys(DENSE, FINER[4]),
    "promoted f32 (3, 1, 16, 2)": 0.25,
    ON_CHIP_FUSED: 0.25,
    ON_CHIP_MODEL: 1.0,
}
# route -> seed of the operand_layouts.make draw whose x0 is x0_B, for routes that no t of TS serves
SECOND_SEED = {
    "quad general, streamed": 90025,
    "workgroup (LDS)": 90094,
    "narrow stage-wise": 90000, "narrow stage-wise, stage-wise entry": 90000,
    "promoted f32 (6, 2, 20, 3)": 90012,
}


def is_model(name: str) -> bool:
    return bool(ROUTES_UNDER_TEST[name].get("model"))


def bound(name: str) -> float:
    return BOUND[bool(ROUTES_UNDER_TEST[name]["f32"])]


@functools.lru_cache(maxsize=None)
def case_a(name: str):
    """(w, full) of a route's A problems: the stored (layout 1) and the materialised operands"""
    r = ROUTES_UNDER_TEST[name]
    if is_model(name):
        return MC.case(r["shape"], r["variant"])
    if name in OL.ROUTES:
        return OL.route_case(name, LAYOUT)[1]
    return OL.make(r["shape"], r["rows"], r["stage"], LAYOUT, r["seed"] + LAYOUT, r["margin"], r["contractive"])


def x0_b(name: str, t=None):
    """x0_B of a route [9, nx] (float32 routes: float32 values held in float64, as operand_layouts.f32_view)"""
    r = ROUTES_UNDER_TEST[name]
    a = case_a(name)[0]["x0"]
    assert a.shape == (OL.BATCH, r["shape"][0])
    if t is None and name in SECOND_SEED:
        return x0_of_seed(name, SECOND_SEED[name])
    t = T[name] if t is None else t
    b = a + t * (np.roll(a, 1, axis=0) - a)
    return b.astype(np.float32).astype(np.float64) if r["f32"] else b


@functools.lru_cache(maxsize=None)
def case_b(name: str, t=None):
    """(w, full) of a route's B problems: A's with x0_B"""
    w, full = (dict(d) for d in case_a(name))
    w["x0"] = full["x0"] = x0_b(name, t)
    return w, full


_SOLVED = {}


def reference(name: str, which: str, t=None):
    """(U, lam, status) of the C oracle on the materialised A or B problems of a route, solved once (routes of equal shape, rows,
    cost, margin, seed and dtype share their problems, and then their x0_B)"""
    import oracle

    problems = OL.route_case(name, LAYOUT)[0] if name in OL.ROUTES else name
    key = (problems, which) + (() if which == "A" else (SECOND_SEED.get(name), T.get(name)) if t is None else (None, t))
    if key not in _SOLVED:
        _SOLVED[key] = oracle.solve_workload((case_a(name) if which == "A" else case_b(name, t))[1])[:3]
    return _SOLVED[key]


# The oracle takes 2 .. 3 s for nine problems of the dense HBM shape, and a GPU case needs A's and B's plans: they are recorded
# (tests/golden/stream_dense_reference.npz, written by `PYTHONPATH=. python tests/stream_cases.py`), tests/test_stream_cases_cpu.py holds the
# record to the oracle on every run, and the GPU tests read the record.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_dense_reference.npz")
RECORDED = {"f64": DENSE[0], "f32": DENSE[3]}  # (the two sets of problems of the six dense routes)


def plan_reference(name: str, which: str):
    """(U, status) of the oracle on a route's A or B problems, as the GPU tests compare against: solved on the spot, except for
    the dense HBM routes, whose plans are read from the record"""
    if name in DENSE:
        tag = "f32" if ROUTES_UNDER_TEST[name]["f32"] else "f64"
        with np.load(GOLDEN) as z:
            return z[f"{tag}_{which}_U"], z[f"{tag}_{which}_status"]
    U, _, st = reference(name, which)
    return U, st


def record_dense():
    out = {}
    for tag, name in RECORDED.items():
        for which in "AB":
            U, _, st = reference(name, which)
            out[f"{tag}_{which}_U"], out[f"{tag}_{which}_status"] = U, st
    np.savez_compressed(GOLDEN, **out)


def separation(Ua, Ub):
    """per item max |U_B - U_A| / max(1, max |U_A|)"""
    return np.abs(Ub - Ua).max(axis=1) / np.maximum(1.0, np.abs(Ua).max(axis=1))


def _judge(name, solved_a, solved_b):
    (Ua, _, sta), (Ub, lamb, stb) = solved_a, solved_b
    failed = []
    if not (sta == 0).all():
        failed.append(f"A statuses {sta.tolist()}")
    if not (stb == 0).all():
        return failed + [f"B statuses {stb.tolist()}"]
    binding = int((lamb > 1e-9).any(axis=1).sum())
    if binding < MIN_BINDING:
        failed.append(f"{binding} of {OL.BATCH} B problems have a binding row")
    sep = separation(Ua, Ub)
    if not (sep >= SEPARATION * bound(name)).all():
        failed.append(f"separation {sep.min():.2e} below {SEPARATION * bound(name):.0e}")
    return failed


def conditions(name: str, t=None):
    """what x0_B (at t; None: the recorded one) fails of the conditions above, as a list of strings (empty: all met)"""
    return _judge(name, reference(name, "A"), reference(name, "B", t))


SEEDS = range(90000, 90400)  # the second seeds tried, in this order


def x0_of_seed(name: str, seed: int):
    """x0 of the operand_layouts.make draw `seed` at a route's shape, as the route stores it"""
    r = ROUTES_UNDER_TEST[name]
    b = OL.make(r["shape"], r["rows"], r["stage"], LAYOUT, seed, r["margin"], r["contractive"])[0]["x0"]
    return b.astype(np.float32).astype(np.float64) if r["f32"] else b


def first_seed(name: str):
    """the first seed of SEEDS whose x0 meets the conditions as x0_B, or None (one oracle solve of nine problems per seed)"""
    import oracle

    for seed in SEEDS:
        full = dict(case_a(name)[1])
        full["x0"] = x0_of_seed(name, seed)
        if not _judge(name, reference(name, "A"), oracle.solve_workload(full)[:3]):
            return seed
    return None


def first_t(name: str):
    """the first t of TS that meets the conditions, or None"""
    return next((t for t in TS if not conditions(name, t)), None)


# ---------------------------------------------------------------------------------------------- stateful launch pairs
# the two pairs tests/test_gpu_memory_discipline.py runs eagerly (test_narrow_stagewise_keep_then_reuse_factor and
# test_cold_launch_with_a_warm_state_then_a_warm_launch), at its shapes: `ltv` are the arguments of its ltv(); `first` and
# `second` the launches (flag names of qpmpc_amd._capi, the warm-start mode by name, the buffers the second launch keeps)
SEQUENCES = {
    "keep then reuse factor": dict(ltv=(830, 5, 3, 1, 24, 2, 1.0, "cd", True), warm=False,
                                   first=dict(flags=("OPT_KEEP_FACTOR",), warm_start=None),
                                   second=dict(flags=("OPT_REUSE_FACTOR",), warm_start=None), carried="ws"),
    "cold with a warm state, then warm": dict(ltv=(870, 5, 3, 1, 16, 2, 0.3, "c", False), warm=True,
                                              first=dict(flags=(), warm_start=None),
                                              second=dict(flags=(), warm_start="WARM_OPERATOR"), carried="warm"),
}

# ---------------------------------------------------------------------------------------------- one instantiation, two LDS sizes
# the workgroup kernel (MPCQP_OPT_FORCE_LDS) in float64 with n > 32: mpcqp_lds_kernel<double, 4, MODE_FUSED> whatever the shape;
# (nx, nu, N, mk) -> mpcqp_lds_bytes, all above 48 KiB (the launcher sets MaxDynamicSharedMemorySize to the launch's own size)
# and below the 160 KiB of a CU. tests/test_stream_cases_cpu.py asks the library for the figures.
LDS_48K = 48 * 1024
LDS_SHAPES = {(4, 2, 28, 3): 127520, (4, 2, 24, 3): 95504, (4, 2, 20, 3): 68096}
_PER_STEP = dict(A="bn", B="bn", C="bn", D="bn", e="bn", goal="b", targets="b")  # (A and B per step: the image mpcqp_lds_bytes prices)


@functools.lru_cache(maxsize=None)
def lds_case(shape):
    """nine problems of operand_layouts.make at a shape of LDS_SHAPES, every operand per problem and per step"""
    return OL.make(shape, "cd", True, _PER_STEP, 8000 + shape[2], 0.2)[0]


if __name__ == "__main__":
    record_dense()
