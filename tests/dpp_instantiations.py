"""The kernels that carry hand-written v_fmac_f64_dpp (fmac_bcast of qpmpc_amd/csrc/mpcqp_lane.h) and the launch that reaches each
(test helper: NumPy and the compiler only, no GPU).

The wait states in front of a hand-written DPP instruction are kept by the source (dpp_ready), and what the register allocator puts
between the two differs per template instantiation: an instantiation nobody launches is guarded by nothing. census() lists, from the
gfx950 assembly of the five units, every kernel that holds such an instruction; MANIFEST maps each to the recipe that selects it --
entry point, shape, rows, cost, flags, batch as a function of the device's SIMD count, and the launcher function that decides --;
tests/test_dpp_instantiations_cpu.py holds the two to each other and the recipes' inputs to the conditions that make a green GPU case
mean something; tests/test_gpu_dpp_instantiations.py runs one case per recipe.

unit_asm() compiles a unit once per process (the units take up to minutes each): the hazard scan of tests/test_host_api.py and the
census read the same text."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

UNITS = ("mpcqp_pair.hip", "mpcqp_quad.hip", "mpcqp_quadw.hip", "mpcqp_quadg.hip", "mpcqp_quadgw.hip")


# ---------------------------------------------------------------------------------------------- the census
@functools.lru_cache(maxsize=None)
def unit_asm(unit: str) -> str:
    """gfx950 assembly of qpmpc_amd/csrc/<unit>, compiled once per process"""
    import tools.check_dpp_hazards as chk

    return chk.device_asm(os.path.join(ROOT, "qpmpc_amd", "csrc", unit))


def all_asm() -> dict:
    """{unit: assembly} of the five units, compiled side by side the first time"""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        return dict(zip(UNITS, pool.map(unit_asm, UNITS)))


def demangle(symbol: str):
    """'mpcqp_quad_kernel<16, false, 1, true, false, true>' of _ZN5mpcqp17mpcqp_quad_kernelILi16ELb0ELi1ELb1ELb0ELb1EEEv...: the
    name as a kernel trace prints it (namespace dropped), for a function template of namespace mpcqp whose arguments are integers
    and booleans; None for any other symbol."""
    m = re.match(r"_ZN5mpcqp(\d+)", symbol)
    if not m:
        return None
    start = m.end()
    name, rest = symbol[start:start + int(m.group(1))], symbol[start + int(m.group(1)):]
    if not rest.startswith("I"):
        return name if rest.startswith("E") else None
    args, pos = [], 1
    while not rest.startswith("E", pos):
        a = re.match(r"L([ib])(n?)(\d+)E", rest[pos:])
        if not a:
            return None
        args.append(("true" if a.group(3) != "0" else "false") if a.group(1) == "b" else ("-" if a.group(2) else "") + a.group(3))
        pos += a.end()
    return f"{name}<{', '.join(args)}>"


def census_of(asm: str) -> dict:
    """{kernel name: number of hand-written v_fmac_f64_dpp} of one assembly text, kernels without any left out"""
    out, func = {}, None
    for raw in asm.split("\n"):
        line = raw.split(";")[0].strip()
        if line.endswith(":") and not line.startswith("."):
            func = line[:-1]
        elif func is not None and line.startswith("v_fmac_f64_dpp"):
            out[func] = out.get(func, 0) + 1
    named = {}
    for symbol, count in out.items():
        name = demangle(symbol)
        assert name is not None and name not in named, symbol
        named[name] = count
    return named


def census() -> dict:
    """{kernel name: (unit, hand-written v_fmac_f64_dpp)} over the five units"""
    out = {}
    for unit, asm in all_asm().items():
        for name, count in census_of(asm).items():
            assert name not in out, name
            out[name] = (unit, count)
    return out


# ---------------------------------------------------------------------------------------------- the recipes
# A recipe: entry "solve" (solve_mpc_batch; the checks "seeded" and "warm" pass it a WarmState) or "model" (SharedModel.prepare(...)
# .launch(): matrices shared, bounds per problem); shape (nx, nu, N, mk); rows "c" / "d" / "cd" (state rows, an input box, both); stage:
# with a stage cost; tight: the generator's tightness (those of tests/test_gpu_quad.py: 3.0, 0.2, 0.1, 0.05); flags: _capi.OPT_*
# names; batch: SMALL problems, or a name of BATCHES -- a function of simds = 4 * compute units --; check: what the GPU case holds
# (see tests/test_gpu_dpp_instantiations.py); site: "<file of csrc/>:<launcher function>", the function that selects the instantiation.
SMALL = 37  # a ragged last wavefront at four and at two problems per wavefront, ten / nineteen wavefronts
BATCHES = {
    # more wavefronts than SIMDs (mpcqp_quad.hip: slim = waves > device_simds_now()), a ragged last wavefront
    "slim": lambda simds: 4 * simds + 5,
    # four rows per lane: more than three wavefronts per compute unit (mpcqp_quadg.hip: waves > 3 * (simds / 4))
    "slim4": lambda simds: 3 * simds + 5,
    # the pair kernel's one_round window, 2 simds - 8 < ceil(batch / 2) <= 2 simds: an odd number of wavefronts (the last workgroup's
    # second wavefront is idle) and an odd batch (the last wavefront's second half is idle)
    "window": lambda simds: 4 * simds - 3,
}
ORACLE_HEAD, ORACLE_TAIL = 256, 64  # of a large launch the oracle checks the first 256 and the last 64 (the ragged wavefront)


def batch_of(recipe, simds: int) -> int:
    b = recipe["batch"]
    return b if isinstance(b, int) else BATCHES[b](simds)


def oracle_subset(batch: int) -> np.ndarray:
    """the problems of a launch the oracle is run on: all of a small one, the first 256 and the last 64 of a large one"""
    if batch <= ORACLE_HEAD + ORACLE_TAIL:
        return np.arange(batch)
    return np.concatenate([np.arange(ORACLE_HEAD), np.arange(batch - ORACLE_TAIL, batch)])


def _r(entry, shape, rows, stage, tight, seed, site, check="oracle", flags=(), batch=SMALL):
    return dict(entry=entry, shape=shape, rows=rows, stage=stage, tight=tight, seed=seed, site=site, check=check, flags=tuple(flags),
                batch=batch)


def _unreachable(site, quote, why):
    """site: the function that refuses the launch; quote: the source text of the rule, verbatim (once in that file)"""
    return dict(unreachable=True, site=site, quote=quote, why=why)


def function_text(source: str, function: str) -> list:
    """the lines of the one definition of `function` in a source text, from its signature to the closing brace in column 0
    (a declaration ends in a semicolon, a call is indented or names template arguments); [] if there is not exactly one"""
    lines = source.split("\n")
    starts = [i for i, s in enumerate(lines) if re.match(r"(?!//)\S.*\b" + function + r"\(", s) and not s.rstrip().endswith(";")]
    if len(starts) != 1 or "}" not in lines[starts[0]:]:
        return []
    return lines[starts[0]: lines.index("}", starts[0]) + 1]


QUAD_T, QUAD_MODEL, QUADG_T = "mpcqp_quad.hip:launch_quad_t", "mpcqp_quad.hip:launch_quad_model", "mpcqp_quadg.hip:launch_quadg_t"
PAIR_T, PAIR_MODEL = "mpcqp_pair.hip:launch_pair_t", "mpcqp_pair.hip:launch_pair_model"
FOUR, TWO = "OPT_FOUR_PER_WAVE", "OPT_TWO_PER_WAVE"
# one shape per compiled size of the general build of mpcqp_quad.hip (nx = 7 .. 16 run the padded sizes 8, 12, 16)
GENERAL = {2: ((2, 1, 16, 2), "d", False), 3: ((3, 1, 16, 2), "c", True), 4: ((4, 2, 8, 2), "cd", True), 5: ((5, 1, 16, 2), "cd", True),
           6: ((6, 2, 8, 2), "cd", True), 8: ((8, 2, 8, 2), "cd", True), 12: ((12, 4, 4, 2), "c", False), 16: ((16, 1, 16, 2), "cd", True)}
LEAN = {2: (2, 1, 16, 2), 3: (3, 1, 16, 2), 4: (4, 1, 16, 2)}
FOUR_ROWS = {2: (2, 1, 16, 4), 3: (3, 1, 16, 4), 4: (4, 1, 16, 4), 8: (8, 4, 4, 8)}
MODEL_SHAPE = (3, 1, 16, 2)
PAIR = {(3, 0): ((3, 1, 16, 2), "cd", True), (3, 2): ((3, 1, 16, 2), "c", False), (4, 0): ((4, 2, 8, 2), "cd", True),
        (4, 2): ((4, 1, 16, 2), "c", False)}


def _b(x: bool) -> str:
    return "true" if x else "false"


def _manifest() -> dict:
    M = {}
    seed = iter(range(7000, 8000))
    # mpcqp_quad_kernel<NX, ORDER, 1, SLIM, MODEL, GEN> -- the general build, both LDS carves
    for nx, (shape, rows, stage) in GENERAL.items():
        M[f"mpcqp_quad_kernel<{nx}, false, 1, false, false, true>"] = _r("solve", shape, rows, stage, 0.2, next(seed), QUAD_T)
        M[f"mpcqp_quad_kernel<{nx}, false, 1, true, false, true>"] = _r("solve", shape, rows, stage, 0.2, next(seed), QUAD_T,
                                                                      check="slim", batch="slim")
    # ... the lean build: natural order / pairing order, roomy / slim carve
    for nx, shape in LEAN.items():
        M[f"mpcqp_quad_kernel<{nx}, false, 1, false, false, false>"] = _r("solve", shape, "c", False, 0.2, next(seed), QUAD_T,
                                                                        flags=[FOUR])
        M[f"mpcqp_quad_kernel<{nx}, false, 1, true, false, false>"] = _r("solve", shape, "c", False, 0.05, next(seed), QUAD_T,
                                                                       check="slim", batch="slim")
        if nx == 2:  # an order is refused unless the pair kernel could take the launch, and that kernel has nx = 3, 4 only
            why = "MpcqpSolveOpts.order needs pair_eligible(MODE_FUSED), which asks for nx == 3 or 4 (pair_eligible of mpcqp_pair.hip): nx = 2 with an order is MPCQP_EUNSUPPORTED"
            rule = "if (ka.order && (ka.warm_state || (fl & (MPCQP_OPT_FORCE_LDS | MPCQP_OPT_ONE_PER_WAVE | MPCQP_OPT_SEED_VIOLATED)) || !pairs())) return MPCQP_EUNSUPPORTED;"
            M["mpcqp_quad_kernel<2, true, 1, false, false, false>"] = _unreachable("mpcqp_capi.hip:refusal", rule, why)
            M["mpcqp_quad_kernel<2, true, 1, true, false, false>"] = _unreachable("mpcqp_capi.hip:refusal", rule, why)
            continue
        M[f"mpcqp_quad_kernel<{nx}, true, 1, false, false, false>"] = _r("solve", shape, "c", False, 0.2, next(seed), QUAD_T,
                                                                       check="order", flags=[FOUR])
        M[f"mpcqp_quad_kernel<{nx}, true, 1, true, false, false>"] = _r("solve", shape, "c", False, 0.2, next(seed), QUAD_T,
                                                                      check="order", batch="slim")
    # ... the shared model (one instantiation for every nx)
    for order in (False, True):
        for slim in (False, True):
            M[f"mpcqp_quad_kernel<3, {_b(order)}, 1, {_b(slim)}, true, false>"] = _r(
                "model", MODEL_SHAPE, "cd", True, 0.2, next(seed), QUAD_MODEL,
                check="order" if order else "slim" if slim else "oracle", flags=[FOUR], batch="slim" if slim else SMALL)
    # mpcqp_quadg_kernel<NX, 4, SLIM>: four rows per lane (more than 32 rows, or more than four per step)
    for nx, shape in FOUR_ROWS.items():
        M[f"mpcqp_quadg_kernel<{nx}, 4, false>"] = _r("solve", shape, "cd", True, 0.2, next(seed), QUADG_T)
        M[f"mpcqp_quadg_kernel<{nx}, 4, true>"] = _r("solve", shape, "cd", True, 0.2, next(seed), QUADG_T, check="slim", batch="slim4")
    # mpcqp_pair_kernel<NX, MK, MODEL, WARM, WPB, SEED, ORDER>
    for (nx, mk), (shape, rows, stage) in PAIR.items():
        k = f"mpcqp_pair_kernel<{nx}, {mk}, false, "
        M[k + "false, 1, false, false>"] = _r("solve", shape, rows, stage, 0.2, next(seed), PAIR_T, flags=[TWO])
        M[k + "false, 1, false, true>"] = _r("solve", shape, rows, stage, 0.2, next(seed), PAIR_T, check="order", flags=[TWO])
        M[k + "false, 2, false, false>"] = _r("solve", shape, rows, stage, 0.2, next(seed), PAIR_T, check="two", flags=[TWO],
                                             batch="window")
        M[k + "false, 1, true, false>"] = _r("solve", shape, rows, stage, 0.2, next(seed), PAIR_T, check="seeded")
        M[k + "true, 1, false, false>"] = _r("solve", shape, rows, stage, 0.2, next(seed), PAIR_T, check="warm")
    k = "mpcqp_pair_kernel<3, 0, true, false, "
    M[k + "1, false, false>"] = _r("model", MODEL_SHAPE, "cd", True, 0.2, next(seed), PAIR_MODEL, flags=[TWO])
    M[k + "1, false, true>"] = _r("model", MODEL_SHAPE, "cd", True, 0.2, next(seed), PAIR_MODEL, check="order", flags=[TWO])
    M[k + "2, false, false>"] = _r("model", MODEL_SHAPE, "cd", True, 0.2, next(seed), PAIR_MODEL, check="two", flags=[TWO],
                                  batch="window")
    return M


MANIFEST = _manifest()
REACHABLE = [k for k, r in MANIFEST.items() if not r.get("unreachable")]


# ---------------------------------------------------------------------------------------------- the inputs
def _general_family(rng, batch, nx, nu, N, tight, rows, stage, mk):
    """tests/test_gpu_quad.py::_general_family (with rows "c" and no stage cost: its _lean_family without the time-invariant
    option), restated here so that the CPU tests do not import a GPU module"""
    from qpmpc_amd.workloads import random_ltv

    w = random_ltv(rng, batch, nx, nu, N, mk, tight)
    if rows == "c":
        w["D"] = None
    elif rows == "d":  # an input box per step: e > 0 keeps u = 0 feasible
        w["C"] = None
        w["e"] = tight * (0.05 + 0.5 * np.abs(rng.standard_normal(w["e"].shape)))
    if not stage:
        w["wx"] = w["targets"] = None
    return w


def _share_model(w, rng, tight):
    """the family with the first problem's A, B, C, D for everybody ([1, N, ...]: what SharedModel asks for) and e per problem,
    recomputed on the shared matrices so that u = 0 stays feasible: e[b, k] = C[k] x_free[b, k] + tight (0.05 + 0.5 |N(0, 1)|)"""
    w = dict(w)
    for X in ("A", "B", "C", "D"):
        w[X] = np.ascontiguousarray(w[X][:1])
    B, N = w["x0"].shape[0], w["N"]
    e = np.empty_like(w["e"])
    for b in range(B):
        x = w["x0"][b].copy()
        for k in range(N):
            e[b, k] = w["C"][0, k] @ x + tight * (0.05 + 0.5 * np.abs(rng.standard_normal(e.shape[2])))
            x = w["A"][0, k] @ x
    w["e"] = e
    return w


_FAMILIES = {}


def family(name: str, simds: int):
    """the workload of a recipe at a device of `simds` SIMDs, drawn once"""
    r = MANIFEST[name]
    key = (name, simds)
    if key not in _FAMILIES:
        rng = np.random.default_rng(r["seed"])
        nx, nu, N, mk = r["shape"]
        w = _general_family(rng, batch_of(r, simds), nx, nu, N, r["tight"], r["rows"], r["stage"], mk)
        _FAMILIES[key] = _share_model(w, rng, r["tight"]) if r["entry"] == "model" else w
    return _FAMILIES[key]


_PER_PROBLEM = ("A", "B", "C", "D", "e", "x0", "goal", "targets")


def take(w, index, materialise=False):
    """the problems `index` (a slice or an index array) of a workload; materialise: operands shared by the batch ([1, ...]) are
    repeated per problem -- the oracle then sees plain per-problem operands"""
    batch = w["x0"].shape[0]
    count = len(np.arange(batch)[index])
    out = dict(w)
    for k in _PER_PROBLEM:
        v = w.get(k)
        if v is None:
            continue
        if v.shape[0] == batch:
            out[k] = np.ascontiguousarray(v[index])
        elif materialise:
            out[k] = np.ascontiguousarray(np.broadcast_to(v, (count,) + v.shape[1:]))
    return out


_ORACLE = {}


def oracle_on(name: str, simds: int):
    """(index, U, lam, status, iters) of the C oracle on the oracle-checked problems of a recipe, solved once"""
    import oracle

    key = (name, simds)
    if key not in _ORACLE:
        w = family(name, simds)
        index = oracle_subset(w["x0"].shape[0])
        _ORACLE[key] = (index,) + tuple(oracle.solve_workload(take(w, index, materialise=True)))
    return _ORACLE[key]
