"""CPU tests (no GPU) of the fixture tests/golden/quad_trip_parent.npz (tools/gen_golden_quad_trip.py) and of the steady loop's
instruction census.

The fixture's INPUTS are drawn from fixed seeds; what makes a bit-for-bit comparison of the steady loop (csrc/mpcqp_quad_steady.h)
mean something is held here with the C oracle and the kernel's trip model (tools/quad_trip_model.py) alone:
  * under each iteration limit of set a (1, 2, 8) some wavefront has a row that stops AT the limit next to a row that has finished --
    the limit is one per-row compare of the loop's trip counter, met by some rows of a wavefront and not by others;
  * a wavefront of set a has rows with three different trip counts (rows leave the loop's masks one after the other);
  * a row of set c reaches nq = n (the other half of the counter's limit);
  * every second problem of set d is not positive definite (done on entry) and the others solve;
  * every problem the recorded launches solved is solved by the oracle, to the same plan.
The census case finds the loop in the gfx950 assembly by what identifies it -- the innermost backward branch around 103 FMAs -- and
holds it to the parent's arithmetic (103 FMAs, 12 LDS instructions), to fewer instructions than the parent's 257, and to lane masks that
never pass through a 0/1 register."""
import os

import numpy as np
import pytest

import tools.gen_golden_quad_trip as G
from tools import quad_trip_model as TM

SOLVED, MAX_ITER, NOT_PD = 0, 1, 3
_CACHE = {}


def _inputs():
    if "sets" not in _CACHE:
        _CACHE["sets"] = G.inputs()
    return _CACHE["sets"]


def _oracle(name):
    import oracle

    if ("oracle", name) not in _CACHE:
        _CACHE["oracle", name] = oracle.solve_workload(_inputs()[name])
    return _CACHE["oracle", name]


def _model(name, max_iter=None):
    if ("model", name, max_iter) not in _CACHE:
        _CACHE["model", name, max_iter] = TM.trips_of_workload(_inputs()[name], max_iter=max_iter)
    return _CACHE["model", name, max_iter]


def _wavefronts(values):
    """the values of a launch by wavefront (idle rows of the last one left out)"""
    return [values[i:i + 4] for i in range(0, len(values), 4)]


def test_shapes_and_the_ragged_wavefront():
    s = _inputs()
    assert s["a"]["x0"].shape == (10, 3) and s["a"]["N"] == 16 and s["a"]["D"] is None and s["a"]["wx"] is None
    assert s["c"]["x0"].shape == (10, 3) and s["c"]["N"] == 9 and s["c"]["D"] is not None
    assert s["d"]["x0"].shape == (8, 3) and s["d"]["N"] == 16 and s["d"]["wt"] < 0.0 and s["d"]["D"] is None
    assert len(s["a"]["x0"]) % 4 == 2  # two idle rows in the last wavefront


@pytest.mark.parametrize("limit", G.LIMITS)
def test_the_limit_stops_some_rows_of_a_wavefront_and_not_others(limit):
    res = _model("a", limit)
    full = _model("a")
    hit = 0
    for wf, wf_full in zip(_wavefronts(res), _wavefronts(full)):
        stopped = [st == MAX_ITER and it == limit for it, st, _ in wf]
        finished = [st == SOLVED and it <= limit for it, st, _ in wf]
        assert all(a or b for a, b in zip(stopped, finished))
        # (a row that finishes inside the limit makes the trips it makes without one)
        assert all((it, st) == (f[0], f[1]) for (it, st, _), f, fin in zip(wf, wf_full, finished) if fin)
        hit += any(stopped) and any(finished)
    assert hit >= 1


def test_a_wavefront_has_rows_with_three_different_trip_counts():
    counts = [len({it for it, _, _ in wf}) for wf in _wavefronts(_model("a"))]
    assert max(counts) >= 3, counts


def test_a_row_reaches_nq_equal_n():
    n = _inputs()["c"]["N"]  # (nu = 1)
    best = []
    for _, st, kinds in _model("c"):
        assert st == SOLVED
        nq = top = 0
        for c in kinds:
            nq += {"P": 1, "F": 1, "d": -1}[c]
            top = max(top, nq)
        best.append(top)
    assert max(best) == n and min(best) < n, best


def test_every_second_problem_of_set_d_is_not_positive_definite():
    from oracle.capi import condense_one
    from qpmpc_amd.workloads import problem_from_workload

    w = _inputs()["d"]
    _, _, st, it = _oracle("d")
    assert st.tolist() == [SOLVED, NOT_PD] * 4
    assert (it[0::2] >= 8).all() and not it[1::2].any()  # (the rows next to a row that is done on entry make trips)
    # by a margin that no rounding decides: the smallest eigenvalue of P
    eig = [np.linalg.eigvalsh(condense_one(problem_from_workload(w, b))["P"])[0] for b in range(8)]
    assert min(eig[0::2]) > 0.5 * w["wu"] and max(eig[1::2]) < -1.0, eig


@pytest.mark.parametrize("name", ["a", "c"])
def test_the_oracle_solves_every_problem(name):
    _, _, st, _ = _oracle(name)
    assert (st == SOLVED).all()
    assert all(r[1] == SOLVED for r in _model(name))


def test_every_problem_the_recorded_launches_solved_is_solved_by_the_oracle():
    assert os.path.getsize(G.PATH) < 64 * 1024
    rec = G.load()
    sizes = {"c": 10, "d": 8}
    for name in G.LAUNCHES:
        U, lam, st, it = rec[name]
        src = name if name in ("c", "d") else "a"
        assert len(U) == sizes.get(name, 10) and U.dtype == np.float64 and st.dtype == np.int32
        Uo, _, sto, _ = _oracle(src)
        solved = st == SOLVED
        assert (sto[solved] == SOLVED).all(), name
        scale = np.maximum(1.0, np.abs(Uo).max(axis=1, keepdims=True))
        assert (np.abs(U - Uo) / scale)[solved].max() <= 1e-6, name
    # what the inputs were chosen for shows in the records: rows stopped at each limit next to rows that solved, rows done on entry
    for limit in G.LIMITS:
        st, it = rec[f"a_mi{limit}"][2], rec[f"a_mi{limit}"][3]
        assert any((s == MAX_ITER).any() and (s == SOLVED).any() for s in _wavefronts(st)), limit
        assert (it[st == MAX_ITER] == limit).all() and (it[st == SOLVED] <= limit).all()
    assert rec["d"][2].tolist() == [SOLVED, NOT_PD] * 4
    for k in range(4):
        assert rec["a_slim"][k].tobytes() == rec["a"][k].tobytes()


def test_steady_loop_census():
    """the headline instantiation's steady loop in the assembly of the unit (compiled once per session with the hazard scan's flags)"""
    import dpp_instantiations as DI
    from tools import quad_census as QC
    from tools import quad_steady_census as SC

    funcs = SC.functions(DI.unit_asm("mpcqp_quad.hip"))
    names = QC.demangle(list(funcs))
    seen = 0
    for mangled, insts in funcs.items():
        if "mpcqp_quad_kernel<" not in names[mangled]:
            continue
        c = SC.census(insts)
        assert c is not None, names[mangled]
        seen += 1
        assert c["classes"]["FMA"] == SC.STEADY_FMAS and c["classes"]["LDS"] == SC.STEADY_LDS, (names[mangled], c["classes"])
        assert c["total"] < SC.PARENT_TOTAL, (names[mangled], c["total"])
        assert c["round_trips"] == [], (names[mangled], [c["span"][i][1:] for i in c["round_trips"]])
        assert c["classes"]["global load"] == 0 and c["classes"]["global store"] == 0  # (one basic block of registers and LDS: no scratch)
    assert seen == 22  # every instantiation of the unit has the loop


def test_the_census_finds_a_round_trip_when_there_is_one():
    """(the detector on a hand-made span: a mask turned into 0/1 and compared again is found; a 0/1 that is also added is not)"""
    from tools import quad_steady_census as SC

    span = [(None, "v_cndmask_b32_e64", "v5, 0, 1, s[10:11]"), (None, "v_add_f64", "v[0:1], v[2:3], v[6:7]"),
            (None, "v_cmp_ne_u32_e64", "s[12:13], 0, v5"), (None, "v_mov_b32_e32", "v5, v9")]
    assert SC.round_trips(span) == [0]
    span[1] = (None, "v_add_u32_e32", "v8, v5, v8")
    assert SC.round_trips(span) == []
