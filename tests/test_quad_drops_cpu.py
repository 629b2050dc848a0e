"""CPU tests of the fixture tests/golden/quad_drops_parent.npz (tools/gen_golden_quad_drops.py) and of the trip model
(tools/quad_trip_model.py) it was drawn with: no GPU, the stored arrays and the C oracle's condensing only.

The fixture holds the four-per-wavefront kernel (csrc/mpcqp_quad.hip) to the bits of the build before its loops finished a non-plain
trip once, dropped a slot inside the partial step's trip and went back to the steady loop (tests/test_gpu_quad_parent_bits.py). It can only
do that if its problems DO drop, in the arrangements those three changes treat differently: that is what is asserted here, on the
model's trips of the stored operands -- and the model is held to the recording: for every solved problem of every set its iteration
count is the one the kernel recorded."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_drops_parent.npz")
_CACHE = {}


def _fixture():
    import tools.gen_golden_quad_drops as G

    if not _CACHE:
        _, _CACHE["sets"], _CACHE["results"], _CACHE["max_iter"] = G.fixture()
        _CACHE["trips"] = G.model_trips(_CACHE["sets"])
    return G, _CACHE["sets"], _CACHE["results"], _CACHE["max_iter"], _CACHE["trips"]


def test_the_fixture_is_small_and_complete():
    G, sets, results, max_iter, _ = _fixture()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert len(sets["model"]["x0"]) == 64 and len(sets["lean16"]["x0"]) == 64 and len(sets["gen12"]["x0"]) == 32
    assert sets["lean16"]["N"] == 16 and sets["lean16"]["D"] is None and sets["gen12"]["N"] == 12
    assert sets["gen12"]["D"] is not None and sets["gen12"]["wx"] is not None and sets["gen12"]["targets"] is not None
    for name in G.SETS:
        U, lam, status, iters = results[name]
        assert len(U) == len(lam) == len(status) == len(iters) == (32 if name == "gen12" else 64)
    # the slim launch repeats the roomy one's problems: a row's arithmetic does not depend on its wavefront or its carve
    for a, b in zip(results["lean16"], results["lean16_slim"]):
        assert a.tobytes() == b.tobytes()


def test_the_models_iteration_counts_are_the_recorded_ones():
    G, sets, results, max_iter, _ = _fixture()
    assert G.model_disagreements(sets, results, max_iter) == []
    for name in G.SETS:
        assert (results[name][2] == 0).sum() >= len(results[name][2]) // 2, name  # (most problems of every set are solved ones)


def test_the_fixture_drops_where_the_loops_differ():
    """Six problems with a drop, two with two drops; a wavefront that drops within its first three trips and makes eight plain trips
    in a row afterwards (the return to the steady loop); two rows of one wavefront in partial steps in the same trip, and in
    consecutive trips; a row that drops while the other three rows of its wavefront are done."""
    G, _, _, _, trips = _fixture()
    assert G.conditions(trips) == []


def test_the_iteration_limit_falls_right_after_a_partial_step():
    G, sets, results, max_iter, trips = _fixture()
    best, rows = G.limit_after_partial(trips["lean16"])
    assert best == max_iter and rows >= 1
    hit = [b for b, (_, _, k) in enumerate(trips["lean16"]) if len(k) > max_iter and k[max_iter - 1] == "d"]
    assert len(hit) == rows
    status, iters = results["lean16_mi"][2], results["lean16_mi"][3]
    assert all(status[b] == 1 and iters[b] == max_iter for b in hit)


def test_the_model_on_a_problem_without_a_binding_row_and_on_an_inconsistent_one():
    import tools.quad_trip_model as TM

    M = np.array([[1.0, 0.0], [-1.0, 0.0]])
    assert TM.active_set(M, np.array([1.0, 1.0]), np.array([1.0, 1.0])) == (0, TM.SOLVED, "")
    assert TM.active_set(M, np.array([-1.0, 1.0]), np.array([-1.0, 1.0])) == (1, TM.SOLVED, "P")
    it, st, kinds = TM.active_set(M, np.array([-1.0, -1.0]), np.array([-1.0, -1.0]))  # x <= -1 and x >= 1
    assert st == TM.INFEASIBLE and kinds.endswith("I")
