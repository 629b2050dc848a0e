"""GPU tests (-m gpu): the four-per-wavefront kernel (csrc/mpcqp_quad.hip) computes, BIT FOR BIT, what earlier builds of it computed.

Four fixtures, tests/golden/quad_{trip,steady,drops,prologue}_parent.npz, each recorded on an MI355X from the build of the commit
before one rearrangement of the kernel that kept every floating-point operation and the order of every sum: the steady loop's lane
masks and single trip counter (trip); the steady loop itself, plain trips in one basic block (steady); a non-plain trip finished once,
the drop inside the partial step's trip, the return to the steady loop (drops); the operand loads first, the chain's sums round
robin (prologue). So the tolerance is zero: U, lam, status and iters of every problem are compared as raw bits, the sign of a zero
included. Each generator (tools/gen_golden_quad_<fixture>.py) says what its launches are and why, in a table of launches that this file
runs through tools/quad_parent_bits.py; a tiled launch (more wavefronts than SIMDs: the slim LDS carve) is held, every tile of it,
to the distinct results stored. What the fixtures contain is asserted without a GPU: below for steady and prologue, by
tests/test_quad_trip_cpu.py and tests/test_quad_drops_cpu.py for the other two."""
import importlib
import os

import numpy as np
import pytest

import tools.quad_parent_bits as H

FIXTURES = ("trip", "steady", "drops", "prologue")
_CACHE = {}


def _generator(fixture):
    return importlib.import_module(f"tools.gen_golden_quad_{fixture}")


def _fixture(fixture):
    """(the generator, its launches, operand sets, recorded outputs and whatever else its file holds), loaded once"""
    if fixture not in _CACHE:
        _CACHE[fixture] = (_generator(fixture),) + tuple(_generator(fixture).fixture())
    return _CACHE[fixture]


CASES = [(fixture, name) for fixture in FIXTURES for name in _generator(fixture).SETS]


def test_the_fixture_is_small_and_mixes_the_wavefronts():
    """The recorded outputs of the 64-problem set show every kind of row the steady loop has to hand over: solved without a trip,
    solved after a drop, inconsistent, stopped by the iteration limit; at least four wavefronts whose rows end with different
    statuses and four where one row runs four or more trips longer than the other three."""
    G, _, sets, results = _fixture("steady")
    assert os.path.getsize(G.PATH) < 200 * 1024
    assert G.conditions(*results["lean16"]) == []
    assert len(sets["lean16"]["x0"]) == 64 and sets["lean16"]["N"] == 16 and sets["lean9"]["N"] == 9 and sets["gen12"]["N"] == 12
    assert sets["gen12"]["D"] is not None and sets["gen12"]["wx"] is not None and sets["gen12"]["targets"] is not None
    assert (results["lean16_mi5"][2] == 1).sum() >= 8 and results["lean16_mi5"][3].max() == 5
    for name in G.SETS:
        assert len(results[name][0]) == {"lean16_cut5": 5, "lean9": 32, "gen12": 32, "model": 32}.get(name, 64)


SHAPES = {  # set of the prologue fixture -> (nx, nu, N, mk, problems, general build)
    "shared16": (3, 1, 16, 2, 8, False), "a_step16": (3, 1, 16, 2, 5, False), "c_step16": (3, 1, 16, 2, 5, False),
    "tight16": (3, 1, 16, 2, 32, False), "tight16_pad": (3, 1, 16, 2, 16, False), "tight16_cut5": (3, 1, 16, 2, 5, False),
    "tight16_cut7": (3, 1, 16, 2, 7, False), "lean1": (3, 1, 1, 2, 8, False), "lean2": (3, 1, 2, 2, 8, False),
    "lean15": (3, 1, 15, 2, 8, False), "nx2": (2, 1, 16, 2, 8, False), "nx4": (4, 1, 16, 2, 8, False),
    "gen_mk1": (3, 1, 16, 1, 8, True), "gen_mk3": (3, 1, 10, 3, 8, True), "gen_mk4": (3, 1, 8, 4, 8, True),
    "gen_nx5": (5, 1, 16, 2, 4, True), "gen_nx6": (6, 1, 16, 2, 4, True),
}


def test_the_fixture_is_small_has_every_set_and_a_refinement():
    """Under 200 KB; every set with its shape, layout and number of problems; in the tight set the kernel's probe counted at least one
    problem in the refinement arm and at least one that failed an acceptance test once; every set but the smallest holds a solved
    problem with an active row."""
    G, launches, sets, results, fails, refinements = _fixture("prologue")
    assert os.path.getsize(G.PATH) < 200 * 1024
    assert set(G.SETS) == set(SHAPES) == set(results) == set(launches)
    for name, (nx, nu, N, mk, count, general) in SHAPES.items():
        w = sets[launches[name].on]
        U, lam, status, iters = results[name]
        assert w["N"] == N and w["x0"].shape[-1] == nx and w["B"].shape[-2:] == (nx, nu) and w["e"].shape[-1] == mk, name
        assert U.shape == (count, N * nu) and lam.shape == (count, N * mk) and status.shape == iters.shape == (count,), name
        assert count <= 64 and (general == (w["D"] is not None)) and (general == (w["wx"] is not None)), name
        assert (status == 0).any(), name
        if name != "lean1":
            assert ((status == 0) & (iters > 0)).any(), name
    assert all(sets["shared16"][k].ndim == (1 if k == "e" else 2) for k in ("A", "B", "C", "e"))  # one block each: every stride 0
    assert sets["a_step16"]["A"].shape[1] == 16 and sets["a_step16"]["C"].shape[1] == 1
    assert sets["c_step16"]["A"].shape[1] == 1 and sets["c_step16"]["C"].shape[1] == 16
    assert any(G.PADS[k] % 2 for k in G.PADS) and all(G.PADS[k] > 0 for k in G.PADS)
    for name, count in (("tight16_pad", G.PAD_COUNT), ("tight16_cut5", 5), ("tight16_cut7", 7)):  # (a row's arithmetic is its own)
        assert launches[name].cut == count and launches[name].on == "tight16"
        for a, b in zip(results[name], results["tight16"]):
            assert a.tobytes() == b[:count].tobytes(), name
    assert refinements > 0
    assert fails.shape == (32,) and (fails > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("fixture,name", CASES)
def test_outputs_are_the_parents_bit_for_bit(fixture, name):
    pytest.importorskip("torch")
    _, launches, sets, results = _fixture(fixture)[:4]
    spec, want = launches[name], results[name]
    got = H.run(spec, sets)
    if spec.tile:  # (every tile is held to the distinct results recorded)
        count = H.count_of(spec)
        assert len(got[0]) == count and len(want[0]) == spec.stored
        want = H.expand(want, count)
    for k, a, b in zip(H.OUTPUTS, got, want):
        H.same_bits(a, b, f"{fixture} {name}: {k}")


@pytest.mark.gpu
def test_the_probe_still_shows_the_failed_acceptance_test():
    """The prologue fixture's tight set under the developer probe: the outputs are the recorded ones, and the probe's record of failed
    acceptance tests (slot 14) names the recorded problems. (The refinement mark exists only in a probe build: the stored count is
    the generator's.)"""
    pytest.importorskip("torch")
    G, _, sets, results, fails, _ = _fixture("prologue")
    res = G.probed(sets)
    for k, a, b in zip(H.OUTPUTS, res, results["tight16"]):
        H.same_bits(a, b, f"tight16 under the probe: {k}")
    assert np.array_equal(G.fails_of(res[4]), fails)
