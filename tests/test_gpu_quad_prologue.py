"""GPU tests (-m gpu): the prologue of the four-per-wavefront kernel (csrc/mpcqp_quad.hip: the operand loads of the build, requested
first and without branches; the chain, whose independent sums are issued round robin) computes, BIT FOR BIT, what the kernel computed
before these were rearranged.

tests/golden/quad_prologue_parent.npz (tools/gen_golden_quad_prologue.py) holds the operands of seventeen small problem sets and the
plans, multipliers, statuses and iteration counts recorded on an MI355X from the build of the parent commit. Every floating-point
instruction is kept and every sum keeps the order of its own terms, so the tolerance is zero: every output of every problem is compared
as raw bits (the sign of a zero included). The sets are the smallest shapes at which the rearranged code takes another path: the full
horizon with every operand at stride 0, with A per step and C time-invariant and the converse, behind padded batch strides; N = 1, 2 and
15 (the clamped loads); batches of 5 and 7 (idle rows); nx = 2 and 4 (four and six sums per step); the general build with one, three
and four rows per step, input rows and a stage cost, and with nx = 5 and 6 (three and four operand registers per step; at nx = 6 the
G rows are summed as a group of their own); and a tight set under a tolerance of 1e-15 in which, by the kernel's own probe, a problem
failed an acceptance test once and -- recorded from a probe build, see the generator -- a problem took the refinement arm. At most 32
problems per launch."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_prologue_parent.npz")
_CACHE = {}


def _fixture():
    import tools.gen_golden_quad_prologue as G

    if not _CACHE:
        _CACHE["sets"], _CACHE["results"], _CACHE["fails"], _CACHE["refinements"] = G.unpack(np.load(GOLDEN))
    return G, _CACHE["sets"], _CACHE["results"], _CACHE["fails"], _CACHE["refinements"]


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if a.tobytes() != b.tobytes():
        raw = np.dtype(f"u{a.dtype.itemsize}")
        bad = np.flatnonzero((a.view(raw) != b.view(raw)).reshape(len(a), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} problems differ from the parent's bits, first {bad[:8].tolist()}")


SHAPES = {  # set -> (nx, nu, N, mk, problems, general build)
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
    G, sets, results, fails, refinements = _fixture()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert set(G.SETS) == set(SHAPES) == set(results)
    for name, (nx, nu, N, mk, count, general) in SHAPES.items():
        w = sets[G.SETS[name]]
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
        for a, b in zip(results[name], results["tight16"]):
            assert a.tobytes() == b[:count].tobytes(), name
    assert refinements > 0
    assert fails.shape == (32,) and (fails > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_outputs_are_the_parents_bit_for_bit(name):
    pytest.importorskip("torch")
    G, sets, results, _, _ = _fixture()
    got = G.run_set(name, sets)
    for k, a, b in zip(G.OUTPUTS, got, results[name]):
        _same_bits(a, b, f"{name}: {k}")


@pytest.mark.gpu
def test_the_probe_still_shows_the_failed_acceptance_test():
    """The tight set under the developer probe: the outputs are the recorded ones, and the probe's record of failed acceptance tests
    (slot 14) names the recorded problems. (The refinement mark exists only in a probe build: the stored count is the generator's.)"""
    pytest.importorskip("torch")
    G, sets, results, fails, _ = _fixture()
    res = G.solve(sets["tight16"], probe=True, feas_tol=G.TIGHT_TOL)
    for k, a, b in zip(G.OUTPUTS, res, results["tight16"]):
        _same_bits(a, b, f"tight16 under the probe: {k}")
    assert np.array_equal(G.fails_of(res[4]), fails)
