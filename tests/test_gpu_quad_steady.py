"""GPU tests (-m gpu): the four-per-wavefront kernel's steady loop (csrc/mpcqp_quad.hip: plain active-set trips in a loop of one basic
block in front of the general loop) computes, BIT FOR BIT, what the kernel computed before it had one.

tests/golden/quad_steady_parent.npz (tools/gen_golden_quad_steady.py) holds the operands of a few small problem sets and the plans,
multipliers, statuses and iteration counts recorded on an MI355X from the build of the parent commit. The steady loop performs the
same floating-point operations in the same order as the general loop's plain arm, so the tolerance is zero: every output of every
problem is compared as raw bits (the sign of a zero included). The sets: the lean build at N = 16 (64 problems, and cut to five: idle
rows), at N = 9 (a partly populated second register row), under max_iter = 5 (the limit exit), tiled to 4100 problems (the slim LDS
carve; recorded separately, every tile must repeat the same bits), the general build (4, 1, 12) with input rows and a stage cost, and
the shared-model mode on the humanoid model. The 64 problems mix tight, loose and inconsistent rows inside every wavefront -- rows
that leave the steady loop at different trips and for different reasons: test_the_fixture_mixes_the_wavefronts re-asserts that from
the stored arrays (no GPU)."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_steady_parent.npz")
_CACHE = {}


def _fixture():
    import tools.gen_golden_quad_steady as G

    if not _CACHE:
        _CACHE["sets"], _CACHE["results"] = G.unpack(np.load(GOLDEN))
    return G, _CACHE["sets"], _CACHE["results"]


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if a.tobytes() != b.tobytes():
        raw = np.dtype(f"u{a.dtype.itemsize}")
        bad = np.flatnonzero((a.view(raw) != b.view(raw)).reshape(len(a), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} problems differ from the parent's bits, first {bad[:8].tolist()}")


def test_the_fixture_is_small_and_mixes_the_wavefronts():
    """The recorded outputs of the 64-problem set show every kind of row the steady loop has to hand over: solved without a trip,
    solved after a drop, inconsistent, stopped by the iteration limit; at least four wavefronts whose rows end with different
    statuses and four where one row runs four or more trips longer than the other three."""
    G, sets, results = _fixture()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert G.conditions(*results["lean16"]) == []
    assert len(sets["lean16"]["x0"]) == 64 and sets["lean16"]["N"] == 16 and sets["lean9"]["N"] == 9 and sets["gen12"]["N"] == 12
    assert sets["gen12"]["D"] is not None and sets["gen12"]["wx"] is not None and sets["gen12"]["targets"] is not None
    assert (results["lean16_mi5"][2] == 1).sum() >= 8 and results["lean16_mi5"][3].max() == 5
    for name in G.SETS:
        assert len(results[name][0]) == {"lean16_cut5": 5, "lean9": 32, "gen12": 32, "model": 32}.get(name, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lean16", "lean16_cut5", "lean16_mi5", "lean16_slim", "lean9", "gen12", "model"])
def test_outputs_are_the_parents_bit_for_bit(name):
    pytest.importorskip("torch")
    G, sets, results = _fixture()
    got = G.run_set(name, sets)
    want = results[name]
    if name == "lean16_slim":  # (4100 problems, 64 distinct ones: every tile is held to the recorded bits)
        assert len(got[0]) == G.SLIM_BATCH
        want = tuple(np.concatenate([v] * (G.SLIM_BATCH // 64 + 1))[: G.SLIM_BATCH] for v in want)
    for k, a, b in zip(G.OUTPUTS, got, want):
        _same_bits(a, b, f"{name}: {k}")
