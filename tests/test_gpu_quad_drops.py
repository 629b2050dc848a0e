"""GPU tests (-m gpu): the four-per-wavefront kernel (csrc/mpcqp_quad.hip) computes, BIT FOR BIT, what it computed before its
active-set loops finished a non-plain trip once (the steady loop hands the trip it leaves to the general loop), dropped the leaving
slot inside the partial step's own trip and went back to the steady loop -- on problems that drop.

tests/golden/quad_drops_parent.npz (tools/gen_golden_quad_drops.py) holds the operands of three small problem sets and the plans,
multipliers, statuses and iteration counts recorded on an MI355X from the build of the parent commit: the shared-model mode on the
humanoid model, the lean build (3, 1, 16, 2) on the mixed family, the general build (4, 1, 12); the lean set again tiled to 4100 (the
slim LDS carve: every tile must repeat the recorded bits) and under the iteration limit that falls on the trip right after a partial
step. Every row performs the same floating-point operations in the same order as before, so the tolerance is zero: raw bits, the
sign of a zero included. What the sets contain is asserted without a GPU by tests/test_quad_drops_cpu.py."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_drops_parent.npz")
_CACHE = {}


def _fixture():
    import tools.gen_golden_quad_drops as G

    if not _CACHE:
        _CACHE["sets"], _CACHE["results"], _CACHE["max_iter"] = G.unpack(np.load(GOLDEN))
    return G, _CACHE["sets"], _CACHE["results"], _CACHE["max_iter"]


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if a.tobytes() != b.tobytes():
        raw = np.dtype(f"u{a.dtype.itemsize}")
        bad = np.flatnonzero((a.view(raw) != b.view(raw)).reshape(len(a), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} problems differ from the parent's bits, first {bad[:8].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["model", "lean16", "gen12", "lean16_slim", "lean16_mi"])
def test_outputs_are_the_parents_bit_for_bit(name):
    pytest.importorskip("torch")
    G, sets, results, max_iter = _fixture()
    got = G.run_set(name, sets, max_iter)
    want = results[name]
    if name == "lean16_slim":  # (4100 problems, 64 distinct ones: every tile is held to the recorded bits)
        assert len(got[0]) == G.SLIM_BATCH
        want = tuple(np.concatenate([v] * (G.SLIM_BATCH // 64 + 1))[: G.SLIM_BATCH] for v in want)
    for k, a, b in zip(G.OUTPUTS, got, want):
        _same_bits(a, b, f"{name}: {k}")
