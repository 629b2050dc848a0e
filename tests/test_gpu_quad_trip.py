"""GPU tests (-m gpu): the steady loop of the four-per-wavefront kernel (csrc/mpcqp_quad_steady.h) with its flags as lane-mask
arithmetic, one trip counter for the iteration limit and nq = n, and status, iters and nq rebuilt behind the loop computes, BIT FOR BIT,
what the parent commit's loop computed.

tests/golden/quad_trip_parent.npz (tools/gen_golden_quad_trip.py) holds U, lam, status and iters recorded on an MI355X from the parent's
build for seven small launches: ten lean problems whose rows leave a wavefront's loop on different trips, the same under max_iter = 1, 2
and 8 (the limit met inside the loop by some rows and not others), ten problems at n = 9 of which some reach nq = n, eight of which
every second is not positive definite (done on entry), and the ten tiled to one wavefront more than the device has SIMDs (slim carve).
The change touches no floating-point operation, so the tolerance is zero: raw bits, the sign of a zero included.
tests/test_quad_trip_cpu.py holds the inputs to those conditions without a GPU."""
import numpy as np
import pytest

_CACHE = {}


def _fixture():
    import tools.gen_golden_quad_trip as G

    if not _CACHE:
        _CACHE["sets"], _CACHE["recorded"] = G.inputs(), G.load()
    return G, _CACHE["sets"], _CACHE["recorded"]


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if a.tobytes() != b.tobytes():
        raw = np.dtype(f"u{a.dtype.itemsize}")
        bad = np.flatnonzero((a.view(raw) != b.view(raw)).reshape(len(a), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} problems differ from the parent's bits, first {bad[:8].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "a_mi1", "a_mi2", "a_mi8", "c", "d", "a_slim"])
def test_outputs_are_the_parents_bit_for_bit(name):
    pytest.importorskip("torch")
    G, sets, recorded = _fixture()
    got = G.run_launch(name, sets)
    want = recorded[name]
    if name == "a_slim":  # (every tile is held to the ten recorded results)
        count = G.slim_batch()
        assert len(got[0]) == count
        want = tuple(np.concatenate([v] * (count // 10 + 1))[:count] for v in want)
    for k, a, b in zip(G.OUTPUTS, got, want):
        _same_bits(a, b, f"{name}: {k}")
