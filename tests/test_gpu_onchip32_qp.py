"""GPU tests (-m gpu): mpcqp_solve_batch with MPCQP_OPT_ON_CHIP_32 -- the QP-given mode of csrc/mpcqp_duo.hip, dense QPs of up to 32
variables and 64 rows on chip, two problems per wavefront, no workspace (replacing qpsolvers.solve_problem at
qpmpc/solve_mpc.py:43). The inputs are those of tests/onchip32_qp_cases.py, held to their conditions on the C oracle by
tests/test_onchip32_qp_cpu.py. Every launch of the export goes through ctypes in the guarded arena of
tests/guarded_launch.py (QPs), the workspace pointer NULL.

Tolerances (float64): |x - x_ref|_inf <= 1e-7 max(1, |x_ref|_inf) against the C oracle, the project's bound for float64 dense QPs
(verdict_cases.DENSE_SIZES), and the same bound between two routes; multipliers on the clear items within 1e-7 (1 + max lam_ref)."""
import ctypes as C

import numpy as np
import pytest

import onchip32_qp_cases as QC
import verdict_cases as VC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers and comparisons; needs torch)
from guarded_launch import EUNSUPPORTED, QPs, _flag  # noqa: E402

OUTS = ("U", "lam", "status", "iters")


_CASES, _RUNS = {}, {}


def _case(n, m):
    if (n, m) not in _CASES:
        _CASES[(n, m)] = QPs(*QC.qps(n, m))
    return _CASES[(n, m)]


def _flagged(n, m):
    """outputs of the flagged launch of a size under fill 0xFF, made once"""
    if (n, m) not in _RUNS:
        _RUNS[(n, m)] = _case(n, m).run(GL.F, _flag())
    return _RUNS[(n, m)]


def _rel(x, ref):
    return float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))).max())


def _same_item(a, i, b, j, what):
    for k in OUTS:
        assert GL.same_bits(a[k][i], b[k][j]), (what, k, i, j)


# ---------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("size,why", QC.SIZES, ids=[str(s[0]) for s in QC.SIZES])
def test_oracle_parity_and_memory_discipline(size, why):
    """Flagged, workspace NULL: statuses verdict_cases.MIXED_STATUS, zeros for unsolved items, solved items within 1e-7 of the
    oracle, lam within 1e-7 (1 + max lam) on the clear items; fills 0x00 and 0xFF and two runs give equal bits; with lam, iters
    and status NULL the other outputs keep their bits and the NULL ones their fill; guards and operands intact (Launch.run)."""
    n, m = size
    c = _case(n, m)
    z1, z2, f = c.run(GL.Z, _flag()), c.run(GL.Z, _flag()), _flagged(n, m)
    GL.equal_outputs(z1, z2, f"{size}: run to run under fill Z")
    GL.equal_outputs(z1, f, f"{size}: fill Z against fill F")
    xo, lamo, sto, ito = QC.reference(n, m)
    assert np.array_equal(f["status"], VC.MIXED_STATUS), f["status"]
    ok = sto == 0
    bad = ~ok
    assert not np.isnan(f["U"]).any() and (f["U"][bad] == 0).all() and (f["lam"][bad] == 0).all()
    clear = QC.clear(n, m)
    err = _rel(f["U"][ok], xo[ok])
    dev = float((np.abs(f["lam"][clear] - lamo[clear]) / (1.0 + lamo[clear].max(axis=1, keepdims=True))).max())
    print(f"    {size}: x err {err:.2e}, lam dev {dev:.2e}, iters {f['iters'].tolist()} (oracle {ito.tolist()})")
    assert err <= QC.TOL and dev <= QC.TOL, (err, dev)
    assert np.array_equal(f["lam"][clear] > 0, lamo[clear] > 0)
    assert (f["iters"] >= 0).all() and (f["iters"] <= 10 * (n + m) + 10).all()
    nn = c.run(GL.F, _flag(), lam=False, iters=False, status=False)
    assert GL.holds(nn["lam"], GL.F) and GL.holds(nn["iters"], GL.F) and GL.holds(nn["status"], GL.F)
    bits_kept = [b for b in range(c.B) if not GL.same_bits(nn["U"][b], f["U"][b])]
    assert not bits_kept, (size, "x differs with lam, iters and status NULL", bits_kept)
    only_lam = c.run(GL.F, _flag(), lam=False)
    assert GL.holds(only_lam["lam"], GL.F)
    GL.equal_outputs(f, only_lam, f"{size}: lam NULL", lam=False)


# ---------------------------------------------------------------------------------------------- 2. a problem's bits are its own
def test_a_problems_bits_are_its_own():
    """(24, 48): every item launched alone (its wavefront's second half idle), and the batch reversed (another neighbour, the other
    half), give the bits the item had in the batch of nine."""
    n, m = 24, 48
    ref = _flagged(n, m)
    P, q, G, h = QC.qps(n, m)
    B = len(q)
    rev = QPs(P[::-1].copy(), q[::-1].copy(), G[::-1].copy(), h[::-1].copy()).run(GL.F, _flag())
    for b in range(B):
        _same_item(ref, b, rev, B - 1 - b, "reversed")
    for b in range(B):
        one = QPs(P[b:b + 1], q[b:b + 1], G[b:b + 1], h[b:b + 1]).run(GL.F, _flag())
        _same_item(ref, b, one, 0, "alone")


# ---------------------------------------------------------------------------------------------- 3. verdicts
def test_indefinite_item():
    """P[5][5] -= 50 on item 3 of (24, 48): status 3, iters 0, zeros (the oracle says (3, 0)); every other item keeps its bits"""
    n, m = 24, 48
    ref = _flagged(n, m)
    out = QPs(*QC.indefinite(n, m)).run(GL.F, _flag())
    b = QC.INDEFINITE_ITEM
    assert out["status"][b] == 3 and out["iters"][b] == 0 and (out["U"][b] == 0).all() and (out["lam"][b] == 0).all()
    for i in range(len(ref["status"])):
        if i != b:
            _same_item(ref, i, out, i, "next to an indefinite item")


def test_iteration_limit():
    """(24, 48) with max_iter the median of the flagged launch's own counts over its solved items: items at or below it keep their
    bits, the others have status 1, iters == max_iter and zeros."""
    n, m = 24, 48
    ref = _flagged(n, m)
    k = int(np.median(ref["iters"][ref["status"] == 0]))
    lo, hi = np.flatnonzero(ref["iters"] <= k), np.flatnonzero(ref["iters"] > k)
    print(f"    iters {ref['iters'].tolist()}, limit {k}: {len(lo)} at or below, {len(hi)} above")
    assert k >= 1 and len(lo) >= 2 and len(hi) >= 2
    lim = _case(n, m).run(GL.F, _flag(), max_iter=k)
    for i in lo:
        _same_item(ref, i, lim, i, "at or below the limit")
    assert (lim["status"][hi] == 1).all() and (lim["iters"][hi] == k).all(), (lim["status"], lim["iters"])
    assert (lim["U"][hi] == 0).all() and (lim["lam"][hi] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. refusals
def _refused(case, flags, what):
    rc, out = case.rc(flags)
    assert rc == EUNSUPPORTED, (what, rc)
    assert all(GL.holds(out[k], GL.F) for k in out), (what, "a refused launch wrote an output")


def test_refusals_write_nothing():
    """With the flag, MPCQP_EUNSUPPORTED and no output written: (33, 10), (10, 65), m = 0, float32 at (24, 48), an order, a warm
    state, and every other kernel-choice or factor flag next to it. The same (24, 48) call without any of them runs."""
    from qpmpc_amd import _capi

    rng = np.random.default_rng(11)
    for n, m in ((33, 10), (10, 65)):
        _refused(QPs(*GL._dense_qps(rng, 3, n, m)), _flag(), (n, m))
    P, q, G, h = GL._dense_qps(rng, 3, 24, 48)
    _refused(QPs(P, q, None, None), _flag(), "m = 0")
    P, q, G, h = QC.qps(24, 48)
    _refused(QPs(P, q, G, h, dtype=GL.F32), _flag(), "float32")
    _refused(QPs(P, q, G, h, order=np.arange(len(q))), _flag(), "order")
    _refused(QPs(P, q, G, h, warm=True), _flag(), "warm_state")
    c = _case(24, 48)
    for name in ("OPT_FORCE_LDS", "OPT_FORCE_CONDENSED", "OPT_FORCE_GWS", "OPT_FORCE_DENSE_G", "OPT_ONE_PER_WAVE", "OPT_TWO_PER_WAVE",
                 "OPT_FOUR_PER_WAVE", "OPT_SEED_VIOLATED", "OPT_KEEP_FACTOR", "OPT_REUSE_FACTOR", "OPT_PIPELINE_FACTOR"):
        _refused(c, _flag() | getattr(_capi, name), name)
    rc, out = c.rc(_flag())
    assert rc == 0 and np.array_equal(out["status"], VC.MIXED_STATUS)


# ---------------------------------------------------------------------------------------------- 5. cross-route
@pytest.mark.parametrize("size", QC.CROSS_ROUTE, ids=str)
def test_flagged_and_default_route_agree(size):
    n, m = size
    from qpmpc_amd import solve_qp_batch

    f = _flagged(n, m)
    P, q, G, h = (torch.from_numpy(np.array(a)).cuda() for a in QC.qps(n, m))
    x, lam, st, it = solve_qp_batch(P, q, G, h, return_multipliers=True)
    torch.cuda.synchronize()
    x, st = x.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, f["status"]), (st, f["status"])
    ok = st == 0
    err = _rel(f["U"][ok], x[ok])
    print(f"    {size}: flagged against the default route {err:.2e}")
    assert err <= QC.TOL
    # ... and the Python layer's flagged call is the arena's launch
    xf, lamf, stf, itf = solve_qp_batch(P, q, G, h, return_multipliers=True, flags=_flag())
    torch.cuda.synchronize()
    assert GL.same_bits(xf.cpu().numpy(), f["U"]) and np.array_equal(stf.cpu().numpy(), f["status"])
    assert np.array_equal(itf.cpu().numpy(), f["iters"])


# ---------------------------------------------------------------------------------------------- 6. through the MPC layer
@pytest.mark.parametrize("shape", QC.MPC_SHAPES, ids=str)
def test_through_the_mpc_layer(shape):
    """Problems outside the fused flag's envelope, condensed by BatchMPCQP and solved with the flag: within 1e-7 of the oracle and
    of solve_mpc_batch's default route; solve_mpc_batch with the flag still refuses them."""
    from qpmpc_amd import BatchMPCQP, solve_mpc_batch
    from qpmpc_amd import workloads as W
    from qpmpc_amd.exceptions import BackendError

    bp = W.to_batch_problem(QC.mpc_family(shape))
    x, lam, st, it = BatchMPCQP(bp).solve(flags=_flag())
    plan = solve_mpc_batch(bp)
    torch.cuda.synchronize()
    Uo, _, sto, _ = QC.mpc_reference(shape)
    x, st = x.cpu().numpy(), st.cpu().numpy()
    assert (sto == 0).all() and (st == 0).all(), st
    assert (plan.status.cpu().numpy() == 0).all()
    err, errd = _rel(x, Uo), _rel(x, plan.U.cpu().numpy().reshape(x.shape))
    print(f"    {shape}: against the oracle {err:.2e}, against the default route {errd:.2e}, iters {it.cpu().numpy().tolist()}")
    assert err <= QC.TOL and errd <= QC.TOL
    with pytest.raises(BackendError):
        solve_mpc_batch(bp, flags=_flag())


# ---------------------------------------------------------------------------------------------- 7. streams
def test_side_stream_capture_and_replay():
    """The flagged launch at (24, 48) on a side stream, then captured once on it -- one stream, one call, one kernel: a linear graph
    of a single kernel node -- and replayed twice, on the loaded inputs and on q negated in place: each replay has the bits of
    the eager launch on the same inputs. A replay that launched nothing would leave the 0xFF fill."""
    n, m = 24, 48
    P, q, G, h = QC.qps(n, m)
    c = QPs(P, q, G, h, inout=("q",))
    s = torch.cuda.Stream()
    handle = C.c_void_p(s.cuda_stream)
    ref = _flagged(n, m)
    side = c.run(GL.F, _flag(), stream=handle)
    for k in OUTS:
        assert GL.same_bits(side[k], ref[k]), ("side stream", k)
    flipped = QPs(P, -q, G, h).run(GL.F, _flag())
    assert not GL.same_bits(flipped["U"], ref["U"])
    g, rcs = torch.cuda.CUDAGraph(), []
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        rcs.append(int(c.c_call(_flag(), stream=handle)))
    assert rcs == [0], f"the call returned {rcs} while the stream was capturing"

    def replay():
        g.replay()
        return 0

    def negate_and_replay():
        c.L.arena.view("q").neg_()
        g.replay()
        return 0

    first = c.shaped(c.L.run(GL.F, replay))
    second = c.shaped(c.L.run(GL.F, negate_and_replay))
    for k in OUTS:
        assert GL.same_bits(first[k], ref[k]), ("first replay", k)
        assert GL.same_bits(second[k], flipped[k]), ("second replay, q negated in place", k)
