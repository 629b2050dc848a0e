"""GPU tests of mpcqp_model_periods_batch and ModelClosedLoop: the closed loop of a shared model, many periods per launch.

The reference is the oracle loop of tests/model_loop_np.py (the C oracle per period) on the seeded cases of
tests/model_loop_cases.py. Every launch goes through the C export itself with every buffer carved at exactly its contract
size in a guarded arena (tests/arena.py), outputs pre-filled with 0xFF: a store that did not happen leaves NaN / -1.

1 parity            X, U0, final states, the last status, loop_stats[:, 0] against the oracle loop, cold and warm; bound
                    PARITY_RTOL (measured: profiles/model_loop.md, tools/measure_model_loop_parity.py); and the status of EVERY
                    period, cold and warm, from launches of 1 .. 7 periods
2 period boundary   warm = 0: one launch of 7 periods is BITWISE seven launches of one period with advanced pointers
3 last plan         U, lam, status against the oracle's plan at the state before the last period (1e-8 max(1, |U|), the
                    multipliers 1e-8 max(1, |lam|))
4 warm start        24-period triple case: fewer iterations warm than cold; loop_stats[:, 2] <= warm periods (recorded)
5 optional pointers X, U0, loop_stats, lam, iters NULL in turn: the rest is unchanged
6 memory contract   guards intact, read-only buffers unchanged, no output element left unwritten
7 stream contract   on a side stream; captured in a HIP graph and replayed with the states restored
8 driver            step(3) twice == step(6); fused=False within the bound; BackendError outside the envelope"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import model_loop_cases as MC
import model_loop_np as ML
from arena import Arena, capacity_for

from tools.measure_model_loop_parity import loop_of_case as _loop, shared_model

pytestmark = pytest.mark.gpu

F64, I32, I64 = torch.float64, torch.int32, torch.int64


@functools.lru_cache(maxsize=None)
def case_and_ref(name, batch, periods):
    c = MC.make(name, batch, periods)
    return c, ML.oracle_loop(c, periods)


class Run:
    """One case in a guarded arena: operands, states and outputs at exactly their contract sizes; `call` is the C export."""

    OUT = ("U", "lam", "status", "iters", "X", "U0")

    def __init__(self, case, periods):
        from qpmpc_amd import _capi

        self.capi, self.lib = _capi, _capi.load()
        c = self.c = case
        self.P = periods
        nx, nu, N, mk = c["nx"], c["nu"], c["N"], c["mk"]
        B = self.B = c["x0"].shape[0]
        self.n, self.m = N * nu, N * mk
        self.sm = shared_model(c)
        torch.cuda.synchronize()
        ro = dict(model=self.sm.model.cpu().numpy(), Ap=c["Ap"], Bp=c["Bp"], dist=c["dist"], goal=c["goal"])
        if c["targets"] is not None:
            ro["targets"] = c["targets"]
        sizes = dict(states=(F64, B * nx), U=(F64, B * self.n), lam=(F64, B * self.m), status=(I32, B), iters=(I32, B),
                     X=(F64, B * (periods + 1) * nx), U0=(F64, B * periods * nu), stats=(I64, B * 3),
                     X1=(F64, B * 2 * nx), U01=(F64, B * nu))  # (X1, U01: the records of a launch of ONE period)
        nbytes = [a.nbytes for a in ro.values()] + [torch.empty((), dtype=d).element_size() * k for d, k in sizes.values()]
        ar = self.ar = Arena(capacity_for(nbytes), device="cuda")
        self.ro = tuple(ro)
        for name, a in ro.items():
            a = np.ascontiguousarray(a)
            view, _ = ar.carve(name, a.nbytes, torch.uint8 if a.dtype == np.uint8 else F64)
            view.copy_(torch.from_numpy(a.reshape(-1)).to("cuda"))
        for name, (dt, k) in sizes.items():
            ar.carve(name, torch.empty((), dtype=dt).element_size() * k, dt)
        ar.snapshot(self.ro)
        self.opts = _capi.SolveOpts()
        self.opts.feas_tol = c["tol"]
        self.reset()

    def reset(self):
        self.ar.view("states").copy_(torch.from_numpy(self.c["x0"].reshape(-1)).to("cuda"))
        self.ar.fill(self.OUT, 0xFF)
        self.ar.view("stats").zero_()

    def operands(self, t0):
        c, ar, cp = self.c, self.ar, self.capi
        nx, nu, N = c["nx"], c["nu"], c["N"]
        P = c["periods"]
        plant = cp.LoopPlant(cp.Operand(ar.ptr("Ap"), nx * nx if c["Ap"].ndim == 3 else 0, 0),
                             cp.Operand(ar.ptr("Bp"), nx * nu if c["Bp"].ndim == 3 else 0, 0),
                             cp.Operand(ar.ptr("dist") + 8 * t0 * nx, P * nx, nx))
        if c["goal_by_period"]:
            goal = cp.Operand(ar.ptr("goal") + 8 * t0 * nx, 0, nx)
        else:
            goal = cp.Operand(ar.ptr("goal"), nx, 0)
        if c["targets"] is None:
            tg = cp.Operand(None, 0, 0)
        elif c["targets"].ndim == 2:
            tg = cp.Operand(ar.ptr("targets"), 0, 0)
        else:
            tg = cp.Operand(ar.ptr("targets") + 8 * t0 * N * nx, P * N * nx, N * nx)
        return plant, goal, tg

    def call(self, nperiods, t0=0, warm=0, null=(), stream=None, single=False):
        """The export for periods t0 .. t0 + nperiods - 1 (single: one period, recorded into X1 / U01). -> return code."""
        ar = self.ar
        plant, goal, tg = self.operands(t0)
        ptr = lambda name: None if name in null else ar.ptr(name)  # noqa: E731
        out = self.capi.LoopOut(ptr("X1" if single else "X"), ptr("U01" if single else "U0"), ptr("stats"))
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        return self.lib.mpcqp_model_periods_batch(
            C.byref(self.sm.dims), ar.ptr("model"), C.byref(plant), ar.ptr("states"), C.byref(goal), C.byref(tg), self.B,
            nperiods, warm, C.byref(self.opts), ar.ptr("U"), ptr("lam"), ar.ptr("status"), ptr("iters"), C.byref(out),
            C.c_void_p(sp))

    def get(self):
        torch.cuda.synchronize()
        c, ar, B, P = self.c, self.ar, self.B, self.P
        v = lambda name: ar.view(name).cpu().numpy().copy()  # noqa: E731
        return dict(states=v("states").reshape(B, c["nx"]), U=v("U").reshape(B, self.n), lam=v("lam").reshape(B, self.m),
                    status=v("status"), iters=v("iters"), X=v("X").reshape(B, P + 1, c["nx"]),
                    U0=v("U0").reshape(B, P, c["nu"]), stats=v("stats").reshape(B, 3))

    def healthy(self):
        assert self.ar.guards_intact() == []
        assert self.ar.unchanged() == []


def close(got, ref, rtol, what):
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{what}: max relative error {err.max():.3e} (bound {rtol:.1e})")
    assert err.max() <= rtol, f"{what}: {err.max():.3e} > {rtol:.1e}"


def same(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


CASES = [(n, b, p) for n in MC.NAMES + ("triple_infeasible",) for b in MC.BATCHES for p in MC.PERIODS
         if not (n == "triple_infeasible" and (b, p) != (67, 7))]


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("warm", (0, 1))
@pytest.mark.parametrize("name,batch,periods", CASES)
def test_parity_with_the_oracle_loop(name, batch, periods, warm):
    c, ref = case_and_ref(name, batch, periods)
    r = Run(c, periods)
    assert r.call(periods, warm=warm) == 0
    o = r.get()
    r.healthy()
    close(o["X"], ref["X"], MC.PARITY_RTOL, "X")
    close(o["U0"], ref["U0"], MC.PARITY_RTOL, "U0")
    close(o["states"], ref["X"][:, -1], MC.PARITY_RTOL, "states")
    assert np.array_equal(o["states"], o["X"][:, -1])
    assert np.array_equal(o["stats"][:, 0], ref["failed"]), "periods without a plan"
    assert np.array_equal(o["status"], ref["status"][-1])
    if name == "triple_infeasible":
        assert o["stats"][:, 0].sum() == 7 * 14 and np.array_equal(o["stats"][:, 0] > 0, c["infeasible"])
        assert (o["U0"][c["infeasible"]] == 0).all()
    if not warm:
        assert (o["stats"][:, 2] == 0).all()


@pytest.mark.parametrize("warm", (0, 1))
@pytest.mark.parametrize("name", MC.NAMES + ("triple_infeasible",))
def test_the_status_of_every_period(name, warm):
    """A launch reports the LAST period's status and the loop's total of failed periods, in which a period wrongly accepted and one
    wrongly failed would cancel. A launch of k periods ends on period k - 1 of the longer launch (the same arithmetic from the same
    state, warm start included), so launches of k = 1 .. 7 periods give every period's status and the failures up to it."""
    c, ref = case_and_ref(name, 67, 7)
    r = Run(c, 7)
    for k in range(1, 8):
        r.reset()
        assert r.call(k, warm=warm) == 0
        torch.cuda.synchronize()
        status = r.ar.view("status").cpu().numpy()
        stats = r.ar.view("stats").cpu().numpy().reshape(67, 3)
        assert np.array_equal(status, ref["status"][k - 1]), f"period {k - 1}"
        assert np.array_equal(stats[:, 0], (ref["status"][:k] != 0).sum(0)), f"failed periods up to {k - 1}"
        for v in range(3):  # per-period counts of each verdict
            assert (status == v).sum() == (ref["status"][k - 1] == v).sum()
    r.healthy()


# ------------------------------------------------------------------------------------------------ 2. period boundary
@pytest.mark.parametrize("name", MC.NAMES + ("triple_infeasible",))
def test_one_launch_of_seven_periods_is_seven_launches_of_one(name):
    c, _ = case_and_ref(name, 67, 7)
    r = Run(c, 7)
    assert r.call(7) == 0
    whole = r.get()
    r.reset()
    X, U0 = [], []
    for t in range(7):
        r.ar.fill(("X1", "U01"), 0xFF)
        assert r.call(1, t0=t, single=True) == 0
        torch.cuda.synchronize()
        x1 = r.ar.view("X1").cpu().numpy().reshape(67, 2, c["nx"])
        X.append(x1 if t == 0 else x1[:, 1:])
        U0.append(r.ar.view("U01").cpu().numpy().reshape(67, 1, c["nu"]).copy())
        if t:
            assert x1[:, 0].tobytes() == X[-2][:, -1].tobytes(), "a launch's first record is the state it found"
    parts = r.get()
    parts["X"], parts["U0"] = np.concatenate(X, 1), np.concatenate(U0, 1)
    r.healthy()
    same(whole, parts, name)


# ------------------------------------------------------------------------------------------------ 3. last plan
@pytest.mark.parametrize("warm", (0, 1))
@pytest.mark.parametrize("name", MC.NAMES)
def test_the_last_periods_plan(name, warm):
    c, ref = case_and_ref(name, 67, 7)
    r = Run(c, 7)
    assert r.call(7, warm=warm) == 0
    o = r.get()
    assert np.array_equal(o["status"], ref["status"][-1]) and (o["status"] == 0).all()
    Uo, lo = ref["U"][-1], ref["lam"][-1]
    bound = 1e-8 * np.maximum(1.0, np.abs(Uo).max(axis=1, keepdims=True))
    err = np.abs(o["U"] - Uo)
    print(f"last plan: max |U - U_oracle| / max(1, |U|) = {(err / bound * 1e-8).max():.3e}")
    assert (err <= bound).all()
    # the multipliers under the same bound, 1e-8 relative to max(1, the loop's largest multiplier) -- the way the project holds
    # multipliers elsewhere (tests/test_gpu_pairing.py) --, the same rows active, none negative
    lscale = np.maximum(1.0, np.abs(lo).max(axis=1, keepdims=True))
    lerr = np.abs(o["lam"] - lo)
    print(f"last plan: max |lam - lam_oracle| / max(1, |lam|) = {(lerr / lscale).max():.3e}; absolute {lerr.max():.3e}")
    assert (lerr <= 1e-8 * lscale).all()
    assert (lerr <= bound).all()  # ... and under the plan's own bound, 1e-8 max(1, |U|), as stated
    assert np.array_equal(o["lam"] > 0, lo > 0) and (o["lam"] >= 0).all()


# ------------------------------------------------------------------------------------------------ 4. warm start
def test_warm_start_earns_its_name():
    P = MC.WARM_PERIODS
    c, ref = case_and_ref("triple", 67, P)
    r = Run(c, P)
    assert r.call(P) == 0
    cold = r.get()
    r.reset()
    assert r.call(P, warm=1) == 0
    warm = r.get()
    r.healthy()
    it_cold, it_warm, recold = cold["stats"][:, 1].sum(), warm["stats"][:, 1].sum(), warm["stats"][:, 2]
    print(f"iterations over {P} periods of 67 loops: cold {it_cold}, warm {it_warm}; warm periods re-solved cold {recold.sum()}")
    assert it_warm < it_cold
    assert (recold <= P - 1).all()
    assert (warm["stats"][:, 0] == 0).all() and (cold["stats"][:, 0] == 0).all()
    close(warm["X"], ref["X"], MC.PARITY_RTOL, "warm X")
    close(cold["X"], ref["X"], MC.PARITY_RTOL, "cold X")


# ------------------------------------------------------------------------------------------------ 5. optional pointers
@pytest.mark.parametrize("warm", (0, 1))
@pytest.mark.parametrize("null", ("X", "U0", "stats", "lam", "iters"))
def test_optional_pointers(null, warm):
    c, _ = case_and_ref("box4", 67, 7)
    r = Run(c, 7)
    assert r.call(7, warm=warm) == 0
    full = r.get()
    r.reset()
    assert r.call(7, warm=warm, null=(null,)) == 0
    part = r.get()
    r.healthy()
    same(full, part, f"{null} = NULL", skip=(null,))
    untouched = part[null].view(np.uint8) if null != "stats" else None
    assert (part["stats"] == 0).all() if null == "stats" else (untouched == 0xFF).all()


# ------------------------------------------------------------------------------------------------ 6. memory contract
@pytest.mark.parametrize("warm", (0, 1))
@pytest.mark.parametrize("name", MC.NAMES)
def test_memory_contract(name, warm):
    c, ref = case_and_ref(name, 67, 7)
    r = Run(c, 7)
    assert r.call(7, warm=warm) == 0
    o = r.get()
    r.healthy()
    for k in ("U", "lam", "X", "U0", "states"):
        assert np.isfinite(o[k]).all(), f"{k} has elements the launch did not write"
    assert (o["status"] >= 0).all() and (o["iters"] >= 0).all()
    assert (o["stats"][:, 1] >= o["iters"]).all()  # (the last period's iterations are part of the loop's)


# ------------------------------------------------------------------------------------------------ 7. stream contract
@pytest.mark.parametrize("warm", (0, 1))
def test_side_stream_and_graph_replay(warm):
    c, _ = case_and_ref("triple", 67, 7)
    r = Run(c, 7)
    assert r.call(7, warm=warm) == 0
    plain = r.get()
    r.reset()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc = r.call(7, warm=warm, stream=s)
    assert rc == 0
    s.synchronize()
    same(plain, r.get(), "side stream")
    r.reset()
    torch.cuda.synchronize()
    g, rcs = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(g, stream=s):
        rcs.append(int(r.call(7, warm=warm, stream=s)))
    assert rcs == [0], f"the call returned {rcs} while the stream was capturing"
    r.reset()  # the states restored, the outputs refilled: a replay that launched nothing would leave the fill
    torch.cuda.synchronize()
    g.replay()
    same(plain, r.get(), "graph replay")
    r.healthy()


# ------------------------------------------------------------------------------------------------ 8. driver
@pytest.mark.parametrize("name", ("triple", "box4"))
def test_driver_steps(name):
    c, ref = case_and_ref(name, 67, 7)
    a, b, h = _loop(c), _loop(c), _loop(c)
    a.step(3)
    a.step(3)
    b.step(6)
    for _ in range(6):
        h.step(1, fused=False)
    torch.cuda.synchronize()
    for k in ("X", "U0", "states", "U", "status", "iters", "_loopstats"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.periods == 6 and tuple(a.X.shape) == (67, 7, c["nx"]) and tuple(a.U0.shape) == (67, 6, c["nu"])
    close(b.X.cpu().numpy(), ref["X"][:, :7], MC.PARITY_RTOL, "fused X")
    close(h.X.cpu().numpy(), ref["X"][:, :7], MC.PARITY_RTOL, "by hand X")
    close(h.U0.cpu().numpy(), b.U0.cpu().numpy(), MC.PARITY_RTOL, "fused against by hand U0")
    assert b.stats()["failed"] == 0 and h.stats()["failed"] == 0 and int(b.failed.item()) == 0
    with pytest.raises(ValueError):
        b.step(2)  # the references are laid out for seven periods


def test_driver_refuses_outside_the_envelope():
    from qpmpc_amd import BackendError, BatchMPCProblem, ModelClosedLoop, SharedModel
    from qpmpc_amd.workloads import triple_integrator_matrices

    A, B, Cm, e = triple_integrator_matrices(20)  # n = 20 > 16
    sm = SharedModel(BatchMPCProblem(A, B, Cm, None, e, 20, 1.0, None, 1e-6, np.zeros((1, 3)), goal_state=np.zeros((1, 3))))
    loop = ModelClosedLoop(sm, np.zeros((5, 3)), goal=np.array([1.0, 0, 0]))
    with pytest.raises(BackendError, match="N nu <= 16"):
        loop.step(2)
    loop.step(2, fused=False)  # ... and the loop written by hand serves it
    with pytest.raises(ValueError, match="fused launch only"):
        ModelClosedLoop(sm, np.zeros((5, 3)), goal=np.array([1.0, 0, 0]), warm=True).step(1, fused=False)
    torch.cuda.synchronize()
    assert loop.periods == 2 and tuple(loop.X.shape) == (5, 3, 3)
    # bounds per problem: refused as well
    A, B, Cm, e = triple_integrator_matrices(16)
    eb = np.broadcast_to(e, (4, 1, 2)).copy()
    smb = SharedModel(BatchMPCProblem(A, B, Cm, None, eb, 16, 1.0, None, 1e-6, np.zeros((4, 3)), goal_state=np.zeros((4, 3))))
    with pytest.raises(BackendError, match="bounds per problem"):
        ModelClosedLoop(smb, np.zeros((4, 3)), goal=np.zeros(3)).step(1)
