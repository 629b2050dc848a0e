"""GPU tests (-m gpu): the stream contract of include/mpcqp.h -- every export is "asynchronous on the caller's hipStream_t,
re-entrant, no global state". Every kernel of a call goes on the given stream, in order; nothing synchronises with the host; a
call can be captured into a HIP graph after one eager launch of the same dimensions; calls on distinct streams with distinct
outputs and workspaces are independent.

A launch that ran in stream order is told from one that ran ahead of the work queued before it by the DATA it saw. Every route
of tests/stream_cases.py (all of operand_layouts.ROUTES at the padded layout 1, and the two on-chip routes for 17 .. 32
variables) has two sets of initial states: x0_A, which the arena loads, and x0_B, which is copied over it on the stream right in
front of the launch -- behind a delay of about 5 ms on that stream. tests/test_stream_cases_cpu.py shows on the oracle that A's
and B's plans differ, item by item, by at least ten times the bound a plan is held to. A kernel of the call that went to another
stream runs ahead of the copy and returns A's plans; test_a_launch_on_the_wrong_stream_is_seen does exactly that on purpose, once.
(Two streams that share a hardware queue run in order whatever the handles say, so these tests take a side stream that the
default stream is first shown to run ahead of: side_stream().)

The arena machinery is that of tests/guarded_launch.py: Launch.run fills outputs and workspace with 0xFF before the
call and checks guards and read-only operands behind it, so a launch or a graph replay that did nothing leaves NaN plans.
Bounds: 1e-7 relative for float64 plans, 1e-3 for float32 ones against the oracle on the float32-rounded operands (those of
tests/test_gpu_operand_layouts.py); a launch on a side stream, a replay, a launch next to another stream's or another thread's
equals the plain default-stream launch bit for bit (status, iters, U, lam of the solved items).

Every graph is linear: one stream, no event and no second stream inside a capture. A return code is taken out of the capture
before it is asserted on, and a graph whose capture returned non-zero is never replayed."""
import ctypes as C
import threading

import numpy as np
import pytest

import operand_layouts as OL
import stream_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers and comparisons; needs torch)
from guarded_launch import Forward, Launch, ModelCase, equal_outputs  # noqa: E402
from guarded_launch import flags as _flags  # noqa: E402

F, F64, F32, I32, U8 = GL.F, GL.F64, GL.F32, GL.I32, GL.U8
OUTS = ("U", "lam", "status", "iters")
ROUTES = list(SC.ROUTES_UNDER_TEST)
DELAY_MS, MIN_DELAY_MS = 5.0, 1.0


def _handle(stream):
    """the hipStream_t of a torch stream as the C ABI takes it"""
    return C.c_void_p(stream.cuda_stream)


# ---------------------------------------------------------------------------------------------- the delay
_RATE = []


def _cycles(ms):
    """argument of torch.cuda._sleep for about `ms` milliseconds: the counter it spins on is not the shader clock on every
    device, so its rate is measured once, on a spin of 10^6 counts between two events"""
    if not _RATE:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)  # (the first call loads the kernel)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(1_000_000)
        b.record()
        torch.cuda.synchronize()
        _RATE.append(1_000_000 / max(a.elapsed_time(b), 1e-3))
        print(f"    torch.cuda._sleep: {_RATE[0]:.0f} counts per millisecond")
    return int(ms * _RATE[0])


class Delay:
    """About DELAY_MS of spinning on the current stream between two events; conclusive() after a synchronise asserts that it
    lasted MIN_DELAY_MS or more (a case whose delay did not last fails as inconclusive, it does not pass)."""

    def __init__(self, ms=DELAY_MS):
        self.cycles = _cycles(ms)
        self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def enqueue(self):
        self.a.record()
        torch.cuda._sleep(self.cycles)
        self.b.record()

    def conclusive(self):
        ms = self.a.elapsed_time(self.b)
        assert ms >= MIN_DELAY_MS, f"inconclusive: the delay in front of the copy lasted {ms:.3f} ms, not {MIN_DELAY_MS} ms or more"


def side_stream(of=None):
    """A fresh torch.cuda.Stream() that work on the stream `of` (None: the default stream) does NOT queue up behind. The runtime
    maps streams onto a few hardware queues, and two streams that share one run in order of submission whatever their handles
    say: a kernel that strayed to the default stream would then still wait for the side stream's delay and copy, and pass; two
    streams "in flight" would run one after the other. So the stream is shown to let `of` run ahead before it is used: a delay
    on it, a small kernel and an event on `of`, and when that event is done the delay must still be running. torch hands out
    its pooled streams in turn; eight are tried."""
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    of = torch.cuda.default_stream() if of is None else of
    probe = torch.zeros((64,), device="cuda")
    for _ in range(8):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        behind, ahead = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(s):
            torch.cuda._sleep(_cycles(DELAY_MS))
            behind.record()
        with torch.cuda.stream(of):
            probe.add_(1.0)
            ahead.record()
        ahead.synchronize()
        independent = not behind.query()
        torch.cuda.synchronize()
        if independent and s != of:
            return s
        print(f"    stream {s.cuda_stream:#x}: stream {of.cuda_stream:#x} waits for it (a shared hardware queue); trying the next")
    pytest.fail("inconclusive: no side stream that the other stream does not wait for")


def two_streams():
    """two fresh streams of which the second is shown not to queue up behind the first (side_stream): work on them can overlap"""
    first = torch.cuda.Stream()
    return [first, side_stream(of=first)]


# ---------------------------------------------------------------------------------------------- a route in the arena
class Case:
    """One route of stream_cases.ROUTES_UNDER_TEST with everything in a guarded arena (GL.Forward, or the ModelCase of
    tests/test_gpu_onchip32_model.py for the shared-model route), x0 as an "inout" buffer -- loaded with x0_A (`which` "B":
    x0_B) before every run, free to be rewritten inside call() --, and the route's raw C call on a stream handle."""

    def __init__(self, name, which="A"):
        from qpmpc_amd import _capi

        r = self.r = SC.ROUTES_UNDER_TEST[name]
        self.name, self.model = name, SC.is_model(name)
        w = (SC.case_a(name) if which == "A" else SC.case_b(name))[0]
        self.dtype = F32 if r["f32"] else F64
        if self.model:
            self.case, x0 = ModelCase(w, OL.model_pads(r["variant"]), inout=("x0",)), "x0"
        else:
            self.case, x0 = Forward(w, dtype=self.dtype, stagewise=r["stagewise"], pad=OL.pads_of(SC.LAYOUT), inout=("x0",)), "op_x0"
        L = self.L = self.case.L
        assert self.case.B == OL.BATCH
        spec = next(s for s in L.specs if s["name"] == x0)
        assert spec["role"] == "inout" and spec["stride"] > spec["rows"].shape[1]  # (a padded batch stride)
        self.x0 = L.arena.view(x0).as_strided(tuple(spec["rows"].shape), (spec["stride"], 1))
        self.x0_B = torch.as_tensor(SC.x0_b(name)).to("cuda", self.dtype)
        self.opts = _capi.SolveOpts()
        self.opts.flags = _flags(r.get("flags", ()))
        torch.cuda.synchronize()

    def c_call(self, sp):
        """the route's C call with `sp` as its stream argument; the return code"""
        _, lib, _ = GL._api()
        L, c = self.L, self.case
        if self.model:
            o = c.ops
            return lib.mpcqp_solve_model_bounds_batch(C.byref(c.mdims), L.ptr("model"), C.byref(o["e"]), C.byref(o["x0"]), C.byref(o["goal"]),
                                                      C.byref(o["targets"]), c.B, C.byref(self.opts), L.ptr("U"), L.ptr("lam"),
                                                      L.ptr("status"), L.ptr("iters"), sp)
        tail = (L.ptr("U"), L.ptr("lam"), L.ptr("status"), L.ptr("iters"), L.ptr("ws"), c.ws_bytes, sp)
        if c.stagewise:
            return lib.mpcqp_stagewise_solve_batch(C.byref(c.dims), C.byref(c.cp), c.B, C.byref(self.opts), c.max_active, *tail)
        return lib.mpcqp_build_solve_batch(C.byref(c.dims), C.byref(c.cp), c.B, C.byref(self.opts), *tail)

    def shaped(self, out):
        out["U"], out["lam"] = out["U"].reshape(self.case.B, self.case.n), out["lam"].reshape(self.case.B, self.case.m)
        return out

    def run(self, call):
        """Launch.run under the 0xFF fill: guards, read-only operands and return code 0 asserted; the outputs"""
        return self.shaped(self.L.run(F, call))

    def copy_B(self):
        """x0_B over x0, in place, on the current stream"""
        self.x0.copy_(self.x0_B)

    def stash(self):
        """copies of the outputs as they are at this point of the current stream, then the outputs back to the 0xFF fill"""
        held = {k: self.L.arena.view(k).clone() for k in OUTS}
        self.L.arena.fill(OUTS, F)
        return held

    def stashed(self, held):
        return self.shaped({k: v.cpu().numpy() for k, v in held.items()})


_CASES, _EAGER = {}, {}


def case_of(name, which="A"):
    if (name, which) not in _CASES:
        _CASES[(name, which)] = Case(name, which)
    return _CASES[(name, which)]


def against_oracle(name, which, out):
    """statuses the oracle's (all solved) and the plan within the route's bound of the oracle's on the materialised problems"""
    Uo, sto = SC.plan_reference(name, which)  # (the dense HBM routes: the oracle's plans as recorded, held to it by the CPU test)
    assert (sto == 0).all() and np.array_equal(out["status"], sto), (name, which, out["status"], sto)
    U = out["U"].astype(np.float64)
    err = float((np.abs(U - Uo) / np.maximum(1.0, np.abs(Uo).max(axis=1, keepdims=True))).max())
    print(f"    {name}, x0_{which}: max rel err vs oracle {err:.2e}")
    assert err <= SC.bound(name), (name, which, err)


def eager(name, which):
    """the plain launch of a route on the default stream, one at a time, on x0_A or (copied in on that stream) x0_B; run once and
    held to the oracle"""
    if (name, which) not in _EAGER:
        c = case_of(name)
        default = _handle(torch.cuda.default_stream())

        def call():
            if which == "B":
                c.copy_B()
            return c.c_call(default)

        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        out = c.run(call)
        against_oracle(name, which, out)
        _EAGER[(name, which)] = out
    return _EAGER[(name, which)]


def delayed_copy_then(c, s, then):
    """call() for Launch.run: on the side stream `s`, with no synchronise in between, a delay, the copy of x0_B over x0, and
    `then()` (which returns the call's return code); and the delay, to be asked whether it lasted"""
    delay = Delay()

    def call():
        with torch.cuda.stream(s):
            delay.enqueue()
            c.copy_B()
        return then()

    return call, delay


# ---------------------------------------------------------------------------------------------- 1. ordering on a side stream
@pytest.mark.parametrize("route", ROUTES)
def test_every_kernel_of_a_call_is_ordered_on_the_side_stream(route):
    """A delay, the copy of x0_B over x0 and the route's C call, all on one side stream: return code 0, guards and read-only
    operands intact, statuses and plan the oracle's for B, and every output bit the plain default-stream launch's on B."""
    c, s = case_of(route), side_stream()
    plain_A, plain_B = eager(route, "A"), eager(route, "B")
    sep = SC.separation(plain_A["U"].astype(np.float64), plain_B["U"].astype(np.float64))
    assert (sep >= SC.SEPARATION * SC.bound(route)).all(), sep  # (A's plans cannot pass for B's)
    call, delay = delayed_copy_then(c, s, lambda: c.c_call(_handle(s)))
    out = c.run(call)
    delay.conclusive()
    against_oracle(route, "B", out)
    equal_outputs(out, plain_B, route + ": side stream against the default stream")


def test_a_launch_on_the_wrong_stream_is_seen():
    """The positive control, once: the same set-up with the C call handed the DEFAULT stream's handle. It does not wait for the
    side stream's delay and copy, reads x0_A (a stale read of a valid buffer) and returns A's plans, which the check above
    tells from B's."""
    route = "quad lean"
    c, s = case_of(route), side_stream()
    plain_A, plain_B = eager(route, "A"), eager(route, "B")
    call, delay = delayed_copy_then(c, s, lambda: c.c_call(_handle(torch.cuda.default_stream())))
    out = c.run(call)
    delay.conclusive()
    equal_outputs(out, plain_A, "a launch that ran ahead of the copy returns A's plans")
    assert not any(GL.same_bits(out["U"][i], plain_B["U"][i]) for i in range(OL.BATCH))
    with pytest.raises(AssertionError):
        against_oracle(route, "B", out)


# ---------------------------------------------------------------------------------------------- 2. the prepared launches
def _wait_then_launch(run, x0, x0_B, s):
    """the delayed copy of x0_B over the problem's x0 on `s`, then run.launch(stream=s) with the default stream current"""
    delay = Delay()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay.enqueue()
        x0.copy_(x0_B)
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    run.launch(stream=s)
    torch.cuda.synchronize()
    delay.conclusive()
    return dict(U=run.U.cpu().numpy(), status=run.status.cpu().numpy())


@pytest.mark.parametrize("route", ["quad lean", "narrow stage-wise", "promoted f32 (3, 1, 16, 2)"])
def test_prepared_solve_launch_takes_the_stream(route):
    """PreparedSolve.launch(stream=s) while torch's current stream stays the default one: four per wavefront, narrow stage-wise
    and float32 promoted (conversion, solve, conversion) through solve-level flags; the plans are B's."""
    from qpmpc_amd import PreparedSolve
    from qpmpc_amd import workloads as W

    r = SC.ROUTES_UNDER_TEST[route]
    bp = W.to_batch_problem(SC.case_a(route)[0], dtype=F32 if r["f32"] else None)
    run = PreparedSolve(bp, flags=_flags(r["flags"]))
    x0_B = torch.as_tensor(SC.x0_b(route)).to("cuda", bp.dtype)
    out = _wait_then_launch(run, bp.initial_state, x0_B, side_stream())
    against_oracle(route, "B", out)


def test_prepared_model_solve_launch_takes_the_stream():
    """The same for a PreparedModelSolve from SharedModel.prepare (bounds per problem at 17 variables: the on-chip kernel)."""
    from qpmpc_amd import SharedModel
    from qpmpc_amd import workloads as W

    bp = W.to_batch_problem(SC.case_a(SC.ON_CHIP_MODEL)[0])
    run = SharedModel(bp).prepare(bp)
    x0_B = torch.as_tensor(SC.x0_b(SC.ON_CHIP_MODEL)).to("cuda", bp.dtype)
    out = _wait_then_launch(run, bp.initial_state, x0_B, side_stream())
    against_oracle(SC.ON_CHIP_MODEL, "B", out)


# ---------------------------------------------------------------------------------------------- 3. capture and replay
def capture(calls, s):
    """One linear graph of `calls` (each returns a C return code) captured on `s`; (graph, return codes). Nothing is asserted, and
    nothing raises, while the stream is capturing."""
    g, rcs = torch.cuda.CUDAGraph(), []
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        for call in calls:
            rcs.append(int(call()))
    return g, rcs


@pytest.mark.parametrize("route", ROUTES)
def test_capture_and_replay(route):
    """After one eager launch, the route's C call captured on a side stream: the replay behind a copy of x0_B gives B's plans --
    the oracle's within the bound, the eager launch's bit for bit --, and a replay without the copy (Launch.run reloads x0_A)
    gives the eager A result bit for bit. A replay that launched nothing would leave the 0xFF fill."""
    c, s = case_of(route), torch.cuda.Stream()
    plain_A, plain_B = eager(route, "A"), eager(route, "B")
    g, rcs = capture([lambda: c.c_call(_handle(s))], s)
    assert rcs == [0], f"the call returned {rcs} while the stream was capturing"

    def copy_and_replay():
        c.copy_B()
        g.replay()
        return 0

    def replay():
        g.replay()
        return 0

    out = c.run(copy_and_replay)
    against_oracle(route, "B", out)
    equal_outputs(out, plain_B, route + ": replay on x0_B against the eager launch")
    again = c.run(replay)
    equal_outputs(again, plain_A, route + ": replay on x0_A against the eager launch")


# ---------------------------------------------------------------------------------------------- 4. captured sequences
class Pair:
    """The two launches of a stateful sequence of stream_cases.SEQUENCES in one arena: the operands, the workspace and the warm
    state once, the outputs once per launch."""

    def __init__(self, seq):
        from qpmpc_amd import _capi
        from qpmpc_amd import workloads as W

        _, lib, _ = GL._api()
        self.w = OL.ltv(*seq["ltv"])
        bp = self.bp = W.to_batch_problem(self.w)
        self.B, self.n, self.m, self.dims = bp.batch_size, bp.nb_variables, bp.nb_constraints, bp.dims()
        nbytes = C.c_size_t(0)
        assert lib.mpcqp_workspace_bytes(C.byref(self.dims), self.B, 1, C.byref(nbytes)) == 0
        self.ws_bytes = nbytes.value
        L = self.L = Launch()
        GL.add_problem(L, bp)
        for i in (1, 2):
            L.add(f"U{i}", "out", F64, self.B * self.n)
            L.add(f"lam{i}", "out", F64, self.B * self.m)
            L.add(f"status{i}", "out", I32, self.B)
            L.add(f"iters{i}", "out", I32, self.B)
        L.add("ws", "scratch", U8, self.ws_bytes)
        if seq["warm"]:
            wb = C.c_size_t(0)
            assert lib.mpcqp_warm_state_bytes(C.byref(self.dims), C.byref(wb)) == 0 and wb.value > 0
            L.add("warm", "scratch", U8, self.B * wb.value)
        L.build()
        assert L.has(seq["carried"])  # (what the second launch reads of the first)
        self.cp = GL.arena_problem(L, bp)
        self.opts = []
        for step in (seq["first"], seq["second"]):
            o = _capi.SolveOpts()
            o.flags = _flags(step["flags"])
            if L.has("warm"):
                o.warm_state, o.warm_state_bytes = L.ptr("warm"), L.nbytes("warm")
                o.warm_start = getattr(_capi, step["warm_start"]) if step["warm_start"] else 0
            self.opts.append(o)

    def c_call(self, i, sp):
        _, lib, _ = GL._api()
        L = self.L
        return lib.mpcqp_build_solve_batch(C.byref(self.dims), C.byref(self.cp), self.B, C.byref(self.opts[i - 1]), L.ptr(f"U{i}"),
                                           L.ptr(f"lam{i}"), L.ptr(f"status{i}"), L.ptr(f"iters{i}"), L.ptr("ws"), self.ws_bytes, sp)

    def run(self, call):
        out = self.L.run(F, call)
        return [dict(U=out[f"U{i}"].reshape(self.B, self.n), lam=out[f"lam{i}"].reshape(self.B, self.m), status=out[f"status{i}"],
                     iters=out[f"iters{i}"]) for i in (1, 2)]


@pytest.mark.parametrize("name", list(SC.SEQUENCES))
def test_captured_sequences(name):
    """Each stateful pair -- keep then reuse the factor in the narrow stage-wise kernel's workspace; a cold launch with a warm state
    then a warm launch -- as one graph of two launches: the replayed pair equals the eager pair bit for bit (the second launch
    reads what the first one of the SAME replay left, under the 0xFF fill), and both are right by the oracle."""
    p, s = Pair(SC.SEQUENCES[name]), torch.cuda.Stream()
    default = _handle(torch.cuda.default_stream())

    def eager_pair():
        return p.c_call(1, default) or p.c_call(2, default)

    first = p.run(eager_pair)
    for i, out in enumerate(first):
        GL.against_oracle(f"{name}, launch {i + 1}", p.w, out, 1e-7)
    g, rcs = capture([lambda: p.c_call(1, _handle(s)), lambda: p.c_call(2, _handle(s))], s)
    assert rcs == [0, 0], f"the calls returned {rcs} while the stream was capturing"

    def replay():
        g.replay()
        return 0

    for what in ("first replay", "second replay"):
        for i, (a, b) in enumerate(zip(first, p.run(replay))):
            equal_outputs(a, b, f"{name}, launch {i + 1}, {what}")


# ---------------------------------------------------------------------------------------------- 5. two LDS sizes of one kernel
_LDS = {}


def lds_case(shape):
    """(workload, arena case) of the workgroup kernel at one shape of stream_cases.LDS_SHAPES"""
    if shape not in _LDS:
        w = SC.lds_case(shape)
        _LDS[shape] = (w, Forward(w))
    return _LDS[shape]


def test_one_graph_holds_two_lds_sizes_of_one_instantiation():
    """The workgroup kernel (MPCQP_OPT_FORCE_LDS) at three shapes of one template instantiation whose dynamic LDS all exceed 48 KiB:
    its launcher sets the kernel's MaxDynamicSharedMemorySize to the launch's own size before every launch. The largest and then
    the middle one are captured into one graph; between capture and replay the smallest is launched eagerly (the last value set
    is then below both captured sizes); the replayed plans are the oracle's and their eager twins' bit for bit."""
    from qpmpc_amd import _capi

    shapes = sorted(SC.LDS_SHAPES, key=SC.LDS_SHAPES.get, reverse=True)
    assert len(shapes) == 3
    (wl, large), (wm, mid), (wsm, small) = (lds_case(shape) for shape in shapes)
    flag = _capi.OPT_FORCE_LDS
    twins = [case.run(F, flag) for case in (large, mid)]
    for shape, w, out in zip(shapes, (wl, wm), twins):
        GL.against_oracle(f"workgroup kernel {shape}", w, out, 1e-7)
    s = torch.cuda.Stream()
    opts = _capi.SolveOpts()
    opts.flags = flag
    _, lib, _ = GL._api()

    def c_call(case):
        L = case.L
        return lib.mpcqp_build_solve_batch(C.byref(case.dims), C.byref(case.cp), case.B, C.byref(opts), L.ptr("U"), L.ptr("lam"),
                                           L.ptr("status"), L.ptr("iters"), L.ptr("ws"), case.ws_bytes, _handle(s))

    g, rcs = capture([lambda: c_call(large), lambda: c_call(mid)], s)
    assert rcs == [0, 0], f"the calls returned {rcs} while the stream was capturing"
    GL.against_oracle(f"workgroup kernel {shapes[2]}", wsm, small.run(F, flag), 1e-7)
    got = {}

    def replay():
        g.replay()
        return 0

    def inner():
        got["mid"] = mid.L.run(F, replay)
        return 0

    got["large"] = large.L.run(F, inner)  # (both arenas under the 0xFF fill and checked around the one replay)
    for key, case, twin, shape, w in (("large", large, twins[0], shapes[0], wl), ("mid", mid, twins[1], shapes[1], wm)):
        out = got[key]
        out["U"], out["lam"] = out["U"].reshape(case.B, case.n), out["lam"].reshape(case.B, case.m)
        GL.against_oracle(f"workgroup kernel {shape}", w, out, 1e-7)
        equal_outputs(out, twin, f"workgroup kernel {shape}: replay against the eager launch")


# ---------------------------------------------------------------------------------------------- 6. two streams in flight
LAUNCHES_IN_FLIGHT = 4


def run_two(a, b, call):
    """Launch.run of two arena cases around one call(): both under the 0xFF fill, the guards and read-only operands of both checked"""
    got = {}

    def inner():
        got["b"] = b.L.run(F, call)
        return 0

    got["a"] = a.L.run(F, inner)
    return a.shaped(got["a"]), b.shaped(got["b"])


def gate(streams, head_ms=0.5):
    """Hold `streams` back behind one event of the default stream, itself behind a delay, so that what is enqueued on them next
    is released together; each starts with a short delay of its own."""
    torch.cuda._sleep(_cycles(DELAY_MS))
    released = torch.cuda.Event()
    released.record()
    for s in streams:
        s.wait_event(released)
        with torch.cuda.stream(s):
            torch.cuda._sleep(_cycles(head_ms))


PAIRINGS = [(("quad lean", "A"), ("quad lean", "B")), (("narrow stage-wise", "A"), ("wide stage-wise f32", "A")),
            (("dense HBM f32", "A"), ("pair generic", "A"))]


@pytest.mark.parametrize("left,right", PAIRINGS, ids=[f"{a[0]} {a[1]} | {b[0]} {b[1]}" for a, b in PAIRINGS])
def test_two_streams_in_flight(left, right):
    """Two arena cases, each with its own outputs and workspace, on two streams that are first shown to run side by side
    (two_streams) and are released together: four launches per stream, alternating, no synchronise. After every launch its outputs are copied aside on its stream and put back to the 0xFF fill;
    every launch's outputs equal the serial result bit for bit."""
    cases = [case_of(*left), case_of(*right)]  # (the same route twice: the second arena loads x0_B)
    serial = [eager(*left), eager(*right)]
    streams = two_streams()
    held, rcs = ([], []), []

    def call():
        gate(streams)
        for _ in range(LAUNCHES_IN_FLIGHT):
            for k in (0, 1):
                rcs.append(cases[k].c_call(_handle(streams[k])))
                with torch.cuda.stream(streams[k]):
                    held[k].append(cases[k].stash())
        return 0

    run_two(cases[0], cases[1], call)
    assert rcs == [0] * (2 * LAUNCHES_IN_FLIGHT), rcs
    for k in (0, 1):
        assert len(held[k]) == LAUNCHES_IN_FLIGHT
        for i, h in enumerate(held[k]):
            equal_outputs(cases[k].stashed(h), serial[k], f"{(left, right)[k]}: launch {i + 1} of {LAUNCHES_IN_FLIGHT} next to another stream's")


def test_order_by_count_on_two_streams():
    """mpcqp_order_by_count (three kernels per call) on two streams (shown to run side by side) with two count vectors, released together: each result a
    permutation, longest first, as tests/test_gpu_memory_discipline.py::test_order_by_count asks of it."""
    _, lib, _ = GL._api()
    batch = 1025
    nbytes = int(lib.mpcqp_order_workspace_bytes(batch))
    streams = two_streams()
    counts, Ls = [], []
    for seed in (1, 2):
        counts.append(np.random.default_rng(seed).integers(0, 40, batch).astype(np.int32))
        L = Launch()
        L.add("counts", "in", I32, data=torch.as_tensor(counts[-1]))
        L.add("order", "out", I32, batch)
        L.add("ws", "scratch", U8, nbytes)
        Ls.append(L.build())
    assert not np.array_equal(counts[0], counts[1])
    rcs, got = [], {}

    def call():
        gate(streams)
        for L, s in zip(Ls, streams):
            rcs.append(lib.mpcqp_order_by_count(L.ptr("counts"), batch, L.ptr("order"), L.ptr("ws"), nbytes, _handle(s)))
        return 0

    def inner():
        got[1] = Ls[1].run(F, call)
        return 0

    got[0] = Ls[0].run(F, inner)
    assert rcs == [0, 0], rcs
    for k in (0, 1):
        order = got[k]["order"]
        assert np.array_equal(np.sort(order), np.arange(batch)), "not a permutation"
        assert (np.diff(counts[k][order]) <= 0).all(), "not sorted, longest first"


# ---------------------------------------------------------------------------------------------- 7. two host threads
LAUNCHES_PER_THREAD = 8


def test_two_host_threads():
    """Two threads behind one barrier, each with its own stream (the two shown to run side by side) and its own route (the four-per-wavefront kernel and the wide
    stage-wise kernel: different kernel functions), eight launches each through the raw C call: every return code 0 and every
    launch's outputs the serial result bit for bit."""
    routes = ("quad lean", "wide stage-wise f64")
    cases = [case_of(r) for r in routes]
    serial = [eager(r, "A") for r in routes]
    barrier, streams = threading.Barrier(2), two_streams()
    held, rcs, errors = ([], []), ([], []), []

    def work(k):
        try:
            s = streams[k]
            barrier.wait(timeout=30)
            for _ in range(LAUNCHES_PER_THREAD):
                rcs[k].append(cases[k].c_call(_handle(s)))
                with torch.cuda.stream(s):
                    held[k].append(cases[k].stash())
            s.synchronize()
        except Exception as exn:  # (reported by the main thread)
            errors.append((k, repr(exn)))
            barrier.abort()

    def call():
        threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        return 0

    run_two(cases[0], cases[1], call)
    assert not errors, errors
    for k in (0, 1):
        assert rcs[k] == [0] * LAUNCHES_PER_THREAD, (routes[k], rcs[k])
        for i, h in enumerate(held[k]):
            equal_outputs(cases[k].stashed(h), serial[k], f"{routes[k]}: launch {i + 1} of {LAUNCHES_PER_THREAD} next to another thread's")


# ---------------------------------------------------------------------------------------------- 8. autograd on a side stream
def _bits_equal(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert GL.same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy()), what


def _diff_run(solve, operands, stream):
    """forward and backward of `solve(*leaves)` -> (U, X, plan), everything on `stream` (None: the default stream): U, X, the
    gradients of a fixed linear functional of both, and the plan"""
    leaves = [t.clone().requires_grad_(True) for t in operands]
    torch.cuda.synchronize()

    def go():
        U, X, plan = solve(*leaves)
        g = torch.Generator(device="cpu").manual_seed(7)
        cU = torch.randn(U.shape, generator=g, dtype=torch.float64).to(U.device)
        cX = torch.randn(X.shape, generator=g, dtype=torch.float64).to(U.device)
        ((U * cU).sum() + (X * cX).sum()).backward()
        return U, X, plan

    if stream is None:
        U, X, plan = go()
    else:
        with torch.cuda.stream(stream):
            U, X, plan = go()
    torch.cuda.synchronize()
    return U, X, [t.grad for t in leaves], plan


def _same_diff(a, b, names):
    (Ua, Xa, ga, pa), (Ub, Xb, gb, pb) = a, b
    assert (pa.status == 0).all() and (pa.vjp_status == 0).all() and (pb.vjp_status == 0).all(), (pa.status, pa.vjp_status, pb.vjp_status)
    _bits_equal(Ua, Ub, "U")
    _bits_equal(Xa, Xb, "X")
    assert torch.equal(pa.status, pb.status) and torch.equal(pa.iters, pb.iters)
    for name, x, y in zip(names, ga, gb):
        assert x is not None and float(x.abs().max()) > 0, name
        _bits_equal(x, y, "gradient with respect to " + name)


def test_solve_mpc_batch_diff_on_a_side_stream():
    """solve_mpc_batch_diff (condensed adjoint) at (3, 2, 8, 2), forward and backward inside torch.cuda.stream(s): plans, states
    and the gradients with respect to x0, goal, targets and e bit for bit those of the default-stream run; vjp_status all zero."""
    from qpmpc_amd import solve_mpc_batch_diff
    from qpmpc_amd import workloads as W

    shape = OL.DIFF_SHAPES[0]
    assert shape == (3, 2, 8, 2)
    bp = W.to_batch_problem(OL.diff_case(shape, SC.LAYOUT)[1])
    operands = (bp.initial_state, bp.goal_state, bp.target_states, bp.e)

    def solve(x0, goal, targets, e):
        return solve_mpc_batch_diff(bp, initial_state=x0, goal_state=goal, target_states=targets, ineq_vector=e, states=True)

    _same_diff(_diff_run(solve, operands, None), _diff_run(solve, operands, torch.cuda.Stream()), ("x0", "goal", "targets", "e"))


def test_shared_model_solve_diff_on_a_side_stream():
    """SharedModel.solve_diff with bounds per problem (the shared-model route's problems), forward and backward inside
    torch.cuda.stream(s), against the default-stream run, bit for bit."""
    from qpmpc_amd import SharedModel
    from qpmpc_amd import workloads as W

    bp = W.to_batch_problem(SC.case_a(SC.ON_CHIP_MODEL)[0])
    model = SharedModel(bp)
    operands = (bp.initial_state, bp.goal_state, bp.target_states, bp.e)

    def solve(x0, goal, targets, e):
        return model.solve_diff(x0, goal, targets, ineq_vector=e, states=True)

    _same_diff(_diff_run(solve, operands, None), _diff_run(solve, operands, torch.cuda.Stream()), ("x0", "goal", "targets", "e"))


# ---------------------------------------------------------------------------------------------- 9. a control period as a graph
@pytest.mark.parametrize("horizon,fused", [(24, True), (12, False)], ids=["fused period, one launch", "two launches per period"])
def test_a_control_period_as_a_graph(horizon, fused):
    """WIPClosedLoop(fused_period=True) with no factor kept between periods makes the same call(s) every period. At 24 timesteps
    the narrow stage-wise kernel serves the period and it is ONE launch, mpcqp_wip_periods_batch; at 12 (n <= 16: an on-chip
    kernel, which has no closed-loop epilogue) the loop falls back by itself to TWO launches per period, the solve and
    mpcqp_wip_advance_stats_batch. Either way: two eager steps, the third step(1) captured (a capture runs nothing), three
    replays; states, failed and iters_total equal those of a twin loop stepped five times eagerly."""
    from qpmpc_amd import workloads as W
    from qpmpc_amd.closed_loop import WIPClosedLoop

    x0 = W.wip_batch(OL.BATCH, N=horizon, seed=21)["x0"]
    x0[0], x0[1] = [0.0, 0.3, 0.0, 1.0], [0.0, -0.25, 0.0, -0.8]  # (these two hold the input box active)
    kw = dict(nb_timesteps=horizon, fused_period=True, reuse_factor=False, pipeline_factor=False, periods_per_launch=1)
    loop, twin = WIPClosedLoop(x0, **kw), WIPClosedLoop(x0, **kw)
    twin.step(5)
    loop.step(1)
    loop.step(1)
    torch.cuda.synchronize()
    assert loop._fused == fused and twin._fused == fused  # (which of the two periods is about to be captured)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        loop.step(1)
    still = loop._fused == fused and twin._fused == fused
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert still, "the loop changed its kind of period while it was captured"
    assert float((twin.states - torch.as_tensor(x0, device="cuda")).abs().max()) > 1e-3  # (the plant moved)
    _bits_equal(loop.states, twin.states, "states after five periods")
    assert int(loop.failed.item()) == int(twin.failed.item()) and int(loop.iters_total.item()) == int(twin.iters_total.item())
    assert int(twin.iters_total.item()) > 0
