"""GPU tests of mpcqp_model_periods_vjp_batch and closed_loop_diff: gradients through closed loops of a shared model.

The reference is the NumPy restatement of the reverse-time recursion (tests/loop_adjoint_np.py) fed the ORACLE loop's
multipliers (tests/model_loop_np.py) on the seeded cases of tests/model_loop_cases.py; tests/test_loop_diff_cpu.py holds that
restatement to central differences. Loops whose oracle margin is under 1e-6 (tools/measure_loop_diff_parity.py, MARGIN) get
zero cotangents and so drop out of every sum over the batch; the filter may drop at most 5 % of a case's loops. The bound is
loop_adjoint_np.GRAD_RTOL, measured (profiles/loop_diff.md): ten times the error of the composed path, never looser than 1e-6.

1 parity             every gradient of the fused path, cold and warm, against the restatement; fused against fused=False; the
                     replay error; every period's status
2 period sums        period_stride 0 equals the sum of the per-period blocks (1e-13)
3 batch striding     16,384 + 67 loops: every copy of loops 0 .. 66 agrees with them (1e-12)
4 optional pointers  each output NULL in turn, gX or gU0 NULL
5 memory contract    guarded arena, outputs poisoned, read-only buffers unchanged
6 stream contract    a launch on a side stream
7 autograd           torch.autograd.grad of a scalar loss; without requires_grad the records are bitwise ModelClosedLoop's;
                     BackendError outside the envelope, which fused=False serves"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import loop_adjoint_np as LA
import model_loop_cases as MC
import model_loop_np as ML
from arena import Arena, capacity_for

from tools.measure_loop_diff_parity import NAMES, case_reference, gradients, operands, worst
from tools.measure_model_loop_parity import loop_of_case, shared_model

pytestmark = pytest.mark.gpu

F64, I32 = torch.float64, torch.int32
ALL = MC.NAMES + ("triple_infeasible",)


@functools.lru_cache(maxsize=None)
def reference(name, B, P):
    return case_reference(name, B, P)


@functools.lru_cache(maxsize=None)
def model_of(name):
    return shared_model(MC.make(name, 67, 7))


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("warm", (False, True))
@pytest.mark.parametrize("periods", (1, 7))
@pytest.mark.parametrize("batch", (1, 5, 67))
@pytest.mark.parametrize("name", ALL)
def test_gradients_against_the_restatement(name, batch, periods, warm):
    c, ref, keep, gX, gU0, want = reference(name, batch, periods)
    assert (~keep).sum() <= 0.05 * batch, f"the margin filter drops {(~keep).sum()} of {batch} loops"
    sm = model_of(name)
    got, info, X, U0 = gradients(sm, c, operands(c), periods, gX, gU0, warm=warm)
    assert X.grad_fn is not None and U0.grad_fn is not None
    err = worst(got, want)
    print(f"{name} B={batch} P={periods} warm={warm}: fused against the restatement {err}")
    assert set(err) == {k for k in NAMES if want[k] is not None}
    assert max(err.values()) <= LA.GRAD_RTOL, err
    replay = float(info.replay_error.item())
    print(f"replay error {replay:.2e} (bound {2 * MC.PARITY_RTOL:.1e})")
    assert replay <= 2 * MC.PARITY_RTOL
    assert np.array_equal(info.status.cpu().numpy(), ref["status"].T), "every period's status"
    assert int(info.failed.item()) == int(ref["failed"].sum())
    assert (info.vjp_status.cpu().numpy() == 0).all()
    if not warm:
        hand, hinfo, _, _ = gradients(sm, c, operands(c), periods, gX, gU0, fused=False)
        err = worst(got, hand)
        print(f"fused against fused=False {err}")
        assert max(err.values()) <= LA.GRAD_RTOL, err
        assert np.array_equal(hinfo.status.cpu().numpy(), ref["status"].T)
    if name == "triple_infeasible" and batch == 67:  # the designated loops: the pure plant adjoint
        for b in np.flatnonzero(c["infeasible"]):
            a = LA.plant_adjoint(c, gX, b)
            assert np.abs(got["x0"][b] - a[0]).max() <= 1e-13 * max(1.0, np.abs(a).max())
            assert np.abs(got["disturbance"][b] - a[1:]).max() <= 1e-13 * max(1.0, np.abs(a).max())


# ------------------------------------------------------------------------------------------------ the export in an arena
class Run:
    """The export on a case, fed the ORACLE loop's multipliers, statuses and records: every operand and output at exactly its
    contract size between guards."""

    OUT = ("g_x0", "g_states", "g_goal", "g_targets", "g_goal_sum", "g_targets_sum", "g_A", "g_B", "vjp_status")

    def __init__(self, name, B=67, P=7, tile=1):
        from qpmpc_amd import _capi

        self.capi, self.lib = _capi, _capi.load()
        c, ref, keep, gX, gU0, _ = reference(name, B, P)
        self.c, self.ref, self.P = c, ref, P
        nx, nu, N = c["nx"], c["nu"], c["N"]
        self.B = B = B * tile
        self.m, self.nT = N * c["mk"], N * nx
        self.sm = model_of(name)
        torch.cuda.synchronize()
        rep = lambda a: np.concatenate([a] * tile, 0) if tile > 1 else a  # noqa: E731
        ro = dict(model=self.sm.model.cpu().numpy(), Ap=rep(c["Ap"]) if c["Ap"].ndim == 3 else c["Ap"],
                  Bp=rep(c["Bp"]) if c["Bp"].ndim == 3 else c["Bp"], lam=rep(ref["lam"].transpose(1, 0, 2)),
                  status=rep(ref["status"].T.astype(np.int32)), X=rep(ref["X"]), U0=rep(ref["U0"]), gX=rep(gX), gU0=rep(gU0))
        self.gX, self.gU0 = gX, gU0
        sizes = dict(g_x0=(F64, B * nx), g_states=(F64, B * (P + 1) * nx), g_goal=(F64, B * P * nx),
                     g_targets=(F64, B * P * self.nT), g_goal_sum=(F64, B * nx), g_targets_sum=(F64, B * self.nT),
                     g_A=(F64, B * nx * nx), g_B=(F64, B * nx * nu), vjp_status=(I32, B))
        ro = {k: np.ascontiguousarray(v) for k, v in ro.items()}
        nbytes = [a.nbytes for a in ro.values()] + [torch.empty((), dtype=d).element_size() * k for d, k in sizes.values()]
        ar = self.ar = Arena(capacity_for(nbytes), device="cuda")
        self.ro = tuple(ro)
        for k, a in ro.items():
            dt = torch.uint8 if a.dtype == np.uint8 else (I32 if a.dtype == np.int32 else F64)
            view, _ = ar.carve(k, a.nbytes, dt)
            view.copy_(torch.from_numpy(a.reshape(-1)).to("cuda"))
        for k, (dt, n) in sizes.items():
            ar.carve(k, torch.empty((), dtype=dt).element_size() * n, dt)
        ar.snapshot(self.ro)
        ar.fill(self.OUT, 0xFF)

    def call(self, null=(), summed=False, stream=None):
        c, ar, cp, P = self.c, self.ar, self.capi, self.P
        nx, nu = c["nx"], c["nu"]
        ptr = lambda k: None if k in null else ar.ptr(k)  # noqa: E731
        plant = cp.LoopPlant(cp.Operand(ar.ptr("Ap"), nx * nx if c["Ap"].ndim == 3 else 0, 0),
                             cp.Operand(ar.ptr("Bp"), nx * nu if c["Bp"].ndim == 3 else 0, 0), cp.Operand(None, 0, 0))
        if summed:
            gg, gt = cp.PeriodGrad(ptr("g_goal_sum"), nx, 0), cp.PeriodGrad(ptr("g_targets_sum"), self.nT, 0)
        else:
            gg, gt = cp.PeriodGrad(ptr("g_goal"), P * nx, nx), cp.PeriodGrad(ptr("g_targets"), P * self.nT, self.nT)
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        return self.lib.mpcqp_model_periods_vjp_batch(
            C.byref(self.sm.dims), ar.ptr("model"), C.byref(plant), self.B, P, ar.ptr("lam"), ar.ptr("status"), ptr("X"),
            ptr("U0"), ptr("gX"), ptr("gU0"), ar.ptr("g_x0"), ptr("g_states"), C.byref(gg), C.byref(gt), ptr("g_A"),
            ptr("g_B"), ptr("vjp_status"), C.c_void_p(sp))

    def get(self):
        torch.cuda.synchronize()
        B, P, nx, nu = self.B, self.P, self.c["nx"], self.c["nu"]
        shapes = dict(g_x0=(B, nx), g_states=(B, P + 1, nx), g_goal=(B, P, nx), g_targets=(B, P, self.nT), g_goal_sum=(B, nx),
                      g_targets_sum=(B, self.nT), g_A=(B, nx, nx), g_B=(B, nx, nu), vjp_status=(B,))
        return {k: self.ar.view(k).cpu().numpy().copy().reshape(s) for k, s in shapes.items()}

    def healthy(self):
        assert self.ar.guards_intact() == []
        assert self.ar.unchanged() == []


def rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def per_loop_reference(r):
    return LA.loop_vjp(r.c, r.ref, r.gX, r.gU0)


@pytest.mark.parametrize("name", ALL)
def test_the_kernel_on_the_oracles_multipliers_and_its_memory_contract(name):
    """The same multipliers on both sides: what is left is the kernel's rounding against NumPy's. Guards intact, read-only
    buffers unchanged, every output written (the 0xFF fill is NaN / -1)."""
    r = Run(name)
    assert r.call() == 0
    o = r.get()
    r.healthy()
    g = per_loop_reference(r)
    pairs = dict(g_x0=g["x0"], g_states=g["states"], g_goal=g["goal"], g_targets=g["targets"])
    for k, want in pairs.items():
        assert np.isfinite(o[k]).all(), f"{k} has elements the launch did not write"
        e = rel(o[k], want)
        print(f"{name} {k}: {e:.2e}")
        assert e <= LA.GRAD_RTOL, (k, e)
    # g_A = sum_t a_{t+1} x_t' and g_B = sum_t a_{t+1} u0_t' per loop: a costate held to GRAD_RTOL max(1, |a|) moves an entry by
    # at most GRAD_RTOL sum_t max(1, |a_{t+1, i}|) |x_{t, j}| -- the bound on the costates carried through the outer products
    # (the jerk of the triple family reaches 86, so an entry of g_B is not held to the costate's own absolute error)
    big = np.maximum(1.0, np.abs(g["states"][:, 1:]))
    for k, want, rec in (("g_A", g["Ap"], r.ref["X"][:, :-1]), ("g_B", g["Bp"], r.ref["U0"])):
        assert np.isfinite(o[k]).all(), f"{k} has elements the launch did not write"
        scale = np.maximum(np.maximum(1.0, np.abs(want)), np.einsum("bti,btj->bij", big, np.abs(rec)))
        e = float((np.abs(o[k] - want) / scale).max())
        print(f"{name} {k}: {e:.2e} of its bound's scale; {rel(o[k], want):.2e} of max(1, |entry|)")
        assert e <= LA.GRAD_RTOL, (k, e)
    assert np.array_equal(o["vjp_status"], g["failed"]) and (o["vjp_status"] == 0).all()
    assert (r.ar.raw("g_goal_sum") == 0xFF).all() and (r.ar.raw("g_targets_sum") == 0xFF).all()  # not passed: not written


# ------------------------------------------------------------------------------------------------ 2. period sums
@pytest.mark.parametrize("name", ("box4", "triple"))
def test_period_sums_equal_the_sum_of_the_per_period_blocks(name):
    r = Run(name)
    assert r.call() == 0 and r.call(summed=True) == 0
    o = r.get()
    r.healthy()
    for k in ("g_goal", "g_targets"):
        want = o[k].sum(1)
        err = np.abs(o[k + "_sum"] - want).max() / max(1.0, np.abs(want).max())
        print(f"{name} {k}: {err:.2e}")
        assert err <= 1e-13
    assert np.abs(o["g_goal"]).max() > 0


# ------------------------------------------------------------------------------------------------ 3. batch striding
def test_workgroups_stride_over_a_batch_beyond_the_grid():
    """16 x kModelDiffMaxGrid = 16,384 loops fill the grid once: 16,384 + 67 loops take a second round on the first workgroups.
    The 67 `tiny` loops tiled 246 times (16,482 loops, 2 periods): every copy agrees with loops 0 .. 66."""
    tile = 246
    assert 67 * tile >= 16 * 1024 + 67
    r = Run("tiny", 67, 2, tile=tile)
    assert r.call() == 0
    o = r.get()
    r.healthy()
    for k in ("g_x0", "g_states", "g_goal", "g_targets", "g_A", "g_B"):
        v = o[k].reshape((tile, 67) + o[k].shape[1:])
        assert np.isfinite(v).all()
        err = np.abs(v - v[:1]).max() / max(1.0, np.abs(v[0]).max())
        assert err <= 1e-12, (k, err)
    assert rel(o["g_x0"][:67], per_loop_reference(Run("tiny", 67, 2))["x0"]) <= LA.GRAD_RTOL
    assert (o["vjp_status"] == 0).all()


# ------------------------------------------------------------------------------------------------ 4. optional pointers
@pytest.mark.parametrize("null", ("g_states", "g_goal", "g_targets", "g_A", "g_B", "vjp_status", "gX", "gU0", "X+g_A", "U0+g_B"))
def test_optional_pointers(null):
    r = Run("box4")
    assert r.call() == 0
    full = r.get()
    r.ar.fill(r.OUT, 0xFF)
    nulls = tuple(null.split("+"))
    assert r.call(null=nulls) == 0
    part = r.get()
    r.healthy()
    if null in ("gX", "gU0"):  # a NULL cotangent is zero: the restatement with zeros in its place
        g = LA.loop_vjp(r.c, r.ref, np.zeros_like(r.gX) if null == "gX" else r.gX,
                        np.zeros_like(r.gU0) if null == "gU0" else r.gU0)
        for k, want in dict(g_x0=g["x0"], g_states=g["states"], g_goal=g["goal"], g_targets=g["targets"], g_A=g["Ap"],
                            g_B=g["Bp"]).items():
            assert rel(part[k], want) <= LA.GRAD_RTOL, k
        assert np.abs(part["g_x0"] - full["g_x0"]).max() > 0
        return
    for k in full:
        if k in nulls:
            assert (r.ar.raw(k) == 0xFF).all(), f"{k} = NULL was written"
        elif not k.endswith("_sum"):
            assert full[k].tobytes() == part[k].tobytes(), f"{null} = NULL changed {k}"


# ------------------------------------------------------------------------------------------------ 6. stream contract
def test_a_launch_on_a_side_stream():
    r = Run("triple")
    assert r.call() == 0
    plain = r.get()
    r.ar.fill(r.OUT, 0xFF)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc = r.call(stream=s)
    assert rc == 0
    s.synchronize()
    side = r.get()
    r.healthy()
    for k in plain:
        assert plain[k].tobytes() == side[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 7. autograd
def test_autograd_grad_of_a_scalar_loss():
    from qpmpc_amd import closed_loop_diff

    c = MC.make("triple", 67, 7)
    sm = model_of("triple")
    x0 = torch.tensor(c["x0"], device="cuda", requires_grad=True)
    goal = torch.tensor(c["goal"][0], device="cuda", requires_grad=True)  # one goal, shared by the batch and the periods
    X, U0, info = closed_loop_diff(sm, x0, 7, goal=goal, disturbance=c["dist"], feas_tol=c["tol"])
    assert info.vjp_status is None and info.status.shape == (67, 7)
    loss = ((X[:, -1] - goal) ** 2).sum() + 1e-4 * (U0 ** 2).sum()
    gx, gg = torch.autograd.grad(loss, (x0, goal))
    assert gx.shape == x0.shape and gg.shape == goal.shape and gx.dtype == F64
    assert torch.isfinite(gx).all() and torch.isfinite(gg).all() and gx.abs().sum() > 0 and gg.abs().sum() > 0
    assert info.vjp_status.shape == (67,) and int(info.vjp_status.sum().item()) == 0
    # the same loss through the composed path
    x1, g1 = x0.detach().clone().requires_grad_(), goal.detach().clone().requires_grad_()
    Xh, Uh, _ = closed_loop_diff(sm, x1, 7, goal=g1, disturbance=c["dist"], feas_tol=c["tol"], fused=False)
    hx, hg = torch.autograd.grad(((Xh[:, -1] - g1) ** 2).sum() + 1e-4 * (Uh ** 2).sum(), (x1, g1))
    for a, b in ((gx, hx), (gg, hg)):
        assert rel(a.cpu().numpy(), b.cpu().numpy()) <= LA.GRAD_RTOL


@pytest.mark.parametrize("warm", (False, True))
def test_without_requires_grad_the_records_are_the_loops(warm):
    from qpmpc_amd import closed_loop_diff

    c = MC.make("box4", 67, 7)
    ops = operands(c, grad=False)
    X, U0, info = closed_loop_diff(model_of("box4"), ops["x0"], 7, goal=ops["goal"], targets=ops["targets"],
                                   plant=(ops["Ap"], ops["Bp"]), disturbance=ops["disturbance"], feas_tol=c["tol"], warm=warm)
    loop = loop_of_case(c, warm=warm)
    loop.step(7)
    torch.cuda.synchronize()
    assert X.grad_fn is None and U0.grad_fn is None and info.replay_error is None
    assert torch.equal(X, loop.X) and torch.equal(U0, loop.U0)
    with torch.no_grad():  # ... and under no_grad, whatever requires grad
        ops = operands(c)
        X2, U2, _ = closed_loop_diff(model_of("box4"), ops["x0"], 7, goal=ops["goal"], targets=ops["targets"],
                                     plant=(ops["Ap"], ops["Bp"]), disturbance=ops["disturbance"], feas_tol=c["tol"], warm=warm)
    assert torch.equal(X2, loop.X) and torch.equal(U2, loop.U0)


def test_outside_the_envelope():
    from qpmpc_amd import BackendError, BatchMPCProblem, SharedModel, closed_loop_diff
    from qpmpc_amd.workloads import triple_integrator_matrices

    A, B, Cm, e = triple_integrator_matrices(20)  # n = 20 > 16
    sm = SharedModel(BatchMPCProblem(A, B, Cm, None, e, 20, 1.0, None, 1e-6, np.zeros((1, 3)), goal_state=np.zeros((1, 3))))
    x0 = torch.zeros((5, 3), dtype=F64, device="cuda", requires_grad=True)
    goal = torch.tensor([1.0, 0.0, 0.0], dtype=F64, device="cuda")
    with pytest.raises(BackendError, match="fused=False"):
        closed_loop_diff(sm, x0, 2, goal=goal)
    X, U0, info = closed_loop_diff(sm, x0, 2, goal=goal, fused=False)  # ... and the composed loop serves it
    (g,) = torch.autograd.grad(X[:, -1].sum(), (x0,))
    assert tuple(X.shape) == (5, 3, 3) and tuple(U0.shape) == (5, 2, 1) and torch.isfinite(g).all()
    assert info.status.shape == (5, 2)
