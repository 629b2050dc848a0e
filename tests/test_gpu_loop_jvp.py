"""GPU tests of mpcqp_model_periods_jvp_batch, closed_loop_jvp and closed_loop_jacobian: forward sensitivities of closed loops
of a shared model.

The reference is the NumPy restatement of the forward-time recursion (tests/loop_tangent_np.py) fed the ORACLE loop's
multipliers (tests/model_loop_np.py) on the seeded cases of tests/model_loop_cases.py; tests/test_loop_jvp_cpu.py holds that
restatement to its transpose and to central differences. Through the public path the loops whose oracle margin is under 1e-6
(tools/measure_loop_diff_parity.py, MARGIN) are left out of the comparison -- the loops do not interact --; the filter may
drop at most 5 % of a case's loops. The bound is loop_tangent_np.TANGENT_RTOL, measured (profiles/loop_jvp.md): ten times the
error of the composed path, never looser than 1e-6.

1 the kernel         on the oracle's multipliers in a guarded arena (tests/guarded_launch.py): T = 1, nx and 17 (a second,
                     ragged pass), tangents on all six operands, every output element written, jvp_status
2 the public path    closed_loop_jvp(fused=True), cold and warm, against the restatement and against fused=False; the replay error
3 sharing, strides   a tangent set shared by the batch, a reference tangent constant in time (1e-13)
4 duality            mpcqp_model_periods_vjp_batch and the new export on the same multipliers
5 batch striding     16,384 + 67 loops: every copy of loops 0 .. 66 agrees with them (1e-12)
6 other paths        nullable outputs, each tangent NULL in turn, a side stream, closed_loop_jacobian against plan_jacobian, a
                     forward_ad dual through closed_loop_diff, BackendError outside the envelope"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402
import loop_adjoint_np as LA  # noqa: E402
import loop_tangent_np as LT  # noqa: E402
import model_loop_cases as MC  # noqa: E402

from tools.measure_loop_diff_parity import operands  # noqa: E402
from tools.measure_loop_jvp_parity import case_reference, sensitivities, worst  # noqa: E402
from tools.measure_model_loop_parity import shared_model  # noqa: E402

pytestmark = pytest.mark.gpu

F64, I32 = torch.float64, torch.int32
ALL = MC.NAMES + ("triple_infeasible",)
TANGENT_KEYS = ("x0", "goal", "targets", "dist", "Ap", "Bp")


@functools.lru_cache(maxsize=None)
def reference(name, B, P, T):
    return case_reference(name, B, P, T)


@functools.lru_cache(maxsize=None)
def model_of(name):
    return shared_model(MC.make(name, 67, 7))


def rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


# ------------------------------------------------------------------------------------------------ the export in an arena
class Run:
    """The export on a case, fed the ORACLE loop's multipliers, statuses and records, with the tangents `tan`
    ({operand: [B|1, T, ...] or None}; a reference's tangent [.., T, w] is constant in time): every operand and output at
    exactly its contract size between guards."""

    def __init__(self, name, T, B=67, P=7, tile=1, tan=None):
        from qpmpc_amd import _capi

        self.capi, self.lib = _capi, _capi.load()
        c, ref, _, full, want = reference(name, B, P, T)
        self.c, self.ref, self.P, self.T, self.want = c, ref, P, T, want
        self.tan = tan = dict(full if tan is None else tan)
        self.B = B = B * tile
        self.sm = model_of(name)
        torch.cuda.synchronize()
        rep = lambda a: np.concatenate([a] * tile, 0) if tile > 1 and a.shape[0] > 1 else a  # noqa: E731
        L = self.L = GL.Launch()
        L.add("model", "in", self.sm.model.dtype, data=self.sm.model.reshape(1, -1))
        ro = dict(Ap=rep(c["Ap"]) if c["Ap"].ndim == 3 else c["Ap"][None], Bp=rep(c["Bp"]) if c["Bp"].ndim == 3 else c["Bp"][None],
                  lam=rep(ref["lam"].transpose(1, 0, 2)), X=rep(ref["X"]), U0=rep(ref["U0"]))
        for k, a in ro.items():
            L.add(k, "in", F64, data=np.ascontiguousarray(a).reshape(a.shape[0], -1))
        L.add("status", "in", I32, data=torch.as_tensor(np.ascontiguousarray(rep(ref["status"].T.astype(np.int32)))))
        for k in TANGENT_KEYS:
            if tan.get(k) is not None:
                a = rep(tan[k])
                L.add("d_" + k, "in", F64, data=np.ascontiguousarray(a).reshape(a.shape[0], -1))
        L.add("dX", "out", F64, B * T * (P + 1) * c["nx"])
        L.add("dU0", "out", F64, B * T * P * c["nu"])
        L.add("jvp_status", "out", I32, B)
        L.build()

    def _tangents(self, null=()):
        cp, L, tan = self.capi, self.L, self.tan
        shared = lambda a: a.shape[0] == 1 and self.B > 1  # noqa: E731

        def flat(k):
            a = tan.get(k)
            if a is None or k in null:
                return (None, 0)
            return (L.ptr("d_" + k), 0 if shared(a) else a[0].size)

        def periodic(k):
            a = tan.get(k)
            if a is None or k in null:
                return cp.PeriodTangent(None, 0, 0, 0)
            return cp.PeriodTangent(L.ptr("d_" + k), 0 if shared(a) else a[0].size, a[0, 0].size, a.shape[-1] if a.ndim == 4 else 0)

        return cp.LoopTangents(*flat("x0"), periodic("goal"), periodic("targets"), periodic("dist"), *flat("Ap"), *flat("Bp"))

    def call(self, null=(), stream=None):
        """the export's call for Launch.run; `null`: outputs or tangents passed as NULL"""
        c, L, cp = self.c, self.L, self.capi
        nx, nu = c["nx"], c["nu"]
        plant = cp.LoopPlant(cp.Operand(L.ptr("Ap"), nx * nx if c["Ap"].ndim == 3 else 0, 0),
                             cp.Operand(L.ptr("Bp"), nx * nu if c["Bp"].ndim == 3 else 0, 0), cp.Operand(None, 0, 0))
        tn = self._tangents(null)
        ptr = lambda k: None if k in null else L.ptr(k)  # noqa: E731

        def go():
            sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
            return self.lib.mpcqp_model_periods_jvp_batch(
                C.byref(self.sm.dims), L.ptr("model"), C.byref(plant), self.B, self.P, self.T, L.ptr("lam"), L.ptr("status"),
                L.ptr("X") if tn.dA else None, L.ptr("U0") if tn.dB else None, C.byref(tn), L.ptr("dX"), ptr("dU0"),
                ptr("jvp_status"), C.c_void_p(sp))

        return go

    def run(self, **kw):
        """One launch under the 0xFF fill: return code 0, guards intact, read-only buffers unchanged (Launch.run asserts
        them) -> dX [B, T, P+1, nx], dU0 [B, T, P, nu], jvp_status [B]."""
        o = self.L.run(GL.F, self.call(**kw))
        B, T, P, c = self.B, self.T, self.P, self.c
        return dict(dX=o["dX"].reshape(B, T, P + 1, c["nx"]), dU0=o["dU0"].reshape(B, T, P, c["nu"]), jvp_status=o["jvp_status"])


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("T", ("1", "nx", "17"))
@pytest.mark.parametrize("name", ALL)
def test_the_kernel_on_the_oracles_multipliers_and_its_memory_contract(name, T):
    """The same multipliers on both sides: what is left is the kernel's rounding against NumPy's. Guards intact, read-only
    buffers unchanged, every output written (the 0xFF fill is NaN / -1)."""
    T = MC.SHAPES["triple" if name == "triple_infeasible" else name][0] if T == "nx" else int(T)
    r = Run(name, T)
    o = r.run()
    for k in ("dX", "dU0"):
        assert np.isfinite(o[k]).all(), f"{k} has elements the launch did not write"
        e = rel(o[k], r.want[k])
        print(f"{name} T={T} {k}: {e:.2e}")
        assert e <= LT.TANGENT_RTOL, (k, e)
    assert np.array_equal(o["jvp_status"], r.want["failed"]) and (o["jvp_status"] == 0).all()
    assert np.abs(o["dU0"]).max() > 0
    if name == "triple_infeasible":  # the designated loops: the tangent rolls through the plant only
        for b in np.flatnonzero(r.c["infeasible"]):
            assert not o["dU0"][b].any()
            want = np.stack([LT.plant_rollout(r.c, r.tan, b, j, r.ref["X"], r.ref["U0"]) for j in range(T)])
            assert np.abs(o["dX"][b] - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------ 2. the public path
@pytest.mark.parametrize("warm", (False, True))
@pytest.mark.parametrize("periods", (1, 7))
@pytest.mark.parametrize("batch", (1, 5, 67))
@pytest.mark.parametrize("name", ALL)
def test_closed_loop_jvp_against_the_restatement(name, batch, periods, warm):
    T = MC.SHAPES["triple" if name == "triple_infeasible" else name][0]
    c, ref, keep, tan, want = reference(name, batch, periods, T)
    assert (~keep).sum() <= 0.05 * batch, f"the margin filter drops {(~keep).sum()} of {batch} loops"
    sm = model_of(name)
    dX, dU0, info = sensitivities(sm, c, periods, tan, warm=warm)
    assert dX.shape == (batch, T, periods + 1, c["nx"]) and dU0.shape == (batch, T, periods, c["nu"])
    err = worst((dX, dU0), want, keep)
    print(f"{name} B={batch} P={periods} warm={warm}: fused against the restatement {err}")
    assert max(err.values()) <= LT.TANGENT_RTOL, err
    replay = float(info.replay_error.item())
    print(f"replay error {replay:.2e} (bound {2 * MC.PARITY_RTOL:.1e})")
    assert replay <= 2 * MC.PARITY_RTOL
    assert np.array_equal(info.status.cpu().numpy(), ref["status"].T), "every period's status"
    assert int(info.failed.item()) == int(ref["failed"].sum())
    assert (info.jvp_status.cpu().numpy() == 0).all()
    if not warm:
        hX, hU0, hinfo = sensitivities(sm, c, periods, tan, fused=False)
        err = worst((dX, dU0), dict(dX=hX, dU0=hU0), keep)
        print(f"fused against fused=False {err}")
        assert max(err.values()) <= LT.TANGENT_RTOL, err
        assert np.array_equal(hinfo.status.cpu().numpy(), ref["status"].T)
        assert (hinfo.jvp_status.cpu().numpy() == 0).all()


# ------------------------------------------------------------------------------------------------ 3. sharing and strides
@pytest.mark.parametrize("name", ("box4", "triple"))
def test_a_tangent_set_shared_by_the_batch_equals_the_same_set_tiled(name):
    T, P = 3, 7
    c = reference(name, 67, P, T)[0]
    one = LT.tangents(c, P, T, shared=True)
    if c["targets"] is None:
        one["targets"] = None
    tiled = {k: (None if v is None else np.repeat(v, 67, axis=0)) for k, v in one.items()}
    a, b = Run(name, T, tan=one).run(), Run(name, T, tan=tiled).run()
    for k in ("dX", "dU0"):
        err = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max())
        print(f"{name} {k}: {err:.2e}")
        assert np.isfinite(a[k]).all() and err <= 1e-13
    assert np.abs(a["dU0"]).max() > 0


@pytest.mark.parametrize("name", ("box4", "triple"))
def test_a_reference_tangent_constant_in_time_equals_the_same_tangent_repeated(name):
    T, P = 3, 7
    c, _, _, full, _ = reference(name, 67, P, T)
    const = dict(full)
    for k in ("goal", "targets", "dist"):
        if full[k] is not None:
            const[k] = np.ascontiguousarray(full[k][:, :, 0])
    repeated = {k: (np.repeat(v[:, :, None], P, axis=2) if k in ("goal", "targets", "dist") and v is not None else v)
                for k, v in const.items()}
    a, b = Run(name, T, tan=const).run(), Run(name, T, tan=repeated).run()
    for k in ("dX", "dU0"):
        err = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max())
        print(f"{name} {k}: {err:.2e}")
        assert np.isfinite(a[k]).all() and err <= 1e-13
    want = LT.loop_jvp(c, reference(name, 67, P, T)[1], const)
    assert rel(a["dX"], want["dX"]) <= LT.TANGENT_RTOL and rel(a["dU0"], want["dU0"]) <= LT.TANGENT_RTOL


# ------------------------------------------------------------------------------------------------ 4. duality on the device
@pytest.mark.parametrize("name", ALL)
def test_the_export_is_the_transpose_of_the_adjoint_export(name):
    """<gX, dX> + <gU0, dU0> = <g, tangents> per loop and tangent, the gradients by mpcqp_model_periods_vjp_batch on the same
    multipliers, relative to the sum of the absolute values of the paired terms."""
    T, P, B = 3, 7, 67
    r = Run(name, T)
    o = r.run()
    c, ref, cp = r.c, r.ref, r.capi
    nx, nu, nT, m = c["nx"], c["nu"], c["N"] * c["nx"], c["N"] * c["mk"]
    gX, gU0 = LA.cotangents(c, P, ref)
    dev = lambda a, dt=F64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")  # noqa: E731
    t = dict(Ap=dev(c["Ap"]), Bp=dev(c["Bp"]), lam=dev(ref["lam"].transpose(1, 0, 2)), status=dev(ref["status"].T, I32),
             X=dev(ref["X"]), U0=dev(ref["U0"]), gX=dev(gX), gU0=dev(gU0))
    g = dict(x0=torch.empty((B, nx), dtype=F64, device="cuda"), states=torch.empty((B, P + 1, nx), dtype=F64, device="cuda"),
             goal=torch.empty((B, P, nx), dtype=F64, device="cuda"), targets=torch.empty((B, P, nT), dtype=F64, device="cuda"),
             Ap=torch.empty((B, nx, nx), dtype=F64, device="cuda"), Bp=torch.empty((B, nx, nu), dtype=F64, device="cuda"))
    vst = torch.empty((B,), dtype=I32, device="cuda")
    plant = cp.LoopPlant(cp.Operand(t["Ap"].data_ptr(), nx * nx if c["Ap"].ndim == 3 else 0, 0),
                         cp.Operand(t["Bp"].data_ptr(), nx * nu if c["Bp"].ndim == 3 else 0, 0), cp.Operand(None, 0, 0))
    gg, gt = cp.PeriodGrad(g["goal"].data_ptr(), P * nx, nx), cp.PeriodGrad(g["targets"].data_ptr(), P * nT, nT)
    rc = r.lib.mpcqp_model_periods_vjp_batch(
        C.byref(r.sm.dims), r.sm.model.data_ptr(), C.byref(plant), B, P, t["lam"].data_ptr(), t["status"].data_ptr(),
        t["X"].data_ptr(), t["U0"].data_ptr(), t["gX"].data_ptr(), t["gU0"].data_ptr(), g["x0"].data_ptr(), g["states"].data_ptr(),
        C.byref(gg), C.byref(gt), g["Ap"].data_ptr(), g["Bp"].data_ptr(), vst.data_ptr(),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    gn = {k: v.cpu().numpy() for k, v in g.items()}
    assert np.array_equal(vst.cpu().numpy(), o["jvp_status"]), "jvp_status equals vjp_status on the same inputs"
    lhs = (gX[:, None] * o["dX"]).sum(axis=(2, 3)) + (gU0[:, None] * o["dU0"]).sum(axis=(2, 3))
    lmag = np.abs(gX[:, None] * o["dX"]).sum(axis=(2, 3)) + np.abs(gU0[:, None] * o["dU0"]).sum(axis=(2, 3))
    rhs, rmag = LT.pairing(gn, r.tan)
    err = float((np.abs(lhs - rhs) / (lmag + rmag)).max())
    print(f"{name}: duality on the device {err:.2e} (bound {LA.GRAD_RTOL + LT.TANGENT_RTOL:.1e})")
    assert err <= LA.GRAD_RTOL + LT.TANGENT_RTOL


# ------------------------------------------------------------------------------------------------ 5. batch striding
def test_workgroups_stride_over_a_batch_beyond_the_grid():
    """16 x kModelDiffMaxGrid = 16,384 loops fill the grid once: 16,384 + 67 loops take a second round on the first workgroups.
    The 67 `tiny` loops tiled 246 times (16,482 loops, 2 periods, T = 1): every copy agrees with loops 0 .. 66."""
    tile = 246
    assert 67 * tile >= 16 * 1024 + 67
    r = Run("tiny", 1, 67, 2, tile=tile)
    o = r.run()
    for k in ("dX", "dU0"):
        v = o[k].reshape((tile, 67) + o[k].shape[1:])
        assert np.isfinite(v).all()
        err = np.abs(v - v[:1]).max() / max(1.0, np.abs(v[0]).max())
        assert err <= 1e-12, (k, err)
        assert rel(v[0], r.want[k]) <= LT.TANGENT_RTOL
    assert (o["jvp_status"] == 0).all()


# ------------------------------------------------------------------------------------------------ 6. other paths
@pytest.mark.parametrize("null", ("dU0", "jvp_status"))
def test_nullable_outputs(null):
    r = Run("box4", 3)
    full, part = r.run(), r.run(null=(null,))
    assert GL.holds(part[null], GL.F), f"{null} = NULL was written"
    for k in full:
        if k != null:
            assert full[k].tobytes() == part[k].tobytes(), f"{null} = NULL changed {k}"


@pytest.mark.parametrize("null", TANGENT_KEYS)
def test_each_tangent_null_in_turn(null):
    """A NULL tangent is zero: the restatement without it."""
    r = Run("box4", 3)
    full, part = r.run(), r.run(null=(null,))
    want = LT.loop_jvp(r.c, r.ref, {k: (None if k == null else v) for k, v in r.tan.items()})
    for k in ("dX", "dU0"):
        assert np.isfinite(part[k]).all()
        assert rel(part[k], want[k]) <= LT.TANGENT_RTOL, k
    assert np.abs(part["dX"] - full["dX"]).max() > 0


def test_a_launch_on_a_side_stream():
    r = Run("triple", 3)
    plain = r.run()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = r.run(stream=s)
    for k in plain:
        assert plain[k].tobytes() == side[k].tobytes(), k


def test_closed_loop_jacobian_against_the_first_periods_plan_jacobian():
    """J_X[:, 0] = I and J_X[:, 1] = Ap + Bp K with K = plan_jacobian(...)[:, 0], the local gain of the first period's plan
    (zero without a plan); the goal's Jacobian starts at zero."""
    from qpmpc_amd import closed_loop_jacobian

    c = MC.make("box4", 67, 7)
    sm = model_of("box4")
    ops = operands(c, grad=False)
    kw = dict(goal=ops["goal"], targets=ops["targets"], plant=(ops["Ap"], ops["Bp"]), disturbance=ops["disturbance"],
              feas_tol=c["tol"])
    JX, JU, info = closed_loop_jacobian(sm, ops["x0"], 7, **kw)
    assert tuple(JX.shape) == (67, 8, 4, 4) and tuple(JU.shape) == (67, 7, 2, 4)
    plan = sm.solve(ops["x0"], ops["goal"][:, 0], ops["targets"][:, 0], return_multipliers=True, feas_tol=c["tol"])
    K = sm.plan_jacobian(plan)[0][:, 0].to(F64)  # [B, nu, nx]
    K = torch.where((plan.status == 0)[:, None, None], K, torch.zeros((), dtype=F64, device="cuda"))
    want = ops["Ap"] + torch.bmm(ops["Bp"], K)
    eye = torch.eye(4, dtype=F64, device="cuda").expand(67, 4, 4)
    assert torch.equal(JX[:, 0], eye)
    assert rel(JU[:, 0].cpu().numpy(), K.cpu().numpy()) <= LT.TANGENT_RTOL
    assert rel(JX[:, 1].cpu().numpy(), want.cpu().numpy()) <= LT.TANGENT_RTOL
    assert (info.jvp_status.cpu().numpy() == 0).all() and K.abs().sum() > 0
    c3 = MC.make("triple", 67, 7)  # a goal that is constant over the periods
    GX, GU, _ = closed_loop_jacobian(model_of("triple"), c3["x0"], 7, goal=c3["goal"], disturbance=c3["dist"], feas_tol=c3["tol"],
                                     wrt="goal")
    assert tuple(GX.shape) == (67, 8, 3, 3) and tuple(GU.shape) == (67, 7, 1, 3)
    assert not GX[:, 0].any() and GU.abs().sum() > 0 and torch.isfinite(GX).all()


def test_a_forward_ad_dual_on_x0_through_closed_loop_diff():
    import torch.autograd.forward_ad as fwAD

    from qpmpc_amd import closed_loop_diff, closed_loop_jvp

    c, ref, keep, tan, want = reference("triple", 67, 7, 1)
    sm = model_of("triple")
    x0 = torch.tensor(c["x0"], device="cuda")
    v = torch.tensor(np.ascontiguousarray(tan["x0"][:, 0]), device="cuda")
    kw = dict(goal=torch.tensor(c["goal"], device="cuda"), disturbance=torch.tensor(c["dist"], device="cuda"), feas_tol=c["tol"])
    with fwAD.dual_level():
        X, U0, info = closed_loop_diff(sm, fwAD.make_dual(x0, v), 7, **kw)
        dX, dU0 = fwAD.unpack_dual(X).tangent, fwAD.unpack_dual(U0).tangent
    assert dX is not None and dU0 is not None and info.jvp_status is not None and info.replay_error is not None
    _, _, eX, eU0, _ = closed_loop_jvp(sm, x0, 7, d_x0=v[:, None], **kw)
    assert torch.equal(dX, eX[:, 0]) and torch.equal(dU0, eU0[:, 0])
    only = LT.loop_jvp(c, ref, dict(x0=tan["x0"]))
    err = worst((dX.cpu().numpy()[:, None], dU0.cpu().numpy()[:, None]), only, keep)
    assert max(err.values()) <= LT.TANGENT_RTOL, err
    X2, U2, info2 = closed_loop_diff(sm, x0, 7, **kw)  # without a dual: the records only, nothing replayed
    assert torch.equal(X2, X) and torch.equal(U2, U0) and info2.replay_error is None and info2.jvp_status is None


def test_outside_the_envelope():
    from qpmpc_amd import BackendError, BatchMPCProblem, SharedModel, closed_loop_jvp
    from qpmpc_amd.workloads import triple_integrator_matrices

    A, B, Cm, e = triple_integrator_matrices(20)  # n = 20 > 16
    sm = SharedModel(BatchMPCProblem(A, B, Cm, None, e, 20, 1.0, None, 1e-6, np.zeros((1, 3)), goal_state=np.zeros((1, 3))))
    x0 = torch.zeros((5, 3), dtype=F64, device="cuda")
    goal = torch.tensor([1.0, 0.0, 0.0], dtype=F64, device="cuda")
    eye = torch.eye(3, dtype=F64, device="cuda")[None]
    with pytest.raises(BackendError, match="fused=False"):
        closed_loop_jvp(sm, x0, 2, goal=goal, d_x0=eye)
    X, U0, dX, dU0, info = closed_loop_jvp(sm, x0, 2, goal=goal, d_x0=eye, fused=False)  # ... and the composed loop serves it
    assert tuple(dX.shape) == (5, 3, 3, 3) and tuple(dU0.shape) == (5, 3, 2, 1) and torch.isfinite(dX).all()
    assert info.status.shape == (5, 2)
