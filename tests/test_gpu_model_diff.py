"""Shared-model derivatives on the MI355X: mpcqp_model_vjp_batch / mpcqp_model_jvp_batch (qpmpc_amd/csrc/
mpcqp_model_adjoint.hip) against the NumPy restatement of tests/model_adjoint_np.py at 1e-8 max(1, |ref|), on the shapes at
which each of the two kernels can go wrong; against mpcqp_plan_vjp_batch / mpcqp_plan_jvp_batch on the same batch and
plan; and the Python surface (SharedModel.solve_diff, .plan_jvp, .plan_jacobian)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import adjoint_np as AN
import model_adjoint_np as MN
from qpmpc_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from guarded_launch import _torch  # noqa: E402  (needs torch)

TOL = MN.TOL
NOT_PD = 3
_REF = {}


def _max_grid():
    """Workgroups a round of the small kernel's launch helper runs at most (sixteen problems each)."""
    src = open(os.path.join(ROOT, "qpmpc_amd", "csrc", "mpcqp_internal.h")).read()
    return int(re.search(r"kModelDiffMaxGrid = (\d+);", src).group(1))


def _triple(N, batch=32, e=2.0, seed=3):
    A, B, C, _ = W.triple_integrator_matrices(N)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-0.5, 0.5, batch), rng.uniform(-0.5, 0.5, batch), rng.uniform(-0.9 * e, 0.9 * e, batch)], 1)
    goal = np.stack([rng.uniform(0.5, 1.5, batch), np.zeros(batch), np.zeros(batch)], 1)
    return dict(A=A, B=B, C=C, D=None, e=np.array([e, e]), N=N, wt=1.0, wx=None, wu=1e-6, x0=x0,
                goal=goal, targets=None, name=f"triple_N{N}")


def _wip50(batch=8):
    w = W.wip_batch(batch, N=50, ltv=False)
    w.pop("pendulum", None)
    w["e"] = 0.25 * np.asarray(w["e"])
    return w


CASES = {
    "triple_n5": lambda: _triple(5, e=1.0),                   # n = 5 padded to 16, m = 10
    "triple_n16": lambda: _triple(16),                        # the full tile: n = 16, m = 32
    "mixed": lambda: MN.mixed_batch(24),                      # nx = 4, nu = 2, N = 8: stage cost, input rows
    "triple_n17": lambda: _triple(17, batch=8),               # first size of the general kernel
    "wip_n50": _wip50,                                        # n = 50, m = 100
    "mixed_n64": lambda: MN.mixed_batch(5, seed=9, nu=2, N=32),      # the envelope's end
}
SMALL, GENERAL = ("triple_n5", "triple_n16", "mixed"), ("triple_n17", "wip_n50", "mixed_n64")


def _case(name):
    """(workload, NumPy model), computed once per case and never changed."""
    if name not in _REF:
        w = CASES[name]()
        _REF[name] = (w, MN.NumpyModel(w))
    return _REF[name]


def _head(w, count):
    B = np.asarray(w["x0"]).shape[0]
    out = dict(w)
    for k in ("x0", "goal", "targets"):
        if w[k] is not None and np.asarray(w[k]).shape[0] == B:
            out[k] = np.ascontiguousarray(np.asarray(w[k])[:count])
    return out


def _solve(w, dtype=None):
    torch = _torch()
    from qpmpc_amd import SharedModel

    bp = W.to_batch_problem(w, dtype=dtype)
    sm = SharedModel(bp)
    plan = sm.solve(bp.initial_state, bp.goal_state, bp.target_states, return_multipliers=True)
    torch.cuda.synchronize()
    return bp, sm, plan


def _fake_plan(plan, lam=None, status=None):
    torch = _torch()
    dev = plan.U.device
    return SimpleNamespace(U=plan.U, multipliers=plan.multipliers if lam is None else torch.as_tensor(lam, device=dev),
                           status=plan.status if status is None else torch.as_tensor(status, dtype=torch.int32,
                                                                                      device=dev))


def _run_vjp(sm, plan, gU, gX):
    torch = _torch()
    from qpmpc_amd import model_diff

    dev = plan.U.device
    g = model_diff.model_vjp(sm, plan, torch.as_tensor(gU, device=dev), None if gX is None else
                             torch.as_tensor(gX, device=dev), {"goal", "targets", "e"})
    torch.cuda.synchronize()
    B = gU.shape[0]
    return (dict(zip(("x0", "goal", "targets", "e"), [None if v is None else v.reshape(B, -1).cpu().numpy() for v in g])),
            plan.vjp_status.cpu().numpy())


def _run_jvp(sm, plan, tan, states=True):
    torch = _torch()
    from qpmpc_amd import model_diff

    dev = plan.U.device
    names = dict(x0="initial_state", goal="goal_state", targets="target_states", e="ineq_vector")
    dU, dX = model_diff.model_jvp(sm, plan, states=states,
                                  **{names[k]: torch.as_tensor(v, device=dev) for k, v in tan.items()})
    torch.cuda.synchronize()
    B = dU.shape[0]
    return (dU.reshape(B, dU.shape[1], -1).cpu().numpy(),
            None if dX is None else dX.reshape(B, dX.shape[1], -1).cpu().numpy(), plan.jvp_status.cpu().numpy())


def _tangents(model, B, T, rng, shared=False):
    lead = 1 if shared else B
    tan = dict(x0=rng.standard_normal((lead, T, model.nx)), goal=rng.standard_normal((lead, T, model.nx)),
               targets=rng.standard_normal((lead, T, model.N * model.nx)))
    if model.m:
        tan["e"] = rng.standard_normal((lead, T, model.N, model.m // model.N))
    return tan


def _assert_close(got, ref, what):
    err = np.abs(got - ref).max() if ref.size else 0.0
    assert err <= TOL * max(1.0, np.abs(ref).max() if ref.size else 0.0), (what, err)
    return err


def _check(name, batch, T=3, gx=True, states=True, shared=False, seed=0):
    """Both exports on the first `batch` problems of a case, every solved problem against the restatement."""
    w, model = _case(name)
    w = _head(w, batch)
    rng = np.random.default_rng(seed)
    bp, sm, plan = _solve(w)
    lam, status = plan.multipliers.cpu().numpy(), plan.status.cpu().numpy()
    gU = rng.standard_normal((batch, model.n))
    gX = rng.standard_normal((batch, (model.N + 1) * model.nx)) if gx else None
    g, vst = _run_vjp(sm, plan, gU, gX)
    tan = _tangents(model, batch, T, rng, shared)
    dU, dX, jst = _run_jvp(sm, plan, tan, states)
    assert (dX is None) == (not states)
    active = 0
    for b in range(batch):
        if status[b] != 0:
            assert vst[b] == status[b] and jst[b] == status[b]
            assert all(np.all(v[b] == 0) for v in g.values()) and np.all(dU[b] == 0)
            continue
        assert vst[b] == 0 and jst[b] == 0, (b, vst[b], jst[b])
        active += int((lam[b] > 0).any())
        ref = model.vjp(lam[b], gU[b], None if gX is None else gX[b])
        for key in ("x0", "goal", "targets", "e"):
            _assert_close(g[key][b], ref[key], (name, b, key))
        for t in range(T):
            rj = model.jvp(lam[b], {k: v[0 if shared else b, t] for k, v in tan.items()})
            _assert_close(dU[b, t], rj["U"], (name, b, t, "dU"))
            if states:
                _assert_close(dX[b, t], rj["X"], (name, b, t, "dX"))
    assert (status == 0).any()
    return active


# ------------------------------------------------------------------------------------------- the small kernel
@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("batch", [1, 7])
def test_small_kernel_against_the_restatement(name, batch):
    """One problem, and a last wavefront that holds three."""
    active = _check(name, batch)
    assert batch == 1 or active >= 1


@pytest.mark.parametrize("name,kw", [("triple_n16", dict(gx=False)), ("mixed", dict(states=False, T=1)),
                                     ("mixed", dict(shared=True, T=4)), ("triple_n5", dict(shared=True, T=3))])
def test_small_kernel_export_options(name, kw):
    """gX and dX NULL, one tangent, nx identity-sized sets, a tangent set shared by the batch (stride 0)."""
    assert _check(name, 24, seed=1, **kw) >= 6


def test_small_kernel_second_round_of_every_workgroup():
    """More problems than one round of the launch helper's grid holds: every workgroup takes a second round."""
    torch = _torch()
    w, model = _case("triple_n5")
    tile = 32
    batch = _max_grid() * 16 * 2 + 5
    idx = np.arange(batch) % tile
    big = dict(w)
    big["x0"], big["goal"] = w["x0"][idx], w["goal"][idx]
    rng = np.random.default_rng(2)
    gU1, gX1 = rng.standard_normal((tile, model.n)), rng.standard_normal((tile, (model.N + 1) * model.nx))
    bp, sm, plan = _solve(big)
    g, vst = _run_vjp(sm, plan, gU1[idx], gX1[idx])
    tan1 = _tangents(model, tile, 1, rng)
    dU, dX, jst = _run_jvp(sm, plan, {k: v[idx] for k, v in tan1.items()})
    lam, status = plan.multipliers.cpu().numpy(), plan.status.cpu().numpy()
    np.testing.assert_array_equal(vst, status)
    np.testing.assert_array_equal(jst, status)
    for b in range(tile):  # the reference once per distinct problem, compared with every copy
        copies = np.flatnonzero(idx == b)
        assert (np.abs(lam[copies] - lam[b]).max() == 0.0) and (status[copies] == status[b]).all()
        if status[b] != 0:
            assert np.all(g["x0"][copies] == 0) and np.all(dU[copies] == 0)
            continue
        ref = model.vjp(lam[b], gU1[b], gX1[b])
        for key in ("x0", "goal", "e"):
            _assert_close(g[key][copies], np.broadcast_to(ref[key], g[key][copies].shape), (b, key))
        rj = model.jvp(lam[b], {k: v[b, 0] for k, v in tan1.items()})
        _assert_close(dU[copies, 0], np.broadcast_to(rj["U"], dU[copies, 0].shape), (b, "dU"))
        _assert_close(dX[copies, 0], np.broadcast_to(rj["X"], dX[copies, 0].shape), (b, "dX"))
    assert not torch.isnan(plan.U).any()


def test_mixed_wavefronts_status_passthrough_and_singular_problems():
    """Problems with zero, some and many active rows, problems whose status is forced non-zero and problems with hand-made
    multipliers on more rows than there are variables alternate inside every wavefront: the latter two get zeros (and the
    forward status, MPCQP_NOT_PD), their neighbours are unaffected."""
    w, model = _case("triple_n16")
    batch = 30
    w = _head(w, batch)
    bp, sm, plan = _solve(w)
    lam, status = plan.multipliers.cpu().numpy().copy(), plan.status.cpu().numpy().copy()
    forced = np.arange(batch) % 4 == 1
    singular = np.arange(batch) % 8 == 2
    slack = np.arange(batch) % 8 == 4
    status[forced] = 2
    lam[forced] = np.nan  # not read
    lam[singular] = 0.0
    lam[singular, :17] = 1.0  # 17 rows on 16 variables
    status[singular] = 0
    lam[slack] = 0.0          # k = 0
    status[slack] = 0
    fake = _fake_plan(plan, lam, status)
    rng = np.random.default_rng(4)
    gU, gX = rng.standard_normal((batch, model.n)), rng.standard_normal((batch, (model.N + 1) * model.nx))
    g, vst = _run_vjp(sm, fake, gU, gX)
    tan = _tangents(model, batch, 2, rng)
    dU, dX, jst = _run_jvp(sm, fake, tan)
    counts = set()
    for b in range(batch):
        if forced[b] or singular[b] or status[b] != 0:
            want = NOT_PD if singular[b] else status[b]
            assert vst[b] == want and jst[b] == want, (b, vst[b], jst[b])
            assert all(np.all(v[b] == 0) for v in g.values()) and np.all(dU[b] == 0) and np.all(dX[b] == 0)
            continue
        assert vst[b] == 0 and jst[b] == 0
        counts.add(int((lam[b] > 0).sum()))
        ref = model.vjp(lam[b], gU[b], gX[b])
        for key in ("x0", "goal", "e"):
            _assert_close(g[key][b], ref[key], (b, key))
        for t in range(2):
            rj = model.jvp(lam[b], {k: v[b, t] for k, v in tan.items()})
            _assert_close(dU[b, t], rj["U"], (b, t, "dU"))
            _assert_close(dX[b, t], rj["X"], (b, t, "dX"))
    assert 0 in counts and max(counts) >= 4, counts


# ------------------------------------------------------------------------------------------- the general kernel
@pytest.mark.parametrize("name", GENERAL)
def test_general_kernel_against_the_restatement(name):
    assert _check(name, 5, T=2) >= 1


def test_general_kernel_singular_and_unsolved():
    w, model = _case("triple_n17")
    w = _head(w, 5)
    bp, sm, plan = _solve(w)
    lam, status = plan.multipliers.cpu().numpy().copy(), plan.status.cpu().numpy().copy()
    lam[1], status[1] = 1.0, 0    # 34 rows on 17 variables
    lam[3], status[3] = np.nan, 1  # not read
    fake = _fake_plan(plan, lam, status)
    rng = np.random.default_rng(5)
    gU = rng.standard_normal((5, model.n))
    g, vst = _run_vjp(sm, fake, gU, None)
    dU, dX, jst = _run_jvp(sm, fake, _tangents(model, 5, 2, rng))
    assert vst[1] == NOT_PD and jst[1] == NOT_PD and vst[3] == 1 and jst[3] == 1
    for b in (1, 3):
        assert all(np.all(v[b] == 0) for v in g.values()) and np.all(dU[b] == 0) and np.all(dX[b] == 0)
    for b in (0, 2, 4):
        if status[b] == 0:
            _assert_close(g["x0"][b], model.vjp(lam[b], gU[b])["x0"], b)


def test_n65_is_unsupported_and_no_rows_need_no_multipliers():
    import ctypes as C

    torch = _torch()
    from qpmpc_amd import _capi
    from qpmpc_amd.batch import _stream_ptr

    lib = _capi.load()
    dev = _capi.require_gpu()
    w, model = _case("triple_n17")
    n, nx, N = model.n, model.nx, model.N
    f64 = dict(dtype=torch.float64, device=dev)
    dims = _capi.Dims(nx, 1, N, 0, _capi.F64, _capi.P_TERMINAL | _capi.Q_TERMINAL, 1.0, 0.0, float(w["wu"]))
    # the model of the same dynamics without rows (mk = 0), from the restatement's P and q basis
    Qg = -(model.L @ model.Wg)
    qb = np.concatenate([np.zeros((1, n)), (model.L @ model.Wx).T, Qg.T, np.zeros((N * nx, n))])
    nbytes = C.c_size_t(0)
    assert lib.mpcqp_model_bytes(C.byref(dims), C.byref(nbytes)) == 0
    mem = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    P, qbt = torch.as_tensor(model.P, **f64).contiguous(), torch.as_tensor(qb, **f64).contiguous()
    assert lib.mpcqp_factor_model(C.byref(dims), P.data_ptr(), None, qbt.data_ptr(), None, mem.data_ptr(), nbytes.value,
                                  _stream_ptr()) == 0
    B = 3
    rng = np.random.default_rng(6)
    gU = rng.standard_normal((B, n))
    dx0 = rng.standard_normal((B, 2, nx))
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    gUt, dxt = torch.as_tensor(gU, **f64), torch.as_tensor(dx0, **f64)
    g_x0, g_goal = torch.empty((B, nx), **f64), torch.empty((B, nx), **f64)
    dU = torch.empty((B, 2, n), **f64)
    st = torch.full((2, B), -1, dtype=torch.int32, device=dev)
    tan = _capi.Tangents(dxt.data_ptr(), None, None, None, 2 * nx, 0, 0, 0)
    assert lib.mpcqp_model_vjp_batch(C.byref(dims), mem.data_ptr(), B, None, status.data_ptr(), gUt.data_ptr(), None, None,
                                     None, g_x0.data_ptr(), g_goal.data_ptr(), None, None, st[0].data_ptr(),
                                     _stream_ptr()) == 0
    assert lib.mpcqp_model_jvp_batch(C.byref(dims), mem.data_ptr(), B, 2, None, status.data_ptr(), C.byref(tan), None, None,
                                     dU.data_ptr(), None, st[1].data_ptr(), _stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (st == 0).all()
    none = np.zeros(model.m)
    for b in range(B):
        ref = model.vjp(none, gU[b])
        _assert_close(g_x0[b].cpu().numpy(), ref["x0"], (b, "x0"))
        _assert_close(g_goal[b].cpu().numpy(), ref["goal"], (b, "goal"))
        for t in range(2):
            _assert_close(dU[b, t].cpu().numpy(), model.jvp(none, dict(x0=dx0[b, t]))["U"], (b, t))
    big = _capi.Dims(nx, 1, 65, 2, _capi.F64, dims.flags, 1.0, 0.0, 1e-3)
    assert lib.mpcqp_model_vjp_batch(C.byref(big), mem.data_ptr(), B, gUt.data_ptr(), status.data_ptr(), gUt.data_ptr(), None,
                                     None, None, g_x0.data_ptr(), None, None, None, None, _stream_ptr()) == -6
    assert lib.mpcqp_model_jvp_batch(C.byref(big), mem.data_ptr(), B, 2, gUt.data_ptr(), status.data_ptr(), C.byref(tan), None,
                                     None, dU.data_ptr(), None, None, _stream_ptr()) == -6


# ------------------------------------------------------------------------------------------- the existing exports
@pytest.mark.parametrize("name", ["triple_n16", "mixed", "wip_n50"])
def test_against_the_condensed_exports_on_the_same_plan(name):
    """mpcqp_plan_vjp_batch / mpcqp_plan_jvp_batch factor every problem's own P; the model exports read the model's factor:
    two correct factorisations of the same KKT system, held to the bound of the other tests. Largest relative gap
    observed on an MI355X (printed by every run): 4.0e-14 on triple_n16, 2.4e-13 on mixed, 3.1e-12 on wip_n50."""
    torch = _torch()
    from qpmpc_amd import autodiff, plan_jvp

    w, model = _case(name)
    B = min(np.asarray(w["x0"]).shape[0], 24)
    w = _head(w, B)
    bp, sm, plan = _solve(w)
    rng = np.random.default_rng(7)
    gU, gX = rng.standard_normal((B, model.n)), rng.standard_normal((B, (model.N + 1) * model.nx))
    g, vst = _run_vjp(sm, plan, gU, gX)
    tan = {k: v for k, v in _tangents(model, B, 2, rng).items() if k in ("x0", "e") or w[k] is not None}
    dU, dX, jst = _run_jvp(sm, plan, tan)
    dev = bp.device
    old = autodiff._plan_vjp(bp, plan, torch.as_tensor(gU, device=dev), torch.as_tensor(gX, device=dev),
                             {"goal", "targets", "e"})
    old_status = plan.vjp_status.cpu().numpy()
    names = dict(x0="initial_state", goal="goal_state", targets="target_states", e="ineq_vector")
    oU, oX = plan_jvp(bp, plan, states=True, **{names[k]: torch.as_tensor(v, device=dev) for k, v in tan.items()})
    torch.cuda.synchronize()
    np.testing.assert_array_equal(vst, old_status)
    np.testing.assert_array_equal(jst, plan.jvp_status.cpu().numpy())
    gap = 0.0
    for key, o in zip(("x0", "goal", "targets", "e"), old[:4]):
        if o is None:
            continue
        ref = o.reshape(B, -1).cpu().numpy()
        gap = max(gap, _assert_close(g[key], ref, (name, key)) / max(1.0, np.abs(ref).max()))
    for got, o in ((dU, oU), (dX, oX)):
        ref = o.reshape(B, 2, -1).cpu().numpy()
        gap = max(gap, _assert_close(got, ref, name) / max(1.0, np.abs(ref).max()))
    print(f"model exports against the condensed ones, {name}: largest relative gap {gap:.3e}")


# ------------------------------------------------------------------------------------------- the Python surface
def _complementary(w, count):
    picked = [b for b, c in enumerate(MN.census(w)) if c[3]][:count]
    assert len(picked) == count
    return picked


def _pick(w, idx):
    out = dict(w)
    for k in ("x0", "goal", "targets"):
        if w[k] is not None:
            out[k] = np.ascontiguousarray(np.asarray(w[k])[idx])
    return out


@pytest.mark.parametrize("states", [False, True])
def test_gradcheck_through_solve_diff(states):
    torch = _torch()
    from qpmpc_amd import SharedModel

    w, _ = _case("mixed")
    w = _pick(w, _complementary(w, 4))
    bp = W.to_batch_problem(w)
    sm = SharedModel(bp)
    dev = bp.device
    x0 = torch.as_tensor(w["x0"], device=dev).clone().requires_grad_()
    goal = torch.as_tensor(w["goal"], device=dev).clone().requires_grad_()
    tg = torch.as_tensor(w["targets"], device=dev).clone().requires_grad_()
    e = torch.as_tensor(np.broadcast_to(w["e"], (4, 8, 3)).copy(), device=dev).requires_grad_()

    def f(x0, goal, tg, e):
        U, X, _ = sm.solve_diff(x0, goal, tg, ineq_vector=e, states=states)
        return (U, X) if states else U

    assert torch.autograd.gradcheck(f, (x0, goal, tg, e), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_shared_goal_gets_the_batch_sum_and_float32_agrees():
    torch = _torch()
    from qpmpc_amd import SharedModel

    w, model = _case("triple_n16")
    w = _head(w, 24)
    grads = {}
    for dt in (torch.float64, torch.float32):
        bp = W.to_batch_problem(w, dtype=dt)
        sm = SharedModel(bp)
        x0 = bp.initial_state.clone().requires_grad_()
        goal = torch.as_tensor(w["goal"][0], dtype=dt, device=bp.device).requires_grad_()  # [nx]: shared by the batch
        U, X, plan = sm.solve_diff(x0, goal, states=True)
        assert U.grad_fn is not None and X.grad_fn is not None and U.dtype == dt
        (U.square().sum() + X[:, -1].sum()).backward()
        torch.cuda.synchronize()
        assert goal.grad.shape == goal.shape and goal.grad.dtype == dt
        grads[dt] = (x0.grad.double().cpu().numpy(), goal.grad.double().cpu().numpy(), plan)
        if dt == torch.float64:
            lam, st = plan.multipliers.cpu().numpy(), plan.status.cpu().numpy()
            Un, Xn = U.detach().cpu().numpy().reshape(24, -1), X.detach().cpu().numpy()
            total = np.zeros(model.nx)
            for b in np.flatnonzero(st == 0):
                gX = np.zeros((model.N + 1, model.nx))
                gX[-1] = 1.0
                ref = model.vjp(lam[b], 2 * Un[b], gX)
                total += ref["goal"]
                _assert_close(grads[dt][0][b], ref["x0"], (b, "x0"))
            _assert_close(grads[dt][1], total, "shared goal")
    (x64, g64, p64), (x32, g32, p32) = grads[torch.float64], grads[torch.float32]
    same = ((p64.status == 0) & (p32.status == 0)).cpu().numpy() & \
        ((p64.multipliers > 0) == (p32.multipliers > 0)).all(dim=1).cpu().numpy()
    assert same.mean() >= 0.8
    scale = np.maximum(1.0, np.abs(x64).max(axis=1))
    assert (np.abs(x32 - x64).max(axis=1)[same] <= 1e-3 * scale[same]).all()
    if same.all():  # the batch sum is comparable only where every problem kept its active set
        assert np.abs(g32 - g64).max() <= 1e-3 * max(1.0, np.abs(x64).max(), np.abs(g64).max())
    # with nothing requiring grad it is solve()
    U0, X0, plan0 = sm.solve_diff(bp.initial_state, bp.goal_state)
    assert U0.grad_fn is None and X0 is None and torch.equal(plan0.U, sm.solve(bp.initial_state, bp.goal_state).U)


def test_forward_ad_duals_agree_with_plan_jvp():
    torch = _torch()
    from torch.autograd import forward_ad as fwAD

    from qpmpc_amd import SharedModel

    w, _ = _case("mixed")
    bp = W.to_batch_problem(w)
    sm = SharedModel(bp)
    dev = bp.device
    rng = np.random.default_rng(8)
    prim = {k: torch.as_tensor(w[k], device=dev) for k in ("x0", "goal", "targets")}
    tan = {k: torch.as_tensor(rng.standard_normal(v.shape), device=dev) for k, v in prim.items()}
    with fwAD.dual_level():
        U, X, plan = sm.solve_diff(*[fwAD.make_dual(prim[k], tan[k]) for k in ("x0", "goal", "targets")], states=True)
        tU, tX = fwAD.unpack_dual(U).tangent, fwAD.unpack_dual(X).tangent
    rU, rX = sm.plan_jvp(plan, initial_state=tan["x0"][:, None], goal_state=tan["goal"][:, None],
                         target_states=tan["targets"][:, None], states=True)
    torch.cuda.synchronize()
    assert torch.equal(tU, rU[:, 0]) and torch.equal(tX, rX[:, 0]) and tU.abs().sum() > 0


def test_plan_jacobian_unconstrained_is_the_lqr_gain():
    torch = _torch()
    from oracle.stagewise_np import Riccati, from_mpc_problem
    from qpmpc_amd import SharedModel
    from qpmpc_amd.workloads import problem_from_workload

    w = dict(MN.mixed_batch(6))
    w["e"] = np.full(3, 1e6)  # no row can be active
    bp = W.to_batch_problem(w)
    sm = SharedModel(bp)
    plan = sm.solve(bp.initial_state, bp.goal_state, bp.target_states, return_multipliers=True)
    JU, JX = sm.plan_jacobian(plan, states=True)
    torch.cuda.synchronize()
    assert JU.shape == (6, 8, 2, 4) and JX.shape == (6, 9, 4, 4)
    assert (plan.status == 0).all() and (plan.jvp_status == 0).all() and (plan.multipliers == 0).all()
    K0 = Riccati(from_mpc_problem(problem_from_workload(AN.single(w, 0), 0))).K[0]
    for b in range(6):
        np.testing.assert_allclose(JU[b, 0].cpu().numpy(), -K0, rtol=0, atol=1e-8 * max(1.0, np.abs(K0).max()))
        np.testing.assert_array_equal(JX[b, 0].cpu().numpy(), np.eye(4))


def test_plan_jacobian_with_active_rows_against_the_restatement():
    """The nx identity tangents (ntan = nx, one set shared by the batch) on problems with active rows, both kernels."""
    torch = _torch()
    for name, count in (("mixed", 12), ("wip_n50", 5)):
        w, model = _case(name)
        bp, sm, plan = _solve(_head(w, count))
        JU, JX = sm.plan_jacobian(plan, states=True)
        torch.cuda.synchronize()
        lam, status = plan.multipliers.cpu().numpy(), plan.status.cpu().numpy()
        JU, JX = JU.reshape(count, model.n, model.nx).cpu().numpy(), JX.reshape(count, -1, model.nx).cpu().numpy()
        active = 0
        for b in np.flatnonzero(status == 0):
            active += int((lam[b] > 0).sum() > 0)
            for j in range(model.nx):
                ref = model.jvp(lam[b], dict(x0=np.eye(model.nx)[j]))
                _assert_close(JU[b, :, j], ref["U"], (name, b, j, "JU"))
                _assert_close(JX[b, :, j], ref["X"], (name, b, j, "JX"))
        assert active >= 3, (name, active)


# ------------------------------------------------------------------------------------------- failed factorisations
@pytest.mark.parametrize("N", [8, 9])  # n = 16, m = 32: sixteen lanes per problem; n = 18: a workgroup per problem
def test_zero_pivot_gives_not_pd_and_leaves_the_neighbours_alone(N):
    """A row of zeros (a padding row) with a hand-made positive multiplier makes a diagonal entry of S exactly 0: the
    pivot test fails on every build, in the middle of the factorisation (the row's slot follows the solve's own active
    rows). Such problems sit between solved neighbours of the same wavefront; both directions."""
    w = MN.mixed_batch(14, zero_row=True, N=N)
    model = MN.NumpyModel(w)
    assert np.all(model.M[3::4] == 0.0)
    batch = 14
    bp, sm, plan = _solve(w)
    lam, status = plan.multipliers.cpu().numpy().copy(), plan.status.cpu().numpy().copy()
    assert (lam[:, 3::4] == 0).all() and (status == 0).sum() >= 10
    broken = np.zeros(batch, dtype=bool)
    broken[[1, 6, 7, 12]] = True
    broken &= status == 0
    assert broken.sum() >= 3
    lam[broken, 4 * (N - 1) + 3] = 1.0  # the last step's zero row: the last slot of the problem
    lam[1, 3] = 1.0                      # ... and for one problem also the first slot
    rng = np.random.default_rng(N)
    gU, gX = rng.standard_normal((batch, model.n)), rng.standard_normal((batch, (model.N + 1) * model.nx))
    fake = _fake_plan(plan, lam, status)
    g, vst = _run_vjp(sm, fake, gU, gX)
    tan = _tangents(model, batch, 2, rng)
    dU, dX, jst = _run_jvp(sm, fake, tan)
    for b in range(batch):
        if broken[b] or status[b] != 0:
            want = NOT_PD if broken[b] else status[b]
            assert vst[b] == want and jst[b] == want, (b, vst[b], jst[b])
            assert all(np.all(v[b] == 0) for v in g.values()) and np.all(dU[b] == 0) and np.all(dX[b] == 0), b
            continue
        assert vst[b] == 0 and jst[b] == 0
        ref = model.vjp(lam[b], gU[b], gX[b])
        for key in ("x0", "goal", "targets", "e"):
            _assert_close(g[key][b], ref[key], (b, key))
        for t in range(2):
            rj = model.jvp(lam[b], {k: v[b, t] for k, v in tan.items()})
            _assert_close(dU[b, t], rj["U"], (b, t, "dU"))
            _assert_close(dX[b, t], rj["X"], (b, t, "dX"))
    for v in list(g.values()) + [dU, dX]:
        assert not np.isnan(v).any()


def _raw_model(dims, P, qb):
    """mpcqp_factor_model of a model without rows from P and the q basis; the model's bytes."""
    import ctypes as C

    torch = _torch()
    from qpmpc_amd import _capi
    from qpmpc_amd.batch import _stream_ptr

    lib = _capi.load()
    dev = _capi.require_gpu()
    nbytes = C.c_size_t(0)
    assert lib.mpcqp_model_bytes(C.byref(dims), C.byref(nbytes)) == 0
    mem = torch.zeros((nbytes.value,), dtype=torch.uint8, device=dev)
    Pt = torch.as_tensor(P, dtype=torch.float64, device=dev).contiguous()
    qt = torch.as_tensor(qb, dtype=torch.float64, device=dev).contiguous()
    assert lib.mpcqp_factor_model(C.byref(dims), Pt.data_ptr(), None, qt.data_ptr(), None, mem.data_ptr(), nbytes.value,
                                  _stream_ptr()) == 0
    torch.cuda.synchronize()
    return mem


@pytest.mark.parametrize("N", [16, 17])  # the small and the general kernel
def test_a_model_whose_P_is_not_positive_definite(N):
    import ctypes as C

    torch = _torch()
    from qpmpc_amd import _capi
    from qpmpc_amd.batch import _stream_ptr

    lib = _capi.load()
    dev = _capi.require_gpu()
    nx, n, B, T = 3, N, 6, 2
    dims = _capi.Dims(nx, 1, N, 0, _capi.F64, _capi.P_TERMINAL | _capi.Q_TERMINAL, 1.0, 0.0, 1e-3)
    P = np.eye(n)
    P[n // 2, n // 2] = -1.0
    mem = _raw_model(dims, P, np.zeros((1 + 2 * nx + N * nx, n)))
    f64 = dict(dtype=torch.float64, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    status[2] = 2
    gU, dx0 = torch.randn((B, n), **f64), torch.randn((B, T, nx), **f64)
    out = {k: torch.full(shape, float("nan"), **f64) for k, shape in
           dict(g_x0=(B, nx), g_goal=(B, nx), g_targets=(B, N * nx), dU=(B, T, n)).items()}
    st = torch.full((2, B), -1, dtype=torch.int32, device=dev)
    tan = _capi.Tangents(dx0.data_ptr(), None, None, None, T * nx, 0, 0, 0)
    assert lib.mpcqp_model_vjp_batch(C.byref(dims), mem.data_ptr(), B, None, status.data_ptr(), gU.data_ptr(), None, None,
                                     None, out["g_x0"].data_ptr(), out["g_goal"].data_ptr(), out["g_targets"].data_ptr(),
                                     None, st[0].data_ptr(), _stream_ptr()) == 0
    assert lib.mpcqp_model_jvp_batch(C.byref(dims), mem.data_ptr(), B, T, None, status.data_ptr(), C.byref(tan), None, None,
                                     out["dU"].data_ptr(), None, st[1].data_ptr(), _stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (st == NOT_PD).all()  # every problem, whatever its forward status
    for k, v in out.items():
        assert (v == 0).all(), k


@pytest.mark.parametrize("name", ["triple_n5", "mixed", "wip_n50"])
def test_the_device_model_is_the_restatements(name):
    """What mpcqp_factor_model wrote, map by map, against the NumPy model; the maps of a term that does not enter q are
    exact zeros on the device too (the kernels do not rely on it: they test the flag)."""
    torch = _torch()
    w, model = _case(name)
    bp, sm, plan = _solve(_head(w, 2))
    n, m, nx, N = model.n, model.m, model.nx, model.N
    nc, nT = max(n, 16), N * nx
    mem = sm.model.view(torch.float64).cpu().numpy()
    off, parts = 0, {}
    for key, count in (("M", m * nc), ("Lt", nc * nc), ("invn", m), ("e", m), ("Hx", m * nx), ("Wx", nc * nx),
                       ("Wg", nc * nx), ("Wt", nc * nT)):
        parts[key] = mem[off:off + count]
        off += (count + 3) & ~3
    assert mem[off] == 0.0  # P is positive definite
    Linv_t = np.linalg.inv(model.L).T
    for key, ref, cols in (("M", model.M, nc), ("Lt", Linv_t, nc), ("Hx", model.Hx, nx), ("Wx", model.Wx, nx),
                           ("Wg", model.Wg, nx), ("Wt", model.Wt, nT)):
        got = parts[key].reshape(-1, cols)
        got = got[:ref.shape[0], :ref.shape[1]] if key in ("M", "Lt") else got[:ref.shape[0]]
        _assert_close(got, ref, (name, key))
    if w["targets"] is None:
        assert np.all(parts["Wt"] == 0.0)
    if n < 16:  # the padded unit variables
        np.testing.assert_array_equal(parts["Lt"].reshape(16, 16)[n:, n:], np.eye(16 - n))
        assert np.all(parts["M"].reshape(m, 16)[:, n:] == 0.0)
