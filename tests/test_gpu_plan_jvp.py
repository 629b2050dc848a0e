"""Forward sensitivities of batched plans on the MI355X: mpcqp_plan_jvp_batch (mpcqp_tangent_kernel in
qpmpc_amd/csrc/mpcqp_adjoint.hip) against the NumPy restatement of tests/tangent_np.py on every forward path, its duality
with mpcqp_plan_vjp_batch, plan_jacobian against the LQR gain, shared tangents, unsolved problems, float32 storage and
forward-mode AD through solve_mpc_batch_diff."""

import numpy as np
import pytest

import adjoint_np as AN
import tangent_np as TN
from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from guarded_launch import _random_ltv, _torch  # noqa: E402  (needs torch)
from host_helpers import dims_of as _dims  # noqa: E402

NAMES = dict(x0="initial_state", goal="goal_state", targets="target_states", e="ineq_vector")


def _tangents(w, B, T, rng):
    """Per-problem random tangents {key: [B, T, ...]} of every operand the workload has."""
    N, nx, nu, mk = _dims(w)
    tails = dict(x0=(nx,), goal=(nx,), targets=(N * nx,), e=(N, mk))
    out = {}
    for key, tail in tails.items():
        if w[key] is None or (key == "e" and mk == 0):
            continue
        out[key] = rng.standard_normal((B, T) + tail)
    return out


def _gpu_jvp(bp, plan, tan, states=True):
    torch = _torch()
    from qpmpc_amd import plan_jvp

    kw = {NAMES[k]: torch.as_tensor(v, device=bp.device) for k, v in tan.items()}
    dU, dX = plan_jvp(bp, plan, states=states, **kw)
    torch.cuda.synchronize()
    return dU, dX


def _check_path(w, seed, T=3, limit=64, **solve_kw):
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch

    rng = np.random.default_rng(seed)
    B = np.asarray(w["x0"]).shape[0]
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True, **solve_kw)
    tan = _tangents(w, B, T, rng)
    dU, dX = _gpu_jvp(bp, plan, tan)
    dU = dU.reshape(B, T, -1).cpu().numpy()
    dX = dX.reshape(B, T, -1).cpu().numpy()
    status = plan.status.cpu().numpy()
    vst = plan.jvp_status.cpu().numpy()
    lam = plan.multipliers.cpu().numpy()
    assert (status == 0).mean() >= 0.9, status
    np.testing.assert_array_equal(vst[status != 0], status[status != 0])
    assert (vst == 0).mean() >= 0.9, vst
    checked = 0
    for b in np.flatnonzero(vst == 0)[:limit]:
        w1 = AN.single(w, b)
        for t in range(T):
            ref = TN.jvp(w1, lam[b], {k: v[b, t] for k, v in tan.items()})
            for key, got in (("U", dU[b, t]), ("X", dX[b, t])):
                err = np.abs(got - ref[key]).max()
                assert err <= 1e-8 * max(1.0, np.abs(ref[key]).max()), (b, t, key, err)
        checked += 1
    assert checked >= min(limit, 8)
    return bp, plan, tan, dU, dX


def test_jvp_config2_four_and_two_per_wavefront():
    from qpmpc_amd import _capi

    w = W.triple_integrator_batch(256)
    _check_path(w, 1, flags=_capi.OPT_FOUR_PER_WAVE)
    _check_path(w, 1, flags=_capi.OPT_TWO_PER_WAVE)


def test_jvp_wip_n50():
    _check_path(W.wip_batch(64, N=50), 2, limit=16)


def test_jvp_random_ltv():
    _check_path(_random_ltv(3, 64, 6, 2, 24, 3), 3, limit=32)


def test_jvp_n128_workspace_carve():
    _check_path(_random_ltv(4, 16, 4, 2, 64, 2), 4, T=5, limit=8)


@pytest.mark.parametrize("make", [lambda: W.triple_integrator_batch(128), lambda: W.wip_batch(32, N=50),
                                  lambda: _random_ltv(5, 32, 4, 2, 12, 3)])
def test_duality_with_the_vjp_export(make):
    torch = _torch()
    from qpmpc_amd import autodiff, solve_mpc_batch

    w = make()
    rng = np.random.default_rng(6)
    B = np.asarray(w["x0"]).shape[0]
    N, nx, nu, mk = _dims(w)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    tan = _tangents(w, B, 1, rng)
    dU, dX = _gpu_jvp(bp, plan, tan)
    gU = rng.standard_normal((B, N * nu))
    gX = rng.standard_normal((B, (N + 1) * nx))
    g = autodiff._plan_vjp(bp, plan, torch.as_tensor(gU, device=bp.device), torch.as_tensor(gX, device=bp.device),
                           {"goal", "targets", "e"})
    torch.cuda.synchronize()
    g = dict(zip(("x0", "goal", "targets", "e"), [None if v is None else v.reshape(B, -1).cpu().numpy() for v in g]))
    ok = (plan.vjp_status == 0).cpu().numpy() & (plan.jvp_status == 0).cpu().numpy()
    assert ok.mean() >= 0.9
    fwd = np.concatenate([gU * dU.reshape(B, -1).cpu().numpy(), gX * dX.reshape(B, -1).cpu().numpy()], axis=1)
    rev = np.concatenate([g[k] * v.reshape(B, -1) for k, v in tan.items()], axis=1)
    lhs, rhs = fwd.sum(1), rev.sum(1)
    # relative to the magnitude of the terms (the rounding bound of an inner product; the WIP sums cancel)
    scale = np.maximum(1.0, np.maximum(np.abs(fwd).sum(1), np.abs(rev).sum(1)))
    assert (np.abs(lhs - rhs)[ok] <= 1e-10 * scale[ok]).all(), np.abs(lhs - rhs)[ok].max()


def test_plan_jacobian_unconstrained_is_the_lqr_gain():
    torch = _torch()
    from oracle.stagewise_np import Riccati, from_mpc_problem
    from qpmpc_amd import plan_jacobian, solve_mpc_batch
    from qpmpc_amd.workloads import problem_from_workload

    w = _random_ltv(7, 16, 4, 2, 10, 2)
    w["e"] = np.full_like(w["e"], 1e6)  # no row can be active
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    JU, JX = plan_jacobian(bp, plan, states=True)
    torch.cuda.synchronize()
    assert JU.shape == (16, 10, 2, 4) and JX.shape == (16, 11, 4, 4)
    assert (plan.status == 0).all() and (plan.jvp_status == 0).all() and (plan.multipliers == 0).all()
    JU = JU.cpu().numpy()
    JX = JX.cpu().numpy()
    for b in range(16):
        K0 = Riccati(from_mpc_problem(problem_from_workload(AN.single(w, b), 0))).K[0]
        np.testing.assert_allclose(JU[b, 0], -K0, rtol=0, atol=1e-8 * max(1.0, np.abs(K0).max()))
        np.testing.assert_array_equal(JX[b, 0], np.eye(4))


def test_shared_tangents_are_bitwise_per_problem_copies():
    torch = _torch()
    from qpmpc_amd import plan_jvp, solve_mpc_batch

    w = _random_ltv(8, 48, 3, 2, 8, 2)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    rng = np.random.default_rng(8)
    one = {k: torch.as_tensor(v[:1], device=bp.device) for k, v in _tangents(w, 1, 4, rng).items()}
    per = {k: v.expand(48, *v.shape[1:]).contiguous() for k, v in one.items()}
    dU1, dX1 = plan_jvp(bp, plan, states=True, **{NAMES[k]: v for k, v in one.items()})
    dU2, dX2 = plan_jvp(bp, plan, states=True, **{NAMES[k]: v for k, v in per.items()})
    torch.cuda.synchronize()
    assert torch.equal(dU1, dU2) and torch.equal(dX1, dX2)
    assert dU1.abs().sum() > 0


def test_unsolved_problems_get_zeros():
    torch = _torch()
    from qpmpc_amd import plan_jvp, solve_mpc_batch

    w = _random_ltv(6, 32, 3, 2, 8, 2)
    for b in (3, 7, 20):  # two contradictory rows at step 0
        w["C"][b, 0, 1], w["D"][b, 0, 1] = -w["C"][b, 0, 0], -w["D"][b, 0, 0]
        w["e"][b, 0, :] = -1.0
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True, max_iter=3)
    tan = _tangents(w, 32, 2, np.random.default_rng(9))
    dU, dX = plan_jvp(bp, plan, states=True, **{NAMES[k]: torch.as_tensor(v, device=bp.device) for k, v in tan.items()})
    torch.cuda.synchronize()
    status = plan.status.cpu().numpy()
    assert (status[[3, 7, 20]] != 0).all() and (status == 0).any()
    np.testing.assert_array_equal(plan.jvp_status.cpu().numpy()[status != 0], status[status != 0])
    bad = torch.as_tensor(status != 0, device=bp.device)
    assert (dU[bad] == 0).all() and (dX[bad] == 0).all()
    assert not torch.isnan(dU).any()
    assert dU[~bad].abs().sum() > 0


def test_float32_storage():
    torch = _torch()
    from qpmpc_amd import plan_jvp, solve_mpc_batch

    w = _random_ltv(10, 40, 3, 2, 6, 2)
    tan = _tangents(w, 40, 2, np.random.default_rng(10))
    out = {}
    for dt in (torch.float64, torch.float32):
        bp = W.to_batch_problem(w, dtype=dt)
        plan = solve_mpc_batch(bp, return_multipliers=True)
        dU, dX = plan_jvp(bp, plan, states=True,
                          **{NAMES[k]: torch.as_tensor(v, dtype=dt, device=bp.device) for k, v in tan.items()})
        torch.cuda.synchronize()
        assert dU.dtype == dt and dX.dtype == dt
        same = ((plan.multipliers > 0).cpu().numpy(), (plan.jvp_status == 0).cpu().numpy())
        out[dt] = (dU.double().cpu().numpy(), same)
    (u64, (a64, ok64)), (u32, (a32, ok32)) = out[torch.float64], out[torch.float32]
    same = ok64 & ok32 & (a64 == a32).all(axis=1)
    assert same.mean() >= 0.8
    scale = np.maximum(1.0, np.abs(u64).reshape(40, -1).max(axis=1))
    err = np.abs(u32 - u64).reshape(40, -1).max(axis=1)
    assert (err[same] <= 1e-3 * scale[same]).all()


def _subset(w, idx):
    B = np.asarray(w["x0"]).shape[0]
    out = dict(w)
    for k, v in w.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B:
            out[k] = np.ascontiguousarray(v[idx])
    return out


def test_forward_ad_through_solve_mpc_batch_diff():
    torch = _torch()
    from torch.autograd import forward_ad as fwAD

    from qpmpc_amd import plan_jvp, solve_mpc_batch_diff

    w = _random_ltv(11, 40, 3, 2, 5, 2)
    w = _subset(w, AN.complementary(w, 8))
    bp = W.to_batch_problem(w)
    dev = bp.device
    rng = np.random.default_rng(11)
    prim = {k: torch.as_tensor(w[k], device=dev) for k in ("x0", "goal", "targets", "e")}
    tan = {k: torch.as_tensor(rng.standard_normal(v.shape), device=dev) for k, v in prim.items()}
    with fwAD.dual_level():
        duals = {NAMES[k]: fwAD.make_dual(prim[k], tan[k]) for k in prim}
        U, X, plan = solve_mpc_batch_diff(bp, states=True, **duals)
        tU, tX = fwAD.unpack_dual(U).tangent, fwAD.unpack_dual(X).tangent
    assert tU is not None and tX is not None
    assert (plan.status == 0).all()
    # bitwise the export with T = 1 on the same plan
    N, nx, nu, mk = _dims(w)
    ref_U, ref_X = plan_jvp(bp, plan, states=True, initial_state=tan["x0"][:, None], goal_state=tan["goal"][:, None],
                            target_states=tan["targets"][:, None], ineq_vector=tan["e"][:, None])
    torch.cuda.synchronize()
    assert torch.equal(tU, ref_U[:, 0]) and torch.equal(tX, ref_X[:, 0])
    # central differences of the GPU forward
    step = 1e-6
    outs = []
    for s in (step, -step):
        kw = {NAMES[k]: prim[k] + s * tan[k] for k in prim}
        Up, Xp, pp = solve_mpc_batch_diff(bp, states=True, **kw)
        assert (pp.status == 0).all()
        outs.append((Up, Xp))
    fdU = (outs[0][0] - outs[1][0]) / (2 * step)
    fdX = (outs[0][1] - outs[1][1]) / (2 * step)
    for got, fd in ((tU, fdU), (tX, fdX)):
        scale = fd.abs().flatten(1).max(dim=1).values.clamp(min=1.0)
        err = (got - fd).abs().flatten(1).max(dim=1).values
        assert (err <= 1e-6 * scale).all(), err.max()


def test_forward_ad_partial_tangents_and_no_dual_unchanged():
    torch = _torch()
    from torch.autograd import forward_ad as fwAD

    from qpmpc_amd import plan_jvp, solve_mpc_batch, solve_mpc_batch_diff

    w = W.triple_integrator_batch(64)
    bp = W.to_batch_problem(w)
    x0 = torch.as_tensor(w["x0"], device=bp.device)
    dx = torch.ones_like(x0)
    with fwAD.dual_level():
        U, X, plan = solve_mpc_batch_diff(bp, initial_state=fwAD.make_dual(x0, dx))
        tU = fwAD.unpack_dual(U).tangent
    assert X is None and tU is not None and tU.shape == U.shape
    ref, _ = plan_jvp(bp, plan, initial_state=dx[:, None])
    torch.cuda.synchronize()
    assert torch.equal(tU, ref[:, 0])
    U2, _, p2 = solve_mpc_batch_diff(bp, initial_state=x0)
    assert U2.grad_fn is None and torch.equal(p2.U, solve_mpc_batch(bp).U)


def test_dual_transition_matrix_raises():
    torch = _torch()
    from torch.autograd import forward_ad as fwAD

    from qpmpc_amd import BackendError, solve_mpc_batch_diff

    w = _random_ltv(12, 8, 3, 2, 6, 2)
    bp = W.to_batch_problem(w)
    A = torch.as_tensor(w["A"], device=bp.device)
    with fwAD.dual_level():
        with pytest.raises(BackendError, match="transition_state_matrix"):
            solve_mpc_batch_diff(bp, transition_state_matrix=fwAD.make_dual(A, torch.ones_like(A)))
