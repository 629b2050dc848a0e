"""Gradients through batched plans on the MI355X: mpcqp_plan_vjp_batch (qpmpc_amd/csrc/mpcqp_adjoint.hip) against the
NumPy restatement of tests/adjoint_np.py on every forward path, torch.autograd.gradcheck of solve_mpc_batch_diff,
unsolved problems, shared operands, float32 storage and the envelope."""

import numpy as np
import pytest

import adjoint_np as AN
from oracle.condense_np import condense
from qpmpc_amd import workloads as W
from qpmpc_amd.workloads import problem_from_workload

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from guarded_launch import _random_ltv, _torch  # noqa: E402  (needs torch)

KEYS = ("x0", "goal", "targets", "e")


def _gpu_vjp(w, gU, gX, **solve_kw):
    """(plan, {key: [B, ...] numpy}) : forward solve with multipliers, then mpcqp_plan_vjp_batch."""
    torch = _torch()
    from qpmpc_amd import autodiff, solve_mpc_batch

    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True, **solve_kw)
    g = autodiff._plan_vjp(bp, plan, torch.as_tensor(gU, device=bp.device), torch.as_tensor(gX, device=bp.device),
                           set(KEYS))
    torch.cuda.synchronize()
    return plan, {k: v.cpu().numpy().reshape(v.shape[0], -1) for k, v in zip(KEYS, g)}


def _check_path(w, batch, seed, **solve_kw):
    rng = np.random.default_rng(seed)
    N, nx = int(w["N"]), np.asarray(w["x0"]).shape[1]
    n = N * np.asarray(w["B"]).shape[-1]
    gU = rng.standard_normal((batch, n))
    gX = rng.standard_normal((batch, (N + 1) * nx))
    plan, g = _gpu_vjp(w, gU, gX, **solve_kw)
    status = plan.status.cpu().numpy()
    vst = plan.vjp_status.cpu().numpy()
    lam = plan.multipliers.cpu().numpy()
    U = plan.U.cpu().numpy()
    assert (status == 0).mean() >= 0.9, status
    np.testing.assert_array_equal(vst[status != 0], status[status != 0])
    for b in np.flatnonzero(status == 0):
        w1 = AN.single(w, b)
        cq = condense(problem_from_workload(w1, 0))
        slack = cq.h - cq.G @ U[b]
        # inactive rows carry EXACT zeros on every forward path (the adjoint reads the active set from them)
        assert (lam[b][slack > 1e-6] == 0.0).all(), (b, lam[b][slack > 1e-6])
        if vst[b] != 0:
            continue
        an = AN.vjp(w1, lam[b], gU[b], gX[b])
        for key in KEYS:
            ref = an[key]
            err = np.abs(g[key][b] - ref).max()
            assert err <= 1e-8 * max(1.0, np.abs(ref).max()), (b, key, err)
    assert (vst == 0).mean() >= 0.9, vst
    return plan, g


def test_vjp_config2_four_and_two_per_wavefront():
    from qpmpc_amd import _capi

    w = W.triple_integrator_batch(256)
    p4, g4 = _check_path(w, 256, 1, flags=_capi.OPT_FOUR_PER_WAVE)
    p2, g2 = _check_path(w, 256, 1, flags=_capi.OPT_TWO_PER_WAVE)
    # the same gradients whichever kernel solved the forward (where both found the same active set)
    same = ((p4.multipliers > 0) == (p2.multipliers > 0)).all(dim=1).cpu().numpy()
    same &= (p4.status == 0).cpu().numpy() & (p2.status == 0).cpu().numpy()
    assert same.mean() >= 0.9
    for key in KEYS:
        d = np.abs(g4[key] - g2[key]).max(axis=1)
        scale = np.maximum(1.0, np.abs(g4[key]).max(axis=1))
        assert (d[same] <= 1e-8 * scale[same]).all(), key


def test_vjp_wip_n50():
    w = W.wip_batch(64, N=50)
    _check_path(w, 64, 2)


def test_vjp_random_ltv_condensed_and_stagewise():
    from qpmpc_amd import _capi

    w = _random_ltv(3, 64, 6, 2, 24, 3)
    pc, gc = _check_path(w, 64, 3, flags=_capi.OPT_FORCE_CONDENSED)
    ps, gs = _check_path(w, 64, 3, formulation="stagewise")
    same = ((pc.multipliers > 0) == (ps.multipliers > 0)).all(dim=1).cpu().numpy()
    same &= (pc.status == 0).cpu().numpy() & (ps.status == 0).cpu().numpy()
    assert same.mean() >= 0.9
    for key in KEYS:
        d = np.abs(gc[key] - gs[key]).max(axis=1)
        scale = np.maximum(1.0, np.abs(gc[key]).max(axis=1))
        assert (d[same] <= 1e-8 * scale[same]).all(), key


def test_vjp_n128_workspace_carve():
    w = _random_ltv(4, 16, 4, 2, 64, 2)
    _check_path(w, 16, 4)


def _subset(w, idx):
    B = np.asarray(w["x0"]).shape[0]
    out = dict(w)
    for k, v in w.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k not in ("N",):
            out[k] = np.ascontiguousarray(v[idx])
    return out


@pytest.mark.parametrize("states", [False, True])
def test_gradcheck(states):
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(5, 40, 3, 2, 5, 2)
    w = _subset(w, AN.complementary(w, 4))
    bp = W.to_batch_problem(w)
    x0 = torch.as_tensor(w["x0"], device=bp.device).clone().requires_grad_()
    goal = torch.as_tensor(w["goal"], device=bp.device).clone().requires_grad_()
    e = torch.as_tensor(w["e"], device=bp.device).clone().requires_grad_()

    def f(x0, goal, e):
        U, X, _ = solve_mpc_batch_diff(bp, initial_state=x0, goal_state=goal, ineq_vector=e, states=states)
        return (U, X) if states else U

    assert torch.autograd.gradcheck(f, (x0, goal, e), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_unsolved_problems_get_zero_gradients():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(6, 32, 3, 2, 8, 2)
    for b in (3, 7, 20):  # two contradictory rows at step 0: c x + d u <= -1 and -(c x + d u) <= -1
        w["C"][b, 0, 1], w["D"][b, 0, 1] = -w["C"][b, 0, 0], -w["D"][b, 0, 0]
        w["e"][b, 0, :] = -1.0
    bp = W.to_batch_problem(w)
    x0 = torch.as_tensor(w["x0"], device=bp.device).clone().requires_grad_()
    goal = torch.as_tensor(w["goal"], device=bp.device).clone().requires_grad_()
    tg = torch.as_tensor(w["targets"], device=bp.device).clone().requires_grad_()
    e = torch.as_tensor(w["e"], device=bp.device).clone().requires_grad_()
    U, X, plan = solve_mpc_batch_diff(bp, x0, goal, tg, e, states=True, max_iter=3)
    (U.square().sum() + X.sum()).backward()
    torch.cuda.synchronize()
    status = plan.status.cpu().numpy()
    assert (status != 0).any() and (status == 0).any(), status
    assert (status[[3, 7, 20]] != 0).all()
    np.testing.assert_array_equal(plan.vjp_status.cpu().numpy()[status != 0], status[status != 0])
    bad = torch.as_tensor(status != 0, device=bp.device)
    for t in (x0, goal, tg, e):
        assert not torch.isnan(t.grad).any()
        assert (t.grad[bad] == 0).all()
    assert (x0.grad[~bad].abs().sum(dim=1) > 0).any()


def test_shared_goal_gets_the_batch_sum():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(8, 24, 3, 2, 6, 2)
    bp = W.to_batch_problem(w)
    g0 = np.asarray(w["goal"][0])
    shared = torch.as_tensor(g0, device=bp.device).clone().requires_grad_()
    per = torch.as_tensor(np.broadcast_to(g0, (24, 3)).copy(), device=bp.device).requires_grad_()
    U1, _, p1 = solve_mpc_batch_diff(bp, goal_state=shared)
    U2, _, p2 = solve_mpc_batch_diff(bp, goal_state=per)
    wts = torch.linspace(0.5, 1.5, U1.numel(), dtype=U1.dtype, device=U1.device).reshape(U1.shape)
    (U1 * wts).sum().backward()
    (U2 * wts).sum().backward()
    assert shared.grad.shape == shared.shape
    ref = per.grad.sum(dim=0)
    assert torch.allclose(shared.grad, ref, rtol=1e-12, atol=1e-12 * max(1.0, float(ref.abs().max())))


def test_float32_storage_gradients():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(9, 60, 3, 2, 6, 2)
    w = _subset(w, AN.complementary(w, 16))
    grads = {}
    for dt in (torch.float64, torch.float32):
        bp = W.to_batch_problem(w, dtype=dt)
        x0 = torch.as_tensor(w["x0"], dtype=dt, device=bp.device).clone().requires_grad_()
        goal = torch.as_tensor(w["goal"], dtype=dt, device=bp.device).clone().requires_grad_()
        tg = torch.as_tensor(w["targets"], dtype=dt, device=bp.device).clone().requires_grad_()
        U, X, plan = solve_mpc_batch_diff(bp, x0, goal, tg, states=True)
        (U.sum() + 0.5 * X.sum()).backward()
        assert (plan.status == 0).all()
        assert x0.grad.dtype == dt
        grads[dt] = [t.grad.double().cpu().numpy() for t in (x0, goal, tg)]
    for g64, g32 in zip(grads[torch.float64], grads[torch.float32]):
        scale = np.maximum(1.0, np.abs(g64).max(axis=1, keepdims=True))
        assert (np.abs(g32 - g64) <= 1e-3 * scale).all()


def test_envelope():
    torch = _torch()
    from qpmpc_amd import BackendError, solve_mpc_batch, solve_mpc_batch_diff

    w = _random_ltv(10, 8, 3, 2, 70, 2)  # n = 140 > 128
    bp = W.to_batch_problem(w)
    x0 = torch.as_tensor(w["x0"], device=bp.device).clone()
    with pytest.raises(BackendError):
        solve_mpc_batch_diff(bp, initial_state=x0.clone().requires_grad_())
    U, X, plan = solve_mpc_batch_diff(bp, initial_state=x0, states=True)
    ref = solve_mpc_batch(bp)
    assert U.grad_fn is None and X.grad_fn is None
    assert torch.equal(plan.U, ref.U) and torch.equal(plan.status, ref.status)
    assert torch.equal(X, ref.states)
